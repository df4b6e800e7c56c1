"""Timings of the phong geometry renderer (model/rendering.py: Renderer.phong_renderer; the march kernel nnr_march_f16.hip).

    python tools/time_phong.py --out DIR             # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_phong.py --inner               # the workload the trace pass runs (also usable on its own)

Reports (JSON lines, and DIR/time_phong.json):
  * march_f16_kernel<256>: ns per sample at 1024 rays x 512 steps, D = 256 (ray mode, device events around nnr_ray_march with no secant
    step: the march launch + the tiny finish launch), beside the inference forward mlp_fwd_f16_kernel<256, false> at the bench shape
    (1024 x 192, fused compositing) -- the bar: the march's ns per sample at most the inference forward's;
  * one 54 x 96 geometry frame (render_visdata's phong loop: 6 calls of 1024 pixels) and one 540 x 960 frame (output_geo: 507 calls);
  * the torch restatement of the reference algorithm (tests/test_gpu_phong.py) at 1024 x 512, D = 256, fp32 matmuls.
The trace pass gives the per-kernel figures (the events include launch gaps); both go to DIR."""
import argparse
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in ("nope-nerf_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def _renderer(hidden=256):
    import test_gpu_phong as tp
    return tp._renderer(hidden)


def _events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps      # ms


def workload(report):
    import nnr
    import nnr.ops as ops
    import test_gpu_phong as tp
    from nnr import camera
    renderer, cfg, G = _renderer(256)
    net = renderer.model
    K, Wm, S = tp._cam(G, 0)
    R, N = 1024, 512
    pix = tp._pixels()[:, :R].contiguous()
    o, ray, _, _, _, _ = camera.ray_setup(pix, None, K, Wm, S, True, True)
    t = torch.linspace(0, 1, N).cuda()
    march = lambda: ops.ray_march(o, ray, t, net.weights(), net.biases(), hidden=256, radius=4.0, n_secant=0)
    ms_march = _events(march, 20)
    report("march_1024x512_d256", ms=ms_march, ns_per_sample=ms_march * 1e6 / (R * N))
    full = lambda: ops.ray_march(o, ray, t, net.weights(), net.biases(), hidden=256, radius=4.0, n_secant=8)
    report("march_plus_8_secant_1024_d256", ms=_events(full, 20))
    # the inference forward at the bench shape (fused compositing: what bench.py's inference kernel runs)
    Rb, Nb = 1024, 192
    z = torch.linspace(0.01, 10, Nb).cuda()
    ob, db = o[:Rb].contiguous(), ray[:Rb].contiguous()
    vb = (-db).contiguous()
    with torch.no_grad():
        fwd = lambda: nnr.render_rays(ob, db, vb, z, z, None, net.weights(), net.biases(), hidden=256, dist_alpha=False, white_bg=False,
                                      relu_sigma=False, samples=False)
        ms_fwd = _events(fwd, 20)
    report("infer_fwd_1024x192_d256", ms=ms_fwd, ns_per_sample=ms_fwd * 1e6 / (Rb * Nb))
    # whole frames through the renderer (the loops of render_visdata / generate_images)
    from model.common import arange_pixels

    def frame(h, w):
        px = arange_pixels(resolution=(h, w))[1].cuda()
        with torch.no_grad():
            for chunk in torch.split(px, 1024, dim=1):
                renderer.phong_renderer(chunk, K, Wm, S, it=0)
    report("frame_54x96_d256", ms=_events(lambda: frame(54, 96), 5, warm=1))
    report("frame_540x960_d256", ms=_events(lambda: frame(540, 960), 1, warm=1))
    # the torch restatement for comparison
    torch.backends.cuda.matmul.allow_tf32 = False
    with torch.no_grad():
        report("torch_restatement_1024x512_d256", ms=_events(lambda: tp._restated_march(net, o, ray, N, 4.0), 3, warm=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_phong.json and the trace (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_phong.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(args.out, "trace"), "-o", "phong", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    print("rocprofv3 exit", r.returncode, r.stderr[-2000:] if r.returncode else "")


if __name__ == "__main__":
    main()
