"""Timings of hierarchical sampling (rendering.num_fine: model/rendering.py; the resampling kernel nnr_resample.hip).

    python tools/time_resample.py --out DIR          # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_resample.py --inner            # the workload the trace pass runs (also usable on its own)

Reports (JSON lines, and DIR/time_resample.json), D = 256, fp32 (two-term fp16) products:
  * resample_kernel at 1024 rays (64 coarse + 128 fine) and at 4096 rays (64 + 64), beside the coarse inference forward that feeds it
    (nnr.render_rays under no_grad with per-sample outputs) and a torch restatement of the definition in fp32 on the device -- the
    bar: the kernel takes no longer than the coarse forward of the same trace;
  * propose_f16_kernel (rendering.proposal: 'density', nnr.ops.propose) on the same inputs at D = 256 and D = 128 -- the bar: no slower than
    the coarse forward + resample_kernel of the same trace (at D = 128 beside a coarse forward of that width);
  * Trainer.train_step (front end, render, losses, backward, Adam for field / poses / distortion; rgb + depth losses) on a synthetic
    scene of tools/scene_writer.py at 1024 rays: 64 + 128 in both proposal modes against 192 uniform samples and 64 uniform samples.
The trace pass gives the per-kernel figures (the events include launch gaps); both go to DIR.  Exit status: the trace pass's."""
import argparse
import json
import os
import signal
import subprocess
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "nope-nerf_amd"), HERE):
    sys.path.insert(0, p)


def torch_resample(alpha, z, xi, n_fine):
    """The definition of nnr_resample (include/nnr.h) in torch ops on the tensors' device, fp32: the yardstick for what the kernel replaces."""
    R, C = alpha.shape
    dev = alpha.device
    keep = (1 - alpha) + 1e-6
    T = torch.cumprod(torch.cat([torch.ones(R, 1, device=dev), keep[:, :-1]], dim=1), dim=1)
    m = 0.5 * (z[:, :-1] + z[:, 1:])
    p = (alpha * T)[:, 1:-1] + 1e-5
    cdf = torch.cat([torch.zeros(R, 1, device=dev), torch.cumsum(p / p.sum(dim=1, keepdim=True), dim=1)], dim=1)
    u = ((torch.arange(n_fine, device=dev, dtype=torch.float32).unsqueeze(0) + xi) / n_fine).contiguous()
    i = torch.searchsorted(cdf.contiguous(), u, right=True)
    below, above = (i - 1).clamp(min=0), i.clamp(max=C - 2)
    cb, mb, ma = cdf.gather(1, below), m.gather(1, below), m.gather(1, above)
    den = cdf.gather(1, above) - cb
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    s = torch.minimum(torch.maximum(mb + (u - cb) / den * (ma - mb), mb), ma).contiguous()
    pos_c = torch.arange(C, device=dev).unsqueeze(0) + torch.searchsorted(s, z.contiguous(), right=False)
    pos_f = torch.arange(n_fine, device=dev).unsqueeze(0) + torch.searchsorted(z.contiguous(), s, right=True)
    return torch.empty(R, C + n_fine, device=dev).scatter_(1, pos_c, z).scatter_(1, pos_f, s)


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


def _renderer(num_points, num_fine, hidden=256):
    import model as mdl
    import train_scene
    cfg = train_scene.scene_cfg("", "", n_samples=num_points, hidden=hidden, num_fine=num_fine)
    torch.manual_seed(0)
    net = mdl.OfficialStaticNerf(cfg)
    return mdl.Renderer(net, cfg['rendering'], device=torch.device('cuda'))


def _train_step_ms(scene_dir, n_samples, num_fine, steps=30, proposal=None):
    import dataloading as dl
    import train_scene
    cfg = train_scene.scene_cfg(scene_dir, "synthetic", n_rays=1024, n_samples=n_samples, hidden=256, num_fine=num_fine, aux=False,
                                sample_rate=10 ** 6, proposal=proposal)
    torch.manual_seed(0)
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=True)
    trainer, _, _ = train_scene.build(cfg, torch.device('cuda'), fields["img"].N_imgs)
    batches = list(loader)
    it = [0]

    def step():
        trainer.train_step(batches[it[0] % len(batches)], it[0], 0, 10 ** 6, None)
        it[0] += 1
    ms = _events(step, steps, warm=5)
    trainer.flush_nan_check()
    return ms


def workload(report):
    import nnr
    import nnr.ops as ops
    import scene_writer
    dev = torch.device('cuda')
    renderer = _renderer(64, 128)
    net = renderer.model
    kw = dict(hidden=256, dist_alpha=False, white_bg=False, relu_sigma=False)
    g = torch.Generator().manual_seed(1)
    for R, C, F in ((1024, 64, 128), (4096, 64, 64)):
        d = torch.randn(R, 3, generator=g)
        d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
        o = (torch.randn(1, 3, generator=g) * 0.1).expand(R, 3).contiguous().to(dev)
        v = (-d).contiguous()
        z_lo, z_hi = renderer._z_tables(C, 0.01, 10., True, dev)
        jit = torch.rand(R, C, device=dev)
        xi = torch.rand(R, F, device=dev)
        with torch.no_grad():
            coarse = lambda: nnr.render_rays(o, d, v, z_lo, z_hi, jit, net.weights(), net.biases(), samples=True, **kw)
            _, _, alpha, z = coarse()
            tag = "%dx(%d+%d)" % (R, C, F)
            report("coarse_forward_" + tag, ms=_events(coarse, 20))
            report("resample_kernel_" + tag, ms=_events(lambda: ops.resample(alpha, z, xi, F), 50), bytes_moved=4 * R * (2 * C + F + C + F))
            report("torch_restatement_fp32_" + tag, ms=_events(lambda: torch_resample(alpha, z, xi, F), 5, warm=1))
            for hidden, n in ((256, net), (128, _renderer(C, F, hidden=128).model)):      # the fused proposal kernel: one launch for the two above
                fused = lambda: ops.propose(o, d, z_lo, z_hi, jit, xi, F, n.weights(), n.biases(), hidden=hidden, dist_alpha=False, relu_sigma=False)
                report("propose_kernel_d%d_%s" % (hidden, tag), ms=_events(fused, 20))
                if hidden == 128:
                    c128 = lambda: nnr.render_rays(o, d, v, z_lo, z_hi, jit, n.weights(), n.biases(), samples=True, **dict(kw, hidden=128))
                    report("coarse_forward_d128_" + tag, ms=_events(c128, 20))
    with tempfile.TemporaryDirectory() as scene_dir:
        scene_writer.write_scene(scene_dir, scene="synthetic", frames=8, size=(60, 80), seed=0)
        for name, n_samples, num_fine, proposal in (("64+128", 64, 128, None), ("64+128_density", 64, 128, "density"), ("192_uniform", 192, 0, None),
                                                    ("64_uniform", 64, 0, None)):
            report("train_step_1024_" + name, ms=_train_step_ms(scene_dir, n_samples, num_fine, proposal=proposal))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_resample.json and the trace (required unless --inner)")
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
        return 0
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_resample.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(args.out, "trace"), "-o", "resample", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    # (its own process group: on a timeout the whole group goes, the Python grandchild that holds the GPU included)
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = child.communicate(timeout=500)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        out, _ = child.communicate()
        print("rocprofv3 pass timed out and was killed")
    print("rocprofv3 exit", child.returncode, out[-2000:] if child.returncode else "")
    return 0 if child.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
