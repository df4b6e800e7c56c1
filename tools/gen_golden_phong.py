"""Golden vectors for the phong geometry renderer (reference model/rendering.py:202-418: phong_renderer, ray_marching, secant).

TEST INFRASTRUCTURE; authoring container only (needs the reference checkout, like oracle/gen_golden*.py):   python tools/gen_golden_phong.py

A randomly initialised network is degenerate for this renderer (val_0 >= 0 nearly everywhere), so a D = 128 and a D = 256 network are
first fitted on the CPU, from a fixed seed, to an analytic shape -- the union of a sphere and a box, raw ~ k * (signed distance inside),
so that raw = 0 (occ = 0.5 with softplus) is the surface -- by a few hundred Adam steps.  The fitted weights are then rounded to int8 with
a power-of-two scale per output row (exact in fp32; the D = 256 fixture stays under 1 MiB), and the rounded network is what the
REFERENCE renders, on the CPU (torch.Tensor.cuda patched to the identity), over 54 x 96 pixels in chunks of 1024, from two cameras: one
outside the radius-4 sphere (its corner rays miss it) and one inside the shape (d = 0 on every ray).

Stored per width in tests/golden/phong_d{128,256}.npz: the int8 weights + row exponents + fp32 biases, K / world_mat per camera, and per
camera d (the reference's ray_marching output), rgb, rgb_surf, the PNG of the frame (its bytes) and margin = min_j |val_j| per ray."""
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg          # noqa: E402

H, W, CHUNK, N_STEPS = 54, 96, 1024, 512
LAYERS = ("layers0.0", "layers0.2", "layers0.4", "layers0.6", "layers1.0", "layers1.2", "layers1.4", "layers1.6", "fc_density",
          "fc_feature", "rgb_layers.0", "fc_rgb")


def inside_distance(p):
    """> 0 inside the union of a sphere (centre 0, radius 1.2) and a box (centre (1.2, 0.4, 0.3), half extents (0.6, 0.5, 0.7))."""
    s = 1.2 - p.norm(dim=-1)
    q = (p - torch.tensor([1.2, 0.4, 0.3])).abs() - torch.tensor([0.6, 0.5, 0.7])
    box = -(q.clamp_min(0).norm(dim=-1) + q.max(dim=-1).values.clamp_max(0))
    return torch.maximum(s, box)


def fit(net, steps, seed):
    g = torch.Generator().manual_seed(seed)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    for _ in range(steps):
        far = (torch.rand(1024, 3, generator=g) * 2 - 1) * 4.0
        near = (torch.rand(1024, 3, generator=g) * 2 - 1) * 2.2
        p = torch.cat([far, near])
        target = (8.0 * inside_distance(p)).clamp(-4, 4)
        _, raw = net.infer_occ(p)
        loss = ((raw[:, 0] - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return float(loss)


def quantise(net):
    """Every weight matrix to int8 x 2^e per output row (in place); returns the stored arrays."""
    out = {}
    sd = net.state_dict()
    with torch.no_grad():
        for name in LAYERS:
            w = sd[name + ".weight"]
            e = torch.ceil(torch.log2(w.abs().amax(dim=1).clamp_min(1e-30) / 127.0))
            q = torch.round(w / torch.exp2(e)[:, None]).clamp(-127, 127)
            w.copy_(q * torch.exp2(e)[:, None])
            out[name + ".q"] = q.to(torch.int8).numpy()
            out[name + ".e"] = e.to(torch.int8).numpy()
            out[name + ".bias"] = sd[name + ".bias"].numpy().copy()
    return out


def look_at(pos, target):
    pos, target = torch.tensor(pos), torch.tensor(target)
    back = pos - target
    back = back / back.norm()
    right = torch.linalg.cross(torch.tensor([0., 1., 0.]), back)
    right = right / right.norm()
    up = torch.linalg.cross(back, right)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, back, pos
    return c2w


CAMERAS = (((0.3, 0.5, 4.5), (0.3, 0.1, 0.0)),      # outside the radius-4 sphere: the corner rays miss it
           ((0.1, -0.2, 0.3), (1.0, 0.0, 0.0)))     # inside the shape: val_0 >= 0, d = 0 everywhere


def main():
    ref = gg.import_reference()
    torch.set_num_threads(8)
    from model.common import arange_pixels
    from PIL import Image
    for hidden in (128, 256):
        cfg = gg.base_cfg(hidden)
        torch.manual_seed(hidden)
        net = ref.OfficialStaticNerf(cfg)
        loss = fit(net, 400, seed=hidden + 1)
        store = quantise(net)
        renderer = ref.Renderer(net, cfg["rendering"], device=torch.device("cpu"))
        K = torch.tensor([[[0.6, 0, 0, 0], [0, -0.6, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]]], dtype=torch.float32)
        pixels = arange_pixels(resolution=(H, W))[1]
        rec = {}
        orig_march, orig_fwd = renderer.ray_marching, net.forward

        def march(*a, **k):
            d = orig_march(*a, **k)
            rec["d"].append(d[0].clone())
            return d

        def fwd(p, *a, **k):
            y = orig_fwd(p, *a, **k)
            if k.get("only_occupancy") and p.shape[-2] == rec["n"] * N_STEPS:      # the proposals of one ray_marching call
                rec["margin"].append((y.view(-1, N_STEPS) - 0.5).abs().amin(dim=1))
            return y

        renderer.ray_marching, net.forward = march, fwd
        for ci, (pos, target) in enumerate(CAMERAS):
            c2w = look_at(pos, target)
            world_mat = torch.inverse(c2w).unsqueeze(0)
            rec.update(d=[], margin=[])
            rgb, rgb_surf = [], []
            with torch.no_grad():
                for pix in torch.split(pixels, CHUNK, dim=1):
                    rec["n"] = pix.shape[1]
                    out = renderer.phong_renderer(pix, K, world_mat, torch.eye(4).unsqueeze(0), it=0)
                    rgb.append(out["rgb"][0])
                    rgb_surf.append(out["rgb_surf"][0])
            rgb, rgb_surf = torch.cat(rgb), torch.cat(rgb_surf)
            d, margin = torch.cat(rec["d"]), torch.cat(rec["margin"])
            assert d.shape == (H * W,) and margin.shape == (H * W,)
            img = (rgb.view(H, W, 3).numpy() * 255).astype(np.uint8)
            buf = io.BytesIO()
            Image.fromarray(img).convert("RGB").save(buf, format="png")
            store.update({"K%d" % ci: K.numpy(), "world_mat%d" % ci: world_mat.numpy(), "d%d" % ci: d.numpy(),
                          "rgb%d" % ci: rgb.numpy(), "rgb_surf%d" % ci: rgb_surf.numpy(), "margin%d" % ci: margin.numpy(),
                          "png%d" % ci: np.frombuffer(buf.getvalue(), dtype=np.uint8)})
            hits = torch.isfinite(d) & (d != 0)
            print("D=%d camera %d: %d hits, %d misses, %d zero; fit loss %.4f" % (hidden, ci, int(hits.sum()), int(torch.isinf(d).sum()),
                                                                                   int((d == 0).sum()), loss))
        store["hidden"] = np.array(hidden)
        path = os.path.join(ROOT, "tests", "golden", "phong_d%d.npz" % hidden)
        np.savez_compressed(path, **store)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
