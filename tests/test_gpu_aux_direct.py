"""The per-image loss kernels of csrc/nnr_aux.hip alone -- nnr_aux_terms_fwd / _bwd through ctypes, raw output layouts included --
against the fp64 definition of tests/aux_ref.py, at the smallest shapes where they can go wrong: two blocks with a partial last one, SSIM
windows across the block boundary, a resize ratio that is no integer, hd == hr, 2-row and 2 x 2 grids, shards that cut rows and blocks.
Cases, inputs, upstream gradients and tolerances (8 x the fp32 rounding noise of the reference on the same case, capped at 1e-5
absolute for losses and 1e-4 of scale for gradients) come from aux_ref; tests/test_aux_ref_cpu.py holds the conditions they rest on.
Every deviation is printed before it is asserted (pytest -s shows them).
Measured on an MI355X, largest kernel-vs-fp64 deviation over all cases, as a fraction of the output's scale: losses 1.6e-6, g_d1_img /
g_d2_img per pixel 2.3e-6, d/d rel 1.8e-6, d/d scale2 5.2e-7, d/dK 6.5e-7, d/dKinv 4.1e-7, d/d aff 3.2e-7.  No gradient uses more than
0.26 of its tolerance; one loss (loss_rgb_s of shard_100_273_ssim, 4.2e-7) uses 0.88 of the smallest tolerance there is, 8 x half an
fp32 ulp.  The kernels are as close to fp64 as the fp32 reference is."""
import ctypes as C
import os
import sys

import pytest
import torch

import aux_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nope-nerf_amd"))
pytestmark = pytest.mark.gpu

SENTINEL = 12345.0      # fills g_rel_scale before the call and 8 floats behind it


def _flags(L, c):
    return ((L.AUX_RGBS if c.rgb_s else 0) | (L.AUX_PC if c.pc else 0) | (L.AUX_SCALE_PCS if c.scale_pcs else 0)
            | (L.AUX_DETACH_RGBS if c.detach else 0) | (L.AUX_SSIM if c.ssim else 0) | (L.AUX_GRAD_K if c.grad_k else 0)
            | (L.AUX_AFFINE if c.aff else 0) | (L.AUX_SHIFT_FIRST if c.shift_first else 0))


def _workspace(L, lib, cfg, dev):
    n_ws = lib.nnr_aux_workspace_floats(C.byref(cfg))
    assert n_ws > 0
    ws = torch.zeros(n_ws + 2, dtype=torch.float32, device=dev)
    return ws[(ws.data_ptr() % 8) // 4:]


def _device_inputs(c, dev):
    inp = R.case_inputs(c)
    flat = lambda k: inp[k].reshape(-1).contiguous().float().to(dev) if inp[k] is not None else None
    return inp, {k: flat(k) for k in inp}


def _abi(c, g_out=R.G_OUT, rounds=1):
    """Forward and backward of a case through the C ABI, `rounds` times on ONE workspace.  Returns one dict of CPU tensors per round."""
    from nnr import lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    inp, t = _device_inputs(c, dev)
    (hd, wd), (hr, wr) = c.maps, c.grid
    cfg = L.AuxCfg(hd, wd, hr, wr, R.NL, _flags(L, c), int(c.shard[0]), int(c.shard[1]))
    ws = _workspace(L, lib, cfg, dev)
    n_g = 44 if c.aff else (40 if c.grad_k else 16)
    g_up = torch.tensor(g_out, dtype=torch.float32, device=dev)
    fixed = (L.ptr(t["d1_img"]), L.ptr(t["d2_img"]), L.ptr(t["img1r"]) if c.rgb_s else None, L.ptr(t["img2r"]) if c.rgb_s else None,
             L.ptr(t["K"]), L.ptr(t["Kinv"]), L.ptr(t["rel"]), L.ptr(t["scale2"]), L.ptr(t["aff"]))
    results = []
    for _ in range(rounds):
        out = torch.full((4,), float("nan"), dtype=torch.float32, device=dev)
        L.check(lib.nnr_aux_terms_fwd(C.byref(cfg), *fixed, L.ptr(out), L.ptr(ws), L.stream()), "nnr_aux_terms_fwd")
        g_d1 = None if c.aff else torch.zeros(hd * wd, dtype=torch.float32, device=dev)
        g_d2 = None if c.aff else torch.zeros(hd * wd, dtype=torch.float32, device=dev)
        g_rs = torch.full((n_g + 8,), SENTINEL, dtype=torch.float32, device=dev)
        L.check(lib.nnr_aux_terms_bwd(C.byref(cfg), *fixed, L.ptr(g_up), L.ptr(g_d1), L.ptr(g_d2), L.ptr(g_rs), L.ptr(ws), L.stream()),
                "nnr_aux_terms_bwd")
        torch.cuda.synchronize()
        cpu = lambda x: None if x is None else x.cpu()
        results.append(dict(out=out.cpu(), g_d1=cpu(g_d1), g_d2=cpu(g_d2), g_rs=g_rs.cpu(), n_g=n_g))
    return inp, results


def _unpack(c, r):
    """The raw outputs of one ABI round as the outputs aux_ref names; the layout's zero slots and the floats behind it are checked here."""
    g_rs, n_g = r["g_rs"], r["n_g"]
    assert torch.equal(g_rs[n_g:], torch.full((8,), SENTINEL)), "the backward wrote behind g_rel_scale[%d]" % n_g
    assert torch.equal(g_rs[13:16], torch.zeros(3)), g_rs[13:16]
    (hd, wd) = c.maps
    got = dict(loss_pc=r["out"][0], loss_rgb_s=r["out"][1], n_valid=float(r["out"][2]), g_rel=g_rs[0:12], g_scale2=g_rs[12])
    assert float(r["out"][3]) == 0.0      # (not NNR_AUX_WEIGHTED)
    if c.grad_k:
        got["g_K"], got["g_Kinv"] = g_rs[16:28], g_rs[28:40]
    if c.aff:
        got["g_aff"] = g_rs[40:44]
    else:
        got["g_d1"], got["g_d2"] = r["g_d1"].view(hd, wd), r["g_d2"].view(hd, wd)
    return got


def _depth_zero_pixels(c, inp, got):
    """g_d*_img must be exactly 0 at every pixel the grid does not sample and at every clamped pixel."""
    (hd, wd), (hr, wr) = c.maps, c.grid
    src = R.nearest_indices(hd, wd, hr, wr)
    for k, d in (("g_d1", inp["d1_img"]), ("g_d2", inp["d2_img"])):
        live = torch.zeros(hd * wd, dtype=torch.bool)
        live[src] = True
        live[src[d.reshape(-1)[src] < R.NL]] = False
        g = got[k].reshape(-1)
        assert not bool(torch.isnan(g).any()), k
        assert torch.equal(g[~live], torch.zeros(int((~live).sum()))), (k, "gradient at an unsampled or clamped pixel")


MAX_DEV = {}      # output -> the largest deviation / tolerance seen in this session (printed by the last test)


def _compare(name, got, ref, tol_case=None):
    tol_case = tol_case or name
    assert got["n_valid"] == float(ref["n_valid"]), (got["n_valid"], ref["n_valid"])
    bad = []
    for k in R.OUTPUTS:
        if k not in got or ref.get(k) is None:
            continue
        want, have = ref[k].double(), got[k].double()
        assert not bool(torch.isnan(have).any()), (name, k)
        scale = float(want.abs().max())
        dev = float((have - want).abs().max())
        if scale == 0.0:
            print("%-20s %-10s reference 0, kernel max |.| %.3e" % (name, k, dev))
            if dev != 0.0:
                bad.append((k, dev, "must be exactly 0"))
            continue
        tol = R.tolerance(tol_case, k) * scale
        if k.startswith("loss"):
            tol = min(tol, 1e-5)
        print("%-20s %-10s dev/scale %.3e  tolerance/scale %.3e  (%.2f of it)" % (name, k, dev / scale, tol / scale, dev / tol))
        MAX_DEV[k] = max(MAX_DEV.get(k, (0.0, 0.0, "")), (dev / scale, dev / tol, name))
        if dev > tol:
            bad.append((k, dev / scale, tol / scale))
    assert not bad, (name, bad)


_GOT = {}      # case name -> (inputs, unpacked outputs) of its ABI run: the shard tests add up what the case tests produced


def _run(name):
    if name not in _GOT:
        c = R.CASES[name]
        inp, (r,) = _abi(c)
        _GOT[name] = (inp, _unpack(c, r))
    return _GOT[name]


_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = R.evaluate(R.CASES[name])
    return _REF[name]


ABI_CASES = [n for n, c in R.CASES.items() if c.via == "abi"]


@pytest.mark.parametrize("name", ABI_CASES)
def test_kernels_equal_the_fp64_reference(name):
    c = R.CASES[name]
    inp, got = _run(name)
    if not c.aff:
        _depth_zero_pixels(c, inp, got)
    _compare(name, got, _ref(name))
    if name == "no_valid":
        assert float(got["loss_rgb_s"]) == 0.0 and got["n_valid"] == 0.0


@pytest.mark.parametrize("ssim", ["", "_ssim"])
def test_two_shards_add_up_to_the_unsharded_result(ssim):
    whole = "ssim" if ssim else "both"
    (_, a), (_, b) = _run("shard_0_100" + ssim), _run("shard_100_273" + ssim)
    total = {k: (a[k] + b[k]) for k in a if k != "n_valid"}
    total["n_valid"] = a["n_valid"]
    assert a["n_valid"] == b["n_valid"]      # the normaliser is global
    _compare("halves of " + whole, total, _ref(whole), tol_case=whole)


@pytest.mark.parametrize("flags", [dict(pc=False), dict(pc=False, ssim=True), dict(ssim=True)])
def test_no_valid_reprojection_leaves_exact_zeros(flags):
    """acc[1] == 0: out[1] and out[2] exactly 0, every re-projection gradient exactly 0, nothing NaN -- with points in front of the second
    camera among those that project outside, and the point-cloud part (where it is on) as the reference has it."""
    c = R.CASES["no_valid"]._replace(**flags)
    inp, (r,) = _abi(c)
    got = _unpack(c, r)
    assert float(got["loss_rgb_s"]) == 0.0 and got["n_valid"] == 0.0
    ref = R.evaluate(c)
    assert ref["n_valid"] == 0
    _depth_zero_pixels(c, inp, got)
    if not c.pc:
        for k in ("g_d1", "g_d2", "g_rel", "g_scale2"):
            assert not bool(got[k].double().abs().max() > 0), k
        assert float(got["loss_pc"]) == 0.0
    else:
        _compare("no_valid", got, ref)      # (the re-projection adds exactly 0 in the reference too: the tolerances of the case hold)


def test_mats_layout_through_the_python_binding():
    """NNR_AUX_AFFINE | NNR_AUX_MATS_GRAD: rel, the distortion pairs and scale2 read in place from the 56-float block, one gradient in that layout."""
    from nnr import aux as nnr_aux
    c = R.CASES["mats"]
    dev = torch.device("cuda", 0)
    inp = R.case_inputs(c)
    mats = torch.full((56,), 7.0)
    mats[34:50], mats[50:54], mats[54] = inp["rel"].reshape(16), inp["aff"], inp["scale2"]
    mats = mats.to(dev).requires_grad_(True)
    b = lambda k: inp[k][None].to(dev)
    l_pc, l_rgbs, n_valid = nnr_aux.aux_terms(b("d1_img")[None], b("d2_img")[None], None, None, b("img1r"), b("img2r"), b("K"), b("Kinv"), c.grid, R.NL,
                                              mats=mats)
    (R.G_OUT[0] * l_pc + R.G_OUT[1] * l_rgbs).backward()
    g = mats.grad.cpu()
    live = torch.zeros(56, dtype=torch.bool)
    live[34:46] = live[50:55] = True
    assert torch.equal(g[~live], torch.zeros(int((~live).sum()))), g
    got = dict(loss_pc=l_pc.detach().cpu(), loss_rgb_s=l_rgbs.detach().cpu(), n_valid=float(n_valid.detach()), g_rel=g[34:46], g_aff=g[50:54], g_scale2=g[54])
    _compare("mats", got, _ref("mats"))


@pytest.mark.parametrize("name", ["weighted_only", "weighted_mixed"])
def test_weighted_sum_through_the_python_binding(name):
    """NNR_AUX_WEIGHTED: out[3] = w_pc out[0] + w_rgbs out[1] as fp32 products and sum; its one upstream gradient alone, and mixed with
    gradients of out[0] and out[1]."""
    from nnr import aux as nnr_aux
    c = R.CASES[name]
    dev = torch.device("cuda", 0)
    inp = R.case_inputs(c)
    leaf = lambda k, shape: inp[k].reshape(shape).to(dev).requires_grad_(True)
    (hd, wd) = c.maps
    d1, d2, rel, s2 = leaf("d1_img", (1, 1, hd, wd)), leaf("d2_img", (1, 1, hd, wd)), leaf("rel", (1, 4, 4)), leaf("scale2", ())
    b = lambda k: inp[k][None].to(dev)
    out = nnr_aux.aux_terms(d1, d2, rel, s2, b("img1r"), b("img2r"), b("K"), b("Kinv"), c.grid, R.NL, weights=c.weights)
    assert len(out) == 4
    o = [x.detach().cpu() for x in out]
    w = torch.tensor(c.weights, dtype=torch.float32)
    assert float(o[3]) == float(w[0] * o[0] + w[1] * o[1])
    loss = c.g_w * out[3]
    if c.extra != (0.0, 0.0):
        loss = loss + c.extra[0] * out[0] + c.extra[1] * out[1]
    loss.backward()
    got = dict(loss_pc=o[0], loss_rgb_s=o[1], n_valid=float(o[2]), g_d1=d1.grad.cpu().view(hd, wd), g_d2=d2.grad.cpu().view(hd, wd),
               g_rel=rel.grad.cpu().reshape(16)[:12], g_scale2=s2.grad.cpu())
    assert torch.equal(rel.grad.cpu().reshape(16)[12:], torch.zeros(4))
    _depth_zero_pixels(c, inp, got)
    _compare(name, got, _ref(name))


def test_a_term_out_of_range_poisons_the_fixed_point_accumulator():
    """An upstream gradient of 1e9 makes every point-cloud term exceed the accumulators' range: fix_add must poison, not wrap, so d/d rel,
    d/d scale2 and the depth gradient of every sampled, unclamped pixel are NaN.  A finite value at any of those places fails."""
    c = R.CASES["both"]
    inp, (r,) = _abi(c, g_out=(1e9, R.G_OUT[1]))
    assert bool(torch.isnan(r["g_rs"][0:13]).all()), r["g_rs"][0:13]
    (hd, wd), (hr, wr) = c.maps, c.grid
    src = R.nearest_indices(hd, wd, hr, wr)
    for k, d in (("g_d1", inp["d1_img"]), ("g_d2", inp["d2_img"])):
        receives = src[d.reshape(-1)[src] >= R.NL]
        assert receives.numel() > 200
        assert bool(torch.isnan(r[k][receives]).all()), (k, int(torch.isfinite(r[k][receives]).sum()), "finite values")


def test_second_forward_backward_on_one_workspace_repeats_the_first_bit_for_bit():
    """The forward re-zeroes the backward's accumulators, the ticket of the last-block finish and the heavy-tile flags."""
    c = R.CASES["ssim"]._replace(scale_pcs=False)
    _, (a, b) = _abi(c, rounds=2)
    for k in ("out", "g_d1", "g_d2", "g_rs"):
        assert not bool(torch.isnan(a[k]).any()), k
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert float(a["out"][0]) > 0 and float(a["out"][1]) > 0 and float(a["g_d1"].abs().max()) > 0


def test_refusals_come_before_any_launch():
    from nnr import lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    base = dict(hd=52, wd=84, hr=13, wr=21, flags=L.AUX_PC | L.AUX_RGBS | L.AUX_SCALE_PCS, lo=0, hi=0)

    def cfg(**kw):
        a = dict(base, **kw)
        return L.AuxCfg(a["hd"], a["wd"], a["hr"], a["wr"], R.NL, a["flags"], a["lo"], a["hi"])

    floats = lambda **kw: lib.nnr_aux_workspace_floats(C.byref(cfg(**kw)))
    assert floats() > 0
    assert floats(hr=1) == 0
    assert floats(hr=53) == 0                 # hr > hd
    assert floats(wr=85) == 0                 # wr > wd
    assert floats(lo=0, hi=274) == 0          # shard_hi > S
    assert floats(lo=100, hi=99) == 0         # shard_hi < shard_lo
    assert floats(flags=base["flags"] | L.AUX_MATS_GRAD) == 0                                   # MATS_GRAD without AFFINE
    assert floats(flags=base["flags"] | L.AUX_MATS_GRAD | L.AUX_AFFINE | L.AUX_GRAD_K) == 0      # MATS_GRAD with GRAD_K
    assert floats(flags=base["flags"] | L.AUX_MATS_GRAD | L.AUX_AFFINE) > 0

    c = R.CASES["both"]
    _, t = _device_inputs(c, dev)
    aff = torch.tensor(R.AFF, device=dev)
    out = torch.full((4,), SENTINEL, device=dev)

    def fwd(flags, ws, **over):
        a = dict(d1=t["d1_img"], d2=t["d2_img"], i1=t["img1r"], i2=t["img2r"], s2=t["scale2"], aff=None)
        a.update(over)
        k = cfg(flags=flags)
        return lib.nnr_aux_terms_fwd(C.byref(k), L.ptr(a["d1"]), L.ptr(a["d2"]), L.ptr(a["i1"]), L.ptr(a["i2"]), L.ptr(t["K"]), L.ptr(t["Kinv"]),
                                     L.ptr(t["rel"]), L.ptr(a["s2"]), L.ptr(a["aff"]), L.ptr(out), L.ptr(ws), L.stream())

    f = base["flags"]
    ws = _workspace(L, lib, cfg(flags=f | L.AUX_AFFINE | L.AUX_SSIM), dev)      # large enough for every configuration below
    BADCFG, ALIGN = -1, -3
    assert fwd(f | L.AUX_AFFINE, ws) == BADCFG              # AFFINE without aff
    assert fwd(f, ws, aff=aff) == BADCFG                    # aff without AFFINE
    assert fwd(f, ws, s2=None) == BADCFG                    # SCALE_PCS without scale2
    assert fwd(f, ws, i1=None) == BADCFG and fwd(f, ws, i2=None) == BADCFG      # RGBS without images
    assert fwd(f, ws[1:]) == ALIGN                          # a workspace offset by 4 bytes
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((4,), SENTINEL)) and float(ws.abs().max()) == 0.0      # nothing ran
    assert fwd(f, ws) == 0                                  # and the same arguments without the fault are accepted
    torch.cuda.synchronize()
    assert float(out[0]) > 0


def test_report_the_largest_deviations():
    """Not a check of its own: the largest deviation of each output over the cases above, as a fraction of scale and of its tolerance."""
    for k, (rel, frac, name) in sorted(MAX_DEV.items()):
        print("largest %-10s %.3e of scale, %.2f of its tolerance (%s)" % (k, rel, frac, name))
