"""The refusal table of the frozen-field family and the sparse inference render: every return code that is decided on the host, recorded once
and replayed by tests/test_frozen_refusals_cpu.py against the built library.

    python oracle/frozen_refusals.py        # writes tests/golden/frozen_refusals.json from the library as it is built now

The eight entry points of include/nnr_frozen.h and include/nnr_frozen_sparse.h and nnr_render_sparse (include/nnr_sparse.h) are called with
fake, 16-byte aligned device pointers and real host grid arrays, as tests/test_frozen_sparse_cpu.py calls them.  No case may get as far as a
launch (the replay also runs on machines with a GPU): every call of a launching entry point carries a PROBE, one required pointer that the
entry point checks for alignment in its last stage, off by two bytes -- the second of two where the case itself sets or nulls the first.
A call whose other arguments are all in order therefore answers NNR_E_ALIGN, and a code other than that says which earlier refusal won:
cases with two defects pin the order of the refusals.  table() is the one statement of the cases; the record is {entry point: {case name: code}}, for the workspace
functions {case name: floats} and {case name: [offset, pitch]}.  Needs no GPU."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "frozen_refusals.json")

DIST_ALPHA, WHITE_BG, RELU_SIGMA, TRAIN, BF16, SPLIT3, SPLIT2 = 1, 2, 4, 8, 16, 32, 64
NAN, INF = float("nan"), float("inf")

FROZEN_FWD = ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter", "packed", "rgb", "dist", "opt_alpha", "opt_z", "ws")
FROZEN_BWD = ("packed", "d_rgb", "d_dist", "d_pts_o", "d_pts_d", "d_view", "ws")
SPARSE_FWD = ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter", "grid_lo", "grid_inv_step", "grid_dims", "bits", "packed", "rgb", "dist",
              "opt_alpha", "opt_z", "opt_count", "opt_live", "opt_n_live", "ws")
RENDER_SPARSE = ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter", "grid_lo", "grid_inv_step", "grid_dims", "bits", "packed", "out",
                 "opt_count", "opt_cell", "opt_out4")
GRID = ("grid_lo", "grid_inv_step", "grid_dims")
NEED = TRAIN | SPLIT3 | SPLIT2
# entry point -> (parameter names, the flags of a cfg it takes, the probes, {pointer: the alignment it is held to})
LAUNCHING = {"nnr_frozen_fwd": (FROZEN_FWD, NEED, ("ws", "packed"), {"packed": 16, "ws": 16}),
             "nnr_frozen_bwd": (FROZEN_BWD, NEED, ("ws", "packed"), {"packed": 16, "ws": 16}),
             "nnr_frozen_sparse_fwd": (SPARSE_FWD, NEED, ("ws", "packed"), {"packed": 16, "ws": 16, "bits": 4, "opt_count": 4, "opt_live": 4, "opt_n_live": 4}),
             "nnr_frozen_sparse_bwd": (FROZEN_BWD, NEED, ("ws", "packed"), {"packed": 16, "ws": 16}),
             "nnr_render_sparse": (RENDER_SPARSE, SPLIT3 | SPLIT2, ("out", "packed"),
                                   dict({"packed": 16}, **{k: 4 for k in RENDER_SPARSE if k not in GRID + ("packed",)}))}
GOOD = (5, 130, 128)      # rays, samples, hidden: a cfg every entry point takes


def cfg_variants(base):
    """name -> (n_rays, n_samples, hidden, flags) or None (a null cfg)"""
    R, N, D = GOOD
    v = {"good": (R, N, D, base), "null": None, "switches": (R, N, D, base | DIST_ALPHA | WHITE_BG | RELU_SIGMA),
         "bf16": (R, N, D, base | BF16), "train_flipped": (R, N, D, base ^ TRAIN),
         "no_split3": (R, N, D, base & ~SPLIT3), "no_split2": (R, N, D, base & ~SPLIT2), "no_split": (R, N, D, base & ~(SPLIT3 | SPLIT2)),
         # R N rounded up to whole workgroups exceeds 2^31 - 1: at 1024 and at 256 samples per ray
         "s_pad_over_int32_n1024": (2 ** 21 + 1, 1024, 256, base), "s_pad_over_int32_n256": (2 ** 23 + 1, 256, 256, base),
         "s_pad_is_2_31": (2 ** 21, 1024, 256, base), "s_pad_under_2_31": (2 ** 21 - 1, 1024, 256, base)}
    for h in (64, 128, 192, 256):
        v["hidden_%d" % h] = (R, N, h, base)
    for n in (-1, 0, 1, 256, 257, 1024, 1025):
        v["n_samples_%d" % n] = (R, n, D, base)
    for r in (-1, 0, 1):
        v["n_rays_%d" % r] = (r, N, D, base)
    return v


GRID_OK = dict(lo=(-1., -1., -1.), inv=(8., 8., 8.), dims=(16, 16, 16))


def grid_variants():
    """name -> the keywords of a grid: every defect in every component, the three overflow limits and the largest grids below them"""
    v = {}
    for c in range(3):
        def put(key, value, c=c):
            t = list(GRID_OK[key])
            t[c] = value
            return {key: tuple(t)}
        for d in (0, -1):
            v["dim%d_%d" % (c, d)] = put("dims", d)
        for name, x in (("nan", NAN), ("inf", INF), ("minus_inf", -INF)):
            v["lo%d_%s" % (c, name)] = put("lo", x)
        for name, x in (("zero", 0.), ("negative", -2.), ("nan", NAN), ("inf", INF)):
            v["inv%d_%s" % (c, name)] = put("inv", x)
    v["rows_over_int32"] = dict(dims=(32, 2 ** 16, 2 ** 16))
    v["rows_2_31"] = dict(dims=(1, 2 ** 16, 2 ** 15))
    v["rows_int32_max"] = dict(dims=(1, 2 ** 31 - 1, 1))
    v["words_over_int32"] = dict(dims=(2 ** 26, 2 ** 10, 1))      # rows wx = 2^31
    v["cells_over_int32"] = dict(dims=(2 ** 16, 2 ** 16, 2))      # rows wx = 2^28, rows n_x = 2^33
    v["cells_int32_max"] = dict(dims=(2 ** 31 - 1, 1, 1))
    v["cells_2_31"] = dict(dims=(2 ** 30, 2, 1))
    return v


def table():
    """(entry point, case name, cfg tuple or None, keywords of call()) for every case of the launching entry points"""
    for entry, (names, base, _, align) in LAUNCHING.items():
        cfgs = cfg_variants(base)
        good = cfgs["good"]
        has_grid = "grid_lo" in names
        optional = [k for k in names if k == "jitter" or k.startswith("opt_")]
        required = [k for k in names if k not in optional]
        for name, c in cfgs.items():
            yield entry, "cfg:" + name, c, {}
        yield entry, "null:every_optional", good, dict(null=tuple(optional))
        for k in names:
            yield entry, "null:" + k, good, dict(null=(k,))
            if k in GRID:
                continue      # (host arrays: no alignment of their own)
            for off in (4, 1):
                yield entry, "off%d:%s" % (off, k), good, dict(off={k: off})
                if k in align and off % align[k]:      # a pointer the entry point holds to an alignment: the defect alone, no probe
                    yield entry, "off%d_alone:%s" % (off, k), good, dict(off={k: off}, probe=False)
        # two defects: which one answers
        for k in required:
            yield entry, "null:%s+off4:packed" % k, good, dict(null=(k,), off={"packed": 4})
            yield entry, "cfg:hidden_64+null:%s" % k, cfgs["hidden_64"], dict(null=(k,))
        yield entry, "cfg:n_rays_0+off4:packed", cfgs["n_rays_0"], dict(off={"packed": 4})
        yield entry, "cfg:n_samples_1025+off4:packed", cfgs["n_samples_1025"], dict(off={"packed": 4})
        yield entry, "cfg:s_pad_over_int32_n256+null:packed", cfgs["s_pad_over_int32_n256"], dict(null=("packed",))
        yield entry, "cfg:s_pad_over_int32_n256+off4:packed", cfgs["s_pad_over_int32_n256"], dict(off={"packed": 4})
        if not has_grid:
            continue
        grids = grid_variants()
        for name, g in grids.items():
            yield entry, "grid:" + name, good, g
        bad, big = grids["dim1_0"], grids["cells_over_int32"]
        for name in ("hidden_64", "n_samples_1025", "bf16", "no_split2", "train_flipped", "s_pad_over_int32_n256", "n_rays_0", "null"):
            yield entry, "cfg:%s+grid:dim1_0" % name, cfgs[name], bad
            yield entry, "cfg:%s+grid:cells_over_int32" % name, cfgs[name], big
        yield entry, "grid:lo0_nan+cells_over_int32", good, dict(lo=(NAN, -1., -1.), dims=big["dims"])
        yield entry, "grid:inv2_zero+rows_over_int32", good, dict(inv=(8., 8., 0.), dims=(32, 2 ** 16, 2 ** 16))
        yield entry, "grid:dim2_0+rows_over_int32", good, dict(dims=(2 ** 16, 2 ** 16, 0))
        for k in required:
            yield entry, "grid:dim1_0+null:" + k, good, dict(null=(k,), **bad)
            yield entry, "grid:cells_over_int32+null:" + k, good, dict(null=(k,), **big)
        for k in align:
            yield entry, "grid:dim1_0+off1:" + k, good, dict(off={k: 1}, **bad)
            yield entry, "grid:cells_over_int32+off1:" + k, good, dict(off={k: 1}, **big)


PLANES = (0, 1, 2, 3, 4, 10, 19, 25, 11, 20, 31, 40, -1, -2, 5, 99, 100, 101, 102, 103, 104, 105, 1000)
SHAPES = ((4, 64), (5, 130), (3, 33), (1, 1), (1024, 192))


def _cfg(L, c):
    return None if c is None else C.byref(L.Cfg(*c))


def call(L, lib, entry, c, null=(), off=None, probe=True, lo=GRID_OK["lo"], inv=GRID_OK["inv"], dims=GRID_OK["dims"]):
    """One launching entry point on fake pointers -> its return code"""
    names, _, probes, _ = LAUNCHING[entry]
    off = dict(off or {})
    free = [k for k in probes if k not in off and k not in null]
    if probe and free:      # (a case that sets both probes holds a null required pointer: refused as it is)
        off[free[0]] = 2
    host = dict(grid_lo=(C.c_float * 3)(*lo), grid_inv_step=(C.c_float * 3)(*inv), grid_dims=(C.c_int32 * 3)(*dims))
    v = [None if k in null else host[k] if k in host else C.c_void_p(0x10000 * (i + 1) + off.get(k, 0)) for i, k in enumerate(names)]
    return getattr(lib, entry)(_cfg(L, c), *v, None)


def record(L, lib):
    """The whole table from the loaded library"""
    out = {}
    for entry, case, c, kw in table():
        rc = call(L, lib, entry, c, **kw)
        if rc not in (-1, -2, -3):
            raise RuntimeError("%s %s: code %d -- a case of this table must be refused on the host" % (entry, case, rc))
        assert case not in out.setdefault(entry, {}), (entry, case)
        out[entry][case] = rc
    for fam in ("nnr_frozen", "nnr_frozen_sparse"):
        floats, planes = out.setdefault(fam + "_workspace_floats", {}), out.setdefault(fam + "_ws_plane", {})
        variants = dict(cfg_variants(NEED))
        for R, N in SHAPES:
            for D in (128, 256):
                variants["shape_%d_%d_%d" % (R, N, D)] = (R, N, D, NEED | (DIST_ALPHA if R == 3 else 0))
        for name, c in variants.items():
            floats[name] = getattr(lib, fam + "_workspace_floats")(_cfg(L, c))
            for p in PLANES:
                pitch = C.c_int32(-7)      # (-7 stays where the entry point writes no pitch)
                planes["%s:plane_%d" % (name, p)] = [getattr(lib, fam + "_ws_plane")(_cfg(L, c), p, C.byref(pitch)), pitch.value]
            planes["%s:plane_0:no_pitch" % name] = [getattr(lib, fam + "_ws_plane")(_cfg(L, c), 0, None), None]
    return out


def main():
    sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
    from nnr import lib as L
    rec = record(L, L.load())
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d values of %d entry points -> %s" % (sum(len(v) for v in rec.values()), len(rec), OUT))


if __name__ == "__main__":
    main()
