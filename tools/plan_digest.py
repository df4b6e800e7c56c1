"""Digests of the weight-gradient plans and of the sizes that depend on them, one line per cfg -- to compare two builds of libnnr.so.

    python tools/plan_digest.py [--lib PATH]               the grid below under this process's environment
    python tools/plan_digest.py [--lib PATH] --all-knobs   the grid once per knob setting (KNOBS), each in a process of its own
                                                           (the library reads the NNR_WGRAD_* variables once per process)

Only the public C ABI (include/nnr.h) through ctypes, no GPU and no torch: it runs unchanged on any ABI-8 library.  A training cfg prints
nnr_plan_counts, nnr_plan_bytes, nnr_workspace_floats, nnr_packed_floats and the SHA-256 of the nnr_plan_build blob; an inference cfg the
sizes alone.  tests/golden/plan_digests.txt is the --all-knobs output of the library before the planners moved into nnr_wgrad_plan.cpp;
tests/test_plan_digest_cpu.py holds the current library to it line for line."""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "nope-nerf_amd", "nnr", "libnnr.so")
TRAIN, BF16, SPLIT3, SPLIT2 = 8, 16, 32, 64                       # NNR_F_* of include/nnr.h
WIDTHS = (128, 256)
MODES = (("mfma", 0), ("split3", SPLIT3), ("split2", SPLIT3 | SPLIT2), ("bf16", BF16))
SHAPES = ((1, 1), (4, 32), (5, 33), (5, 130), (2, 128), (3, 128), (32, 64), (256, 64), (4, 1024), (1024, 192), (4096, 128))
INFERENCE_SHAPES = ((1024, 192), (4096, 128))                     # without NNR_F_TRAIN: the sizes alone
KNOBS = ("", "NNR_WGRAD_BUNDLES=1", "NNR_WGRAD_MAX_BLOCKS=2", "NNR_WGRAD_NO_COOP=1", "NNR_WGRAD_FP32=1", "NNR_WGRAD_BF16_TERMS=1",
         "NNR_WGRAD_ENC2_WEIGHT=0", "NNR_WGRAD_NO_MERGE=1")


class Cfg(C.Structure):
    _fields_ = [("n_rays", C.c_int32), ("n_samples", C.c_int32), ("hidden", C.c_int32), ("flags", C.c_uint32)]


def digest_lines(lib_path):
    lib = C.CDLL(lib_path)
    for f in (lib.nnr_plan_bytes, lib.nnr_workspace_floats, lib.nnr_packed_floats):
        f.restype, f.argtypes = C.c_size_t, [C.c_void_p]
    lib.nnr_plan_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nnr_plan_build.argtypes = [C.c_void_p, C.c_void_p]
    lines = []
    for D in WIDTHS:
        for name, mode in MODES:
            for train, shapes in ((TRAIN, SHAPES), (0, INFERENCE_SHAPES)):
                for R, N in shapes:
                    cfg = Cfg(R, N, D, mode | train)
                    ref = C.byref(cfg)
                    nj, nw = C.c_int32(-1), C.c_int32(-1)
                    rc = lib.nnr_plan_counts(ref, C.byref(nj), C.byref(nw))
                    nbytes = lib.nnr_plan_bytes(ref)
                    line = "D=%d mode=%s train=%d R=%d N=%d counts_rc=%d jobs=%d waves=%d plan_bytes=%d workspace_floats=%d packed_floats=%d" % (
                        D, name, 1 if train else 0, R, N, rc, nj.value, nw.value, nbytes, lib.nnr_workspace_floats(ref), lib.nnr_packed_floats(ref))
                    if train:
                        blob = C.create_string_buffer(b"\xa5" * (nbytes + 64), nbytes + 64)      # a guard behind the blob: the writer stays inside plan_bytes
                        rc = lib.nnr_plan_build(ref, blob)
                        raw = blob.raw
                        assert raw[nbytes:] == b"\xa5" * 64, "nnr_plan_build wrote past nnr_plan_bytes: " + line
                        line += " build_rc=%d sha256=%s" % (rc, hashlib.sha256(raw[:nbytes]).hexdigest())
                    lines.append(line)
    return lines


def all_knobs(lib_path):
    """The digest lines of every knob setting, each under a '# <setting>' header; one child process per setting."""
    out = []
    for knob in KNOBS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("NNR_WGRAD_")}
        if knob:
            env[knob.split("=")[0]] = knob.split("=")[1]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib_path], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("plan_digest under %r failed:\n%s" % (knob, r.stderr[-2000:]))
        out.append("# " + (knob or "no knob set"))
        out.extend(r.stdout.splitlines())
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--all-knobs", action="store_true")
    args = ap.parse_args()
    print("\n".join(all_knobs(args.lib) if args.all_knobs else digest_lines(args.lib)))
