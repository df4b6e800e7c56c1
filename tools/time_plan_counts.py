"""Wall time of 1000 nnr_plan_counts calls on one cfg (D = 256, 1024 x 192, two-term training): what the launch path paid per plan build before
plan_counts kept its memo.  python tools/time_plan_counts.py [--lib PATH]; ctypes only, no GPU."""
import argparse
import ctypes as C
import time

from plan_digest import Cfg, DEFAULT_LIB, SPLIT2, SPLIT3, TRAIN

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--calls", type=int, default=1000)
    args = ap.parse_args()
    lib = C.CDLL(args.lib)
    lib.nnr_plan_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    cfg = Cfg(1024, 192, 256, TRAIN | SPLIT3 | SPLIT2)
    nj, nw = C.c_int32(0), C.c_int32(0)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            lib.nnr_plan_counts(C.byref(cfg), C.byref(nj), C.byref(nw))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    print("%d nnr_plan_counts calls (jobs %d, waves %d): %.3f ms in all, %.2f us per call (best of 3)" % (args.calls, nj.value, nw.value, 1e3 * best, 1e6 * best / args.calls))
