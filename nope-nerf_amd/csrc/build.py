"""Build libnnr.so (gfx950) in-tree:  python nope-nerf_amd/csrc/build.py

hipcc cross-compiles without a GPU.  Objects go to csrc/build/, the library to nope-nerf_amd/nnr/libnnr.so
(git-ignored, but shipped to the GPU box by gpurun)."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "build")
LIB = os.path.join(os.path.dirname(HERE), "nnr", "libnnr.so")
# (source, defines): the two fp32 MLP kernels are compiled one template instantiation per translation unit -- each is minutes of hipcc
# time (straight-line code of ~8 000 MFMAs), in one unit the forward alone took 8.5 minutes.  The longest units first: the two D = 256
# three-term forwards take some 25 minutes each where the next longest takes 13, so a full build lasts as long as they do from their start
SOURCES = [("nnr_mlp_fwd.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=1", "NNR_FWD_MODE=2")), ("nnr_mlp_fwd.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=0", "NNR_FWD_MODE=2")),
           ("nnr_wgrad.hip", ()), ("nnr_wgrad.hip", ("NNR_WGRAD_F16_TU=1",)), ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=1")), ("nnr_mlp_dgrad_f16.hip", ("NNR_DGRAD_D=256",)),
           ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=0")),
           # the frozen-field variants (include/nnr_frozen.h): the training forward and the input gradient without their stashes, one unit per D
           ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=2")), ("nnr_mlp_dgrad_f16.hip", ("NNR_DGRAD_D=256", "NNR_DGRAD_STASH=0")),
           ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=2")), ("nnr_mlp_dgrad_f16.hip", ("NNR_DGRAD_D=128", "NNR_DGRAD_STASH=0")),
           # the list-driven frozen variants (include/nnr_frozen_sparse.h): the same two kernels walking a device-built list of live samples
           ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=3")), ("nnr_mlp_dgrad_f16.hip", ("NNR_DGRAD_D=256", "NNR_DGRAD_STASH=0", "NNR_DGRAD_LIST=1")),
           ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=3")), ("nnr_mlp_dgrad_f16.hip", ("NNR_DGRAD_D=128", "NNR_DGRAD_STASH=0", "NNR_DGRAD_LIST=1")),
           ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=1")), ("nnr_mlp_dgrad_f16.hip", ("NNR_DGRAD_D=128",)),
           ("nnr_mlp_fwd_f16.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=0")), ("nnr_sparse_f16.hip", ()), ("nnr_sparse_f16.hip", ("NNR_SPARSE_STOP=1",)), ("nnr_march_f16.hip", ()), ("nnr_propose_f16.hip", ()), ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1",)), ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1", "NNR_PROPOSE_DEPTH=1")),
           # the quantile-depth builds of the two depth kernels (include/nnr_depth_median.h)
           ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1", "NNR_PROPOSE_DEPTH=2")), ("nnr_depth_f16.hip", ("NNR_DEPTH_MEDIAN=1",)),
           ("nnr_grid_f16.hip", ()), ("nnr_bricks_f16.hip", ()),
           ("nnr_mlp_dgrad.hip", ("NNR_DGRAD_D=256", "NNR_DGRAD_MODE=2")),
           ("nnr_mlp_fwd.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=1", "NNR_FWD_MODE=2")), ("nnr_mlp_dgrad.hip", ("NNR_DGRAD_D=128", "NNR_DGRAD_MODE=2")),
           ("nnr_mlp_fwd.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=0", "NNR_FWD_MODE=2")),
           ("nnr_mlp_fwd.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=1")), ("nnr_mlp_fwd.hip", ("NNR_FWD_D=256", "NNR_FWD_TRAIN=0")),
           ("nnr_mlp_dgrad.hip", ("NNR_DGRAD_D=256",)), ("nnr_mlp_fwd.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=1")),
           ("nnr_mlp_fwd.hip", ("NNR_FWD_D=128", "NNR_FWD_TRAIN=0")), ("nnr_mlp_dgrad.hip", ("NNR_DGRAD_D=128",)),
           ("nnr_mlp_fwd_bf16.hip", ()), ("nnr_mlp_dgrad_bf16.hip", ()), ("nnr_mlp_fwd.hip", ()), ("nnr_mlp_dgrad.hip", ()), ("nnr_depth_f16.hip", ()),
           ("nnr_api.cpp", ()), ("nnr_wgrad_plan.cpp", ()), ("nnr_fusion_api.cpp", ()), ("nnr_sparse_api.cpp", ()), ("nnr_frozen_api.cpp", ()), ("nnr_regularise_api.cpp", ()), ("nnr_tsdf.hip", ()),
           ("nnr_frozen_sparse.hip", ()), ("nnr_pack.hip", ()), ("nnr_wgrad_bf16.hip", ()), ("nnr_composite.hip", ()), ("nnr_ray_distortion.hip", ()), ("nnr_resample.hip", ()),
           ("nnr_camera.hip", ()), ("nnr_pointcloud.hip", ()), ("nnr_aux.hip", ()), ("nnr_randperm.hip", ()), ("nnr_optim.hip", ())]


def _obj_name(src, defines):
    tag = "".join("_" + d.split("=")[0].lower().replace("nnr_", "") + d.split("=")[1] for d in defines)
    return os.path.splitext(src)[0] + tag + ".o"


# -pragma-unroll-threshold: the MLP kernels are straight-line code by construction (every `#pragma unroll` loop must unroll fully, or
# the register arrays they index fall back to scratch memory).  LLVM caps `#pragma unroll` at 16 K instructions per loop; one GEMM part
# of the fp32 input-gradient kernel sat right at that cap, and an unrelated clean-up pushed it over: the kernel compiled without a
# warning, kept passing every parity test and ran 8x slower (832 bytes of scratch per lane).  Hence the raised cap AND the check below.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-pragma-unroll-threshold=1048576",
         "-Rpass-analysis=kernel-resource-usage", "-I" + HERE, "-I" + os.path.join(HERE, "..", "..", "include"), "-x", "hip"]
# Scratch bytes per lane a hot kernel may use, by substring of the MANGLED name (the longest matching substring decides).  In the bf16
# training kernels a spill reload is not just a slow load: stores are always in flight there, hipcc waits for any load next to pending
# stores with vmcnt(0), and every reload drains the stash-store queue with the matrix pipe idle -- the TRAINING kernels may only keep a handful of
# prologue values in scratch, reloaded at pass start (where the pass waits for its inputs anyway), nothing inside a pass; the inference forward (no stores in flight) may spill its composite carry.
# (three-term kernels: only the D = 256 training forward keeps a few pass-start values in scratch, 32 bytes)
SCRATCH_LIMIT = {"18mlp_fwd_f16_kernelI": 0, "18mlp_fwd_f16_kernelILi256ELb0E": 48, "18mlp_fwd_f16_kernelILi128ELb0E": 48,      # (inference: prologue values and the composite carry, outside the MFMA streams)
                 "30mlp_fwd_frozen_list_f16_kernelI": 0, "25mlp_dgrad_list_f16_kernelI": 0,      # (the list-driven frozen pair: include/nnr_frozen_sparse.h)
                 "25mlp_fwd_frozen_f16_kernelI": 0,      # (the frozen-field forward; its input gradient is mlp_dgrad_f16_kernel<D, false>: the next key)
                 "20mlp_dgrad_f16_kernelI": 0, "14mlp_fwd_kernelI": 0, "14mlp_fwd_kernelILi256ELb1ELi2E": 48, "16mlp_dgrad_kernelI": 0, "12wgrad_kernelI": 0, "14wgrad_b_kernelE": 0,
                 "19mlp_fwd_bf16_kernelI": 48, "19mlp_fwd_bf16_kernelILi256ELb1E": 16, "19mlp_fwd_bf16_kernelILi128ELb1E": 16,
                 "21mlp_dgrad_bf16_kernelI": 64, "20composite_fwd_kernelE": 0, "20composite_bwd_kernelE": 0,
                 "16march_f16_kernelI": 0, "19march_finish_kernel": 0, "15resample_kernelE": 0, "18propose_f16_kernelI": 0, "15grid_f16_kernelI": 0, "17bricks_f16_kernelI": 0,
                 "16depth_f16_kernelI": 0, "21tsdf_integrate_kernelE": 0,
                 "25ray_distortion_fwd_kernelE": 0, "25ray_distortion_bwd_kernelE": 0,
                 "25frozen_sparse_flag_kernelE": 0, "25frozen_sparse_scan_kernelE": 0, "25frozen_sparse_fill_kernelE": 0,      # (the compaction: nnr_frozen_sparse.hip)
                 "17sparse_f16_kernelI": 48,      # (the inference forward's passes and composite carry: its allowance)
                 "22sparse_stop_f16_kernelI": 48,      # (the same text under NNR_SPARSE_STOP=1: include/nnr_sparse_stop.h)
                 "25propose_sparse_f16_kernelI": 0,      # (the proposal's text under NNR_PROPOSE_SPARSE=1: include/nnr_propose_sparse.h)
                 "23depth_sparse_f16_kernelI": 0,      # (the same text under NNR_PROPOSE_SPARSE=1 NNR_PROPOSE_DEPTH=1: include/nnr_depth_sparse.h)
                 "23depth_median_f16_kernelI": 0,      # (the depth kernel's text under NNR_DEPTH_MEDIAN=1: include/nnr_depth_median.h)
                 "30depth_sparse_median_f16_kernelI": 0}      # (the sparse depth build under NNR_PROPOSE_DEPTH=2: include/nnr_depth_median.h)


def check_resources(remarks, what):
    """Parse hipcc's kernel-resource-usage remarks and fail the build when a hot kernel went to scratch memory."""
    import re
    name, bad = None, []
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            keys = [k for k in SCRATCH_LIMIT if ("3nnr" + k) in name]
            if keys:
                key = max(keys, key=len)
                if int(m.group(1)) > SCRATCH_LIMIT[key]:
                    bad.append("%s: %s bytes of scratch per lane (limit %d)" % (name, m.group(1), SCRATCH_LIMIT[key]))
    if bad:
        raise RuntimeError("%s: a hot kernel uses scratch memory -- a loop did not unroll or registers spilled:\n  " % what + "\n  ".join(bad))


def _usable_cpus():
    """CPUs this process may really use: os.cpu_count() is the whole machine's, while an affinity mask, a cgroup quota or MAX_JOBS may allow
    fewer -- and more compile jobs than CPUs only stretch the two 20-minute units that decide how long a full build takes."""
    n = os.cpu_count() or 4
    if hasattr(os, "sched_getaffinity"):
        n = min(n, len(os.sched_getaffinity(0)))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:      # cgroup v2: "<quota> <period>" in microseconds, or "max <period>"
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    jobs = os.environ.get("MAX_JOBS", "")
    if jobs.isdigit() and int(jobs) > 0:
        n = min(n, int(jobs))
    return n


WORKERS = max(2, min(12, _usable_cpus()))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_variant(name, defines, only=None):
    """Profiling-only library nnr/libnnr_<name>.so with compile-time switches (-DNNR_ABLATE=<bits>, -DNNR_TIMELINE: nnr_device.h); results
    of such a build are NOT valid.  `only`: a substring of the source names to recompile (e.g. "_f16": the fp16-term kernels, minutes instead
    of the whole library); every other object comes from the main build.  Selected at run time with NNR_LIB=<path> (nnr/lib.py)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(os.path.dirname(HERE), "nnr", "libnnr_%s.so" % name)
    tmp = os.path.join(OUT_DIR, "variant_" + name)
    os.makedirs(tmp, exist_ok=True)
    mine = [(src, d) for src, d in SOURCES if only is None or only in src]
    jobs = [[hipcc] + FLAGS + ["-D" + d for d in list(defines) + list(d0)] + ["-c", os.path.join(HERE, src), "-o", os.path.join(tmp, _obj_name(src, d0))]
            for src, d0 in mine]

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)

    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(tmp if (src, d) in mine else OUT_DIR, _obj_name(src, d)) for src, d in SOURCES]
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
    return out


_INCLUDES = {}      # file -> the files its `#include "..."` lines name: every file is read once


def _includes(path, root):
    if path not in _INCLUDES:
        dirs = (os.path.dirname(path), root, os.path.join(root, "..", "..", "include"))
        found = []
        with open(path) as f:
            for n, line in enumerate(f, 1):
                m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
                if m:
                    hits = [t for t in (os.path.normpath(os.path.join(d, m.group(1))) for d in dirs) if os.path.isfile(t)]
                    if not hits:
                        raise FileNotFoundError('%s:%d: #include "%s" is in none of %s' % (path, n, m.group(1), ", ".join(map(os.path.normpath, dirs))))
                    found.append(hits[0])
        _INCLUDES[path] = found
    return _INCLUDES[path]


def deps(src, root=HERE):
    """Every file that csrc/<src> includes in quotes, directly or through another such file (absolute, normalised paths): what beside the
    source makes its objects stale.  A name is looked up as hipcc does with FLAGS: in the including file's directory, then in csrc/ (`root`),
    then in include/.  Includes in angle brackets are the toolchain's and are ignored, and so is conditional compilation: a superset only
    rebuilds more.  A name found nowhere is an error, never skipped -- a dependency this scan misses links a stale object without a word."""
    found, todo = [], [os.path.normpath(os.path.join(root, src))]
    while todo:
        for inc in _includes(todo.pop(), root):
            if inc not in found:
                found.append(inc)
                todo.append(inc)
    return found


LAST_BUILD = {"compiled": [], "reused": [], "linked": False}      # what the newest build() call did (printed by __graft_entry__.build())


def build(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OUT_DIR, exist_ok=True)
    jobs = []
    for src, defines in SOURCES:
        obj = os.path.join(OUT_DIR, _obj_name(src, defines))
        if force or _stale(obj, [os.path.join(HERE, src)] + deps(src)):
            jobs.append([hipcc] + FLAGS + ["-D" + d for d in defines] + ["-c", os.path.join(HERE, src), "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))
        try:
            check_resources(r.stderr, cmd[-3] if len(cmd) > 3 else "link")
        except RuntimeError:
            if os.path.exists(cmd[-1]) and cmd[-1].endswith(".o"):
                os.remove(cmd[-1])       # so that the next build compiles (and checks) this file again
            raise
        if verbose:
            other = "\n".join(l for l in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" not in l and l.strip())
            if other:
                print(other, file=sys.stderr)

    with ThreadPoolExecutor(max_workers=min(WORKERS, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(OUT_DIR, _obj_name(src, defines)) for src, defines in SOURCES]
    relink = bool(force or jobs or _stale(LIB, objs))
    if relink:
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    compiled = [os.path.basename(j[-1]) for j in jobs]
    LAST_BUILD.update(compiled=compiled, reused=[os.path.basename(o) for o in objs if os.path.basename(o) not in compiled], linked=relink)
    return LIB


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--variant":      # build.py --variant noside [--only _f16] NNR_ABLATE=1
        rest = sys.argv[3:]
        only = None
        if rest and rest[0] == "--only":
            only, rest = rest[1], rest[2:]
        print(build_variant(sys.argv[2], rest, only))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
