"""CPU: the build script (nope-nerf_amd/csrc/build.py) -- the scratch limits it holds the kernels to, what SOURCES lists, and which objects a
touched file makes stale: build.deps() reads that from the `#include "..."` lines, and is checked here against one table written out by hand
and against what hipcc itself reports (-MM) for every entry of SOURCES."""
import functools
import importlib.util
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nope-nerf_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _build():
    spec = importlib.util.spec_from_file_location("nnr_build", os.path.join(CSRC, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _lines(name):
    with open(os.path.join(CSRC, name)) as f:
        return [l.strip() for l in f]


# ------------------------------------------------------------------------------------------------------------ scratch limits
REMARK = "remark: Function Name: %s\nremark:     ScratchSize [bytes/lane]: %d\n"
# (key of SCRATCH_LIMIT, a mangled name it decides, what the limit must be -- None: at most the inference forward's --, a scratch size above it)
KERNELS = [("15grid_f16_kernelI", "_ZN3nnr15grid_f16_kernelILi256EEEvNS_8GridArgsE", 0, 16),
           ("17bricks_f16_kernelI", "_ZN3nnr17bricks_f16_kernelILi256EEEvNS_10BricksArgsE", 0, 16),
           ("16depth_f16_kernelI", "_ZN3nnr16depth_f16_kernelILi256EEEvNS_9DepthArgsE", 0, 16),
           ("16depth_f16_kernelI", "_ZN3nnr16depth_f16_kernelILi128EEEvNS_9DepthArgsE", 0, 16),
           ("21tsdf_integrate_kernelE", "_ZN3nnr21tsdf_integrate_kernelENS_8TsdfArgsE", 0, 16),
           ("25ray_distortion_fwd_kernelE", "_ZN3nnr25ray_distortion_fwd_kernelENS_17RayDistortionArgsE", 0, 8),
           ("25ray_distortion_bwd_kernelE", "_ZN3nnr25ray_distortion_bwd_kernelENS_17RayDistortionArgsE", 0, 8),
           ("17sparse_f16_kernelI", "_ZN3nnr17sparse_f16_kernelILi256EEEvNS_10SparseArgsE", None, 64)]


@pytest.mark.parametrize("key,mangled,limit,above", KERNELS,
                         ids=["grid", "bricks", "depth_256", "depth_128", "tsdf", "ray_distortion_fwd", "ray_distortion_bwd", "sparse"])
def test_the_build_holds_the_kernel_to_its_scratch_limit(key, mangled, limit, above):
    b = _build()
    if limit is None:      # the sparse kernel runs the inference forward's passes and composite carry: its allowance, and no more
        assert b.SCRATCH_LIMIT[key] <= b.SCRATCH_LIMIT["18mlp_fwd_f16_kernelILi256ELb0E"] == 48
    else:
        assert b.SCRATCH_LIMIT[key] == limit
    at = b.SCRATCH_LIMIT[key]
    assert above > at
    b.check_resources(REMARK % (mangled, at), "test")
    for size in (at + 1, above):
        with pytest.raises(RuntimeError, match="scratch"):
            b.check_resources(REMARK % (mangled, size), "test")
    with pytest.raises(RuntimeError, match="scratch"):      # the remark without hipcc's "remark:" prefix is read as well
        b.check_resources("Function Name: %s\nScratchSize [bytes/lane]: %d\n" % (mangled, above), "test")


# ------------------------------------------------------------------------------------------------------------ SOURCES
def test_sources_lists_every_unit_once():
    b = _build()
    for src in ("nnr_march_f16.hip", "nnr_propose_f16.hip", "nnr_grid_f16.hip", "nnr_bricks_f16.hip", "nnr_depth_f16.hip", "nnr_tsdf.hip",
                "nnr_fusion_api.cpp", "nnr_sparse_f16.hip", "nnr_sparse_api.cpp", "nnr_ray_distortion.hip", "nnr_regularise_api.cpp",
                "nnr_wgrad_plan.cpp", "nnr_frozen_api.cpp", "nnr_frozen_sparse.hip"):
        assert (src, ()) in b.SOURCES and os.path.exists(os.path.join(CSRC, src)), src
    assert len(set(b.SOURCES)) == len(b.SOURCES)
    assert len({b._obj_name(s, d) for s, d in b.SOURCES}) == len(b.SOURCES)
    # the main host unit holds no device code and no other unit's text: every .cpp and .hip is an entry of SOURCES, compiled on its own
    assert not [l for l in _lines("nnr_api.cpp") if re.match(r'#\s*include\s*["<][^">]*\.(cpp|hip)[">]', l)]


# ------------------------------------------------------------------------------------------------------------ who depends on what
DENSITY = {"nnr_march_f16.hip", "nnr_propose_f16.hip", "nnr_grid_f16.hip", "nnr_bricks_f16.hip", "nnr_depth_f16.hip"}
SHARED = ("nnr_density_setup_f16.inc", "nnr_density_pass_f16.inc")
TRUNK = DENSITY | {"nnr_mlp_fwd_f16.hip", "nnr_sparse_f16.hip"}                     # the units that run the two-term trunk
F16 = TRUNK | {"nnr_mlp_dgrad_f16.hip"}
SPLIT = F16 | {"nnr_mlp_fwd.hip", "nnr_mlp_dgrad.hip", "nnr_wgrad.hip"}
# the host units of the newer families include their own family's headers and nnr.h; nnr_tsdf.hip its family's nnr_fusion_kernels.h alone
NO_LAYOUT = {"nnr_fusion_api.cpp", "nnr_sparse_api.cpp", "nnr_regularise_api.cpp", "nnr_tsdf.hip"}
# header -> the source files whose objects it makes stale; written out by hand, never taken from deps()
USERS = {"nnr_density_setup_f16.inc": DENSITY,
         "nnr_density_pass_f16.inc": DENSITY,
         "nnr_trunk_f16.inc": TRUNK,
         "nnr_trunk_f16.h": TRUNK,
         "nnr_colour_f16.inc": {"nnr_mlp_fwd_f16.hip", "nnr_sparse_f16.hip"},
         "nnr_split2.h": F16,
         "nnr_resample_row.h": {"nnr_resample.hip", "nnr_propose_f16.hip"},
         "nnr_wgrad_plan.h": {"nnr_api.cpp", "nnr_wgrad_plan.cpp"},
         "nnr_fusion_kernels.h": {"nnr_depth_f16.hip", "nnr_tsdf.hip", "nnr_fusion_api.cpp"},
         "nnr_sparse_kernels.h": {"nnr_sparse_f16.hip", "nnr_sparse_api.cpp"},
         "nnr_regularise_kernels.h": {"nnr_ray_distortion.hip", "nnr_regularise_api.cpp"},
         "include/nnr_regularise.h": {"nnr_ray_distortion.hip", "nnr_regularise_api.cpp"},
         "include/nnr_geometry.h": {"nnr_api.cpp"},
         "include/nnr_fusion.h": {"nnr_fusion_api.cpp"},
         "include/nnr_sparse.h": {"nnr_sparse_api.cpp"},
         "nnr_grid_check.h": {"nnr_sparse_api.cpp", "nnr_frozen_api.cpp"},
         "nnr_sparse_cell.h": {"nnr_sparse_f16.hip", "nnr_frozen_sparse.hip"},
         "nnr_frozen_kernels.h": {"nnr_mlp_fwd_f16.hip", "nnr_mlp_dgrad_f16.hip", "nnr_frozen_sparse.hip", "nnr_frozen_api.cpp", "nnr_api.cpp"},
         "nnr_frozen_sparse_kernels.h": {"nnr_mlp_fwd_f16.hip", "nnr_mlp_dgrad_f16.hip", "nnr_frozen_sparse.hip", "nnr_frozen_api.cpp"},
         "include/nnr_frozen.h": {"nnr_frozen_api.cpp"},
         "include/nnr_frozen_sparse.h": {"nnr_frozen_api.cpp"},
         "nnr_mlp_fwd_common.h": TRUNK | {"nnr_mlp_fwd.hip"},
         "nnr_split.h": SPLIT,
         "nnr_mlp_bf16.h": SPLIT | {"nnr_mlp_fwd_bf16.hip", "nnr_mlp_dgrad_bf16.hip"}}


def _header(name):
    return os.path.join(ROOT, name) if name.startswith("include/") else os.path.join(CSRC, name)


def test_a_header_makes_exactly_the_units_that_include_it_stale():
    b = _build()
    sources = {s for s, _ in b.SOURCES}
    assert len(sources) == 31 and len(SPLIT) == 11 and len(USERS["nnr_mlp_bf16.h"]) == 13
    for header, want in list(USERS.items()) + [("nnr_layout.h", sources - NO_LAYOUT)]:
        assert want <= sources, header
        path = _header(header)
        got = {src for src in sources if any(os.path.samefile(d, path) for d in b.deps(src))}
        assert got == want, header
    for src in sources:
        assert all(os.path.isabs(d) and d == os.path.normpath(d) and os.path.isfile(d) for d in b.deps(src)), src
        assert len(set(b.deps(src))) == len(b.deps(src)) and os.path.join(CSRC, src) not in b.deps(src), src


def test_the_density_units_include_the_shared_pass_once_and_the_trunk_through_it():
    for src in sorted(DENSITY):
        lines = _lines(src)
        for h in SHARED:
            assert lines.count('#include "%s"' % h) == 1, (src, h)
        assert '#include "nnr_trunk_f16.inc"' not in lines, src      # the trunk's text comes through the pass alone
    assert _lines("nnr_density_pass_f16.inc").count('#include "nnr_trunk_f16.inc"') == 1
    for src in ("nnr_mlp_fwd_f16.hip", "nnr_sparse_f16.hip"):      # the two full kernels: the trunk's and the colour branch's text once each
        lines = _lines(src)
        assert lines.count('#include "nnr_trunk_f16.inc"') == 1 and lines.count('#include "nnr_colour_f16.inc"') == 1, src
    # the point is formed without contraction in the bricks kernel, as the grid kernel forms it, and in the TSDF integrator
    assert "#pragma clang fp contract(off)" in _lines("nnr_bricks_f16.hip")
    assert "#pragma clang fp contract(off)" in _lines("nnr_tsdf.hip")


def test_the_fusion_units_keep_to_their_own_headers_and_use_no_atomics():
    for src in ("nnr_depth_f16.hip", "nnr_tsdf.hip", "nnr_fusion_api.cpp"):
        with open(os.path.join(CSRC, src)) as f:
            text = f.read()
        assert '#include "nnr_resample_row.h"' not in text and '#include "nnr_wgrad_plan.h"' not in text, src
        assert "atomic" not in re.sub(r"//.*", "", text), src


# ------------------------------------------------------------------------------------------------------------ the scanner against the compiler
def test_deps_is_what_hipcc_reports():
    """For every entry of SOURCES: the files of this repository that hipcc reads beside the source (-MM with the build's flags and the entry's
    defines, host pass) are deps(src), as sets.  deps() ignores conditional compilation; no quoted include stands under a condition today, so
    the two are equal and not merely deps() the larger."""
    b = _build()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    flags = [f for f in b.FLAGS if not f.startswith("-Rpass-analysis")]
    root = os.path.realpath(ROOT) + os.sep

    def reported(entry):
        src, defines = entry
        r = subprocess.run([hipcc] + flags + ["-D" + d for d in defines] + ["--cuda-host-only", "-MM", "-MT", "x", os.path.join(CSRC, src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (src, r.stderr[-2000:])
        files = {os.path.realpath(p) for p in r.stdout.replace("\\\n", " ").split()[1:]}
        return {p for p in files if p.startswith(root)} - {os.path.realpath(os.path.join(CSRC, src))}

    with ThreadPoolExecutor(max_workers=b.WORKERS) as ex:
        seen = list(ex.map(reported, b.SOURCES))
    for (src, defines), cc in zip(b.SOURCES, seen):
        assert cc, (src, "hipcc reported no file of the repository")
        assert {os.path.realpath(d) for d in b.deps(src)} == cc, (src, defines)


def test_an_include_that_is_nowhere_raises(tmp_path):
    b = _build()
    root = tmp_path / "pkg" / "csrc"
    (tmp_path / "include").mkdir()
    (root / "sub").mkdir(parents=True)
    (tmp_path / "include" / "api.h").write_text("#include <stdint.h>\n")
    (root / "sub" / "near.h").write_text('#include "here.h"\n#include "top.h"\n')      # here.h: beside the includer first; top.h: in csrc/
    (root / "sub" / "here.h").write_text("")
    (root / "here.h").write_text("")
    (root / "top.h").write_text('// #include "commented_out.h"\n  #  include "api.h"\n')
    (root / "good.hip").write_text('#include <missing_but_in_angle_brackets.h>\n#include "sub/near.h"\n')
    got = b.deps("good.hip", root=str(root))
    assert sorted(got) == sorted(str(p) for p in (root / "sub" / "near.h", root / "sub" / "here.h", root / "top.h", tmp_path / "include" / "api.h"))
    (root / "bad.hip").write_text('#include "top.h"\n\n#include "not_there.h"\n')
    for _ in range(2):      # and again: a failed scan is not remembered as a file without includes
        with pytest.raises(FileNotFoundError, match=r'bad\.hip:3: #include "not_there\.h"'):
            b.deps("bad.hip", root=str(root))
    (root / "deep.hip").write_text('#include "sub/broken.h"\n')
    (root / "sub" / "broken.h").write_text('\n#include "gone.h"\n')
    with pytest.raises(FileNotFoundError, match=r'broken\.h:2: #include "gone\.h"'):
        b.deps("deep.hip", root=str(root))
