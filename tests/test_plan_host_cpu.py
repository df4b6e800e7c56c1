"""The weight-gradient planners as a host unit (csrc/nnr_wgrad_plan.h): (a) the plans and every size that depends on them, digest by digest
against what the library produced before the planners moved out of nnr_api.cpp; (b) a stand-alone program over the unit under the host
sanitizers.  No GPU."""
import importlib.util
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nope-nerf_amd", "csrc")


def _tool():
    spec = importlib.util.spec_from_file_location("plan_digest", os.path.join(ROOT, "tools", "plan_digest.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plan_digests_equal_the_parents():
    """tools/plan_digest.py over the whole grid, once per knob setting in a process of its own, line for line against tests/golden/plan_digests.txt
    (made from the library of the commit named in profiles/api_refactor/README.md): counts, blob bytes, workspace and packed sizes, and the
    SHA-256 of every plan blob."""
    m = _tool()
    with open(os.path.join(ROOT, "tests", "golden", "plan_digests.txt")) as f:
        want = f.read().splitlines()
    got = m.all_knobs(m.DEFAULT_LIB)
    per_setting = len(m.WIDTHS) * len(m.MODES) * (len(m.SHAPES) + len(m.INFERENCE_SHAPES)) + 1
    assert len(want) == len(m.KNOBS) * per_setting and sum(l.startswith("#") for l in want) == len(m.KNOBS)
    assert sum("sha256=" in l for l in want) == len(m.KNOBS) * len(m.WIDTHS) * len(m.MODES) * len(m.SHAPES)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # the knobs do shape the plans: every setting's block differs from the block with no knob set
    blocks = [want[i * per_setting + 1:(i + 1) * per_setting] for i in range(len(m.KNOBS))]
    assert all(b != blocks[0] for b in blocks[1:])


def test_planners_stand_alone_under_host_sanitizers(tmp_path):
    """tests/host/plan_check.cpp + csrc/nnr_wgrad_plan.cpp as a plain executable with AddressSanitizer and UBSan: every plan of the grid with the
    knobs passed explicitly (bundles on and off, 2 and 256 workgroups), its coverage / chaining / balance, serialisation into exactly
    plan_bytes, plan_counts' memo and the workspace regions behind the planes.  The unit includes no HIP header: a plain clang++ builds it."""
    cxx = shutil.which("clang++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    assert os.path.exists(cxx), "no clang++ to build the stand-alone plan check with"
    with open(os.path.join(CSRC, "nnr_wgrad_plan.h")) as f, open(os.path.join(CSRC, "nnr_wgrad_plan.cpp")) as g:
        text = f.read() + g.read()
    own = {'#include "../../include/nnr.h"', '#include "nnr_layout.h"', '#include "nnr_wgrad_plan.h"'}
    assert all((l.startswith("#include <") and "hip" not in l) or l.strip() in own for l in text.splitlines() if l.startswith("#include"))
    assert text.count("getenv(") == 2      # (the two lambdas of PlanKnobs::from_env)
    exe = str(tmp_path / "plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, os.path.join(ROOT, "tests", "host", "plan_check.cpp"), os.path.join(CSRC, "nnr_wgrad_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "352 plans, 88 cfgs, 0 failed" in r.stdout and not r.stderr.strip()
