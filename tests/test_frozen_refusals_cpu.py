"""CPU: the refusal table of the frozen-field family and the sparse inference render (tests/golden/frozen_refusals.json, recorded by
oracle/frozen_refusals.py before their host code was merged into one unit) replayed against the built library: every return code that is
decided on the host, the workspaces' sizes and every plane's offset and pitch are what they were.  Fake device pointers; no case gets as far
as a launch (the table's own statement: every call carries a misaligned required pointer)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))

import frozen_refusals as FR      # noqa: E402

ENTRIES = sorted(FR.LAUNCHING) + [fam + tail for fam in ("nnr_frozen", "nnr_frozen_sparse") for tail in ("_workspace_floats", "_ws_plane")]


@pytest.fixture(scope="module")
def replayed():
    from nnr import lib as L
    return FR.record(L, L.load())


@pytest.fixture(scope="module")
def golden():
    with open(FR.OUT) as f:
        return json.load(f)


def test_the_table_covers_the_nine_entry_points_and_every_kind_of_case(golden):
    assert sorted(golden) == sorted(ENTRIES) and len(ENTRIES) == 9
    for entry in FR.LAUNCHING:
        codes = set(golden[entry].values())
        assert codes == {-1, -2, -3}, entry      # refused, every one, and each of the three codes occurs
        assert golden[entry]["cfg:good"] == -3      # the probe alone: a call in order gets as far as the alignment stage
        kinds = {c.split(":")[0] for c in golden[entry]}
        assert {"cfg", "null", "off4", "off1", "off1_alone"} <= kinds, entry
        assert any("+" in c for c in golden[entry]), entry      # two defects at once: the order of the refusals
    for entry in ("nnr_frozen_sparse_fwd", "nnr_render_sparse"):
        assert sum(c.startswith("grid:") and "+" not in c for c in golden[entry]) == 3 * 9 + 7      # nine defects per component, seven sizes
        assert sum("grid:" in c and "+" in c for c in golden[entry]) >= 20      # a grid defect beside another one
    # the two units order a bad grid and an unsupported cfg differently, and the table says so
    assert golden["nnr_frozen_sparse_fwd"]["cfg:hidden_64+grid:dim1_0"] == -2 and golden["nnr_render_sparse"]["cfg:hidden_64+grid:dim1_0"] == -1
    # the int32 bound on the padded sample count is the sparse family's alone
    assert golden["nnr_frozen_fwd"]["cfg:s_pad_over_int32_n256"] == -3 and golden["nnr_frozen_sparse_fwd"]["cfg:s_pad_over_int32_n256"] == -2
    assert golden["nnr_frozen_workspace_floats"]["s_pad_over_int32_n256"] > 0 and golden["nnr_frozen_sparse_workspace_floats"]["s_pad_over_int32_n256"] == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_library_answers_what_the_table_says(entry, replayed, golden):
    got, want = replayed[entry], golden[entry]
    assert sorted(got) == sorted(want)      # the cases of oracle/frozen_refusals.py are the recorded ones
    wrong = {c: (got[c], want[c]) for c in want if got[c] != want[c]}
    assert not wrong, (entry, len(wrong), dict(list(wrong.items())[:8]))
