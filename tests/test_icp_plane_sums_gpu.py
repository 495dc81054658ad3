"""The culled registration accumulates only the update sums its mode reads (acc_live, kpx_icpdefs.h: point-to-point slots 0..16,
point-to-plane slots 0, 1 and 17..43 of the 44): the sums it no longer forms fed nothing, so every registration must come out as
it did before, to the last bit.

Expected values: tests/golden/icp_plane_sums_parent.npz, recorded by tests/golden/make_icp_plane_sums_golden.py with the build of
the commit before that change (its id is in the file).  Inputs and cases: tests/icp_plane_sums_cases.py -- sources of 1, 15, 16, 17,
63, 64, 65 and 129 rows (tile edge, block edge, one past each), one out of reach (count 0, identity update), one with a third of its
rows out of reach; both modes; max_iteration 0, 1 and 30; through ops.icp (the update in its own kernel) and through ops.icp_batch
with three ragged registrations (the grouped driver: the update in the block that draws the last ticket).  The forms of the iteration
are chosen by switches read once per process, so each form runs the cases in one child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_plane_sums_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "icp_plane_sums_parent.npz")

FORMS = {
    "blocks of four": {"KPX_ICP_ROWS": "0"},
    "rows": {"KPX_ICP_ROWS": "2", "KPX_ICP_CHAIN": "0"},
    "prologue": {"KPX_ICP_BATCH_LAUNCH": "0"},
    "kernel": {"KPX_ICP_BATCH_LAUNCH": "0", "KPX_ICP_FUSE": "0"},
}


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    commit = str(g.pop("parent_commit"))
    assert len(commit) == 40 and all(c in "0123456789abcdef" for c in commit), commit
    return g


def compare(got, golden, what):
    assert sorted(got) == sorted(golden), (what, sorted(set(got) ^ set(golden))[:5])
    bad = [key for key in sorted(golden) if not S.same_bits(got[key], golden[key])]
    assert not bad, (what, len(bad), bad[:8], got[bad[0]], golden[bad[0]])


def test_cases_cover_the_edges(golden):
    """what the recorded values are worth: every case is there; the sources converge, the one out of reach pairs nothing and keeps
    its transform, the one with a third of its rows out of reach pairs the other two thirds"""
    n_keys = len(S.MODES) * len(S.ITERATIONS) * (len(S.SIZES) + 2 + len(S.BATCH)) * 2
    assert len(golden) == n_keys, (len(golden), n_keys)
    for mode in S.MODES:
        far = golden["%s.it30.icp.far.s" % mode]
        assert far[3] == 0.0 and far[0] == 0.0 and np.array_equal(golden["%s.it30.icp.far.T" % mode], np.eye(4))
        part = golden["%s.it30.icp.partial.s" % mode]
        assert part[3] == 129 - 43, part
        for name in ("icp.n129", "icp.n65", "batch.n129", "batch.n65", "batch.n17"):
            s = golden["%s.it30.%s.s" % (mode, name)]
            assert s[3] == float(name.rsplit("n", 1)[1]) and s[2] >= 2 and s[1] < 1.0, (mode, name, s)
        assert golden["%s.it0.icp.n64.s" % mode][2] == 0 and golden["%s.it1.icp.n64.s" % mode][2] == 1


def test_default_forms_equal_the_parent(golden):
    """in this process: the forms the library picks by itself"""
    from kinectpy_amd import ops
    compare(S.run(ops), golden, "default")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_form_equals_the_parent(form, golden, tmp_path):
    """one child process per form, all cases inside it"""
    f = str(tmp_path / "got.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "icp_plane_sums_cases.py"), f], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "KPX_ICP_CHAIN_LOCK": "0", **FORMS[form]})    # (this process may hold the device's chain lock; it is idle meanwhile)
    assert r.returncode == 0, r.stderr[-2000:]
    compare(dict(np.load(f)), golden, form)
