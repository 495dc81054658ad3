"""The KPX_* environment names the sources read, held against the switch matrix and INTEGRATION.md; and the precondition of the GPU
module's SOR comparison, from the CPU oracle alone."""
import glob
import os
import re

from tests import switch_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_names():
    """quoted "KPX_..." names in the library's sources: every one of them reaches getenv (directly or through icp_switches' readers)
    or os.environ"""
    names = {}
    files = glob.glob(os.path.join(ROOT, "kinectpy_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "kinectpy_amd", "*.py"))
    for path in sorted(f for f in files if os.path.isfile(f)):
        text = open(path, errors="replace").read()
        if "getenv" not in text and "os.environ" not in text:
            continue
        for name in re.findall(r'"(KPX_[A-Z0-9_]+)"', text):
            names.setdefault(name, os.path.relpath(path, ROOT))
    return names


def test_every_switch_the_sources_read_is_tested_or_exempt():
    names = _read_names()
    assert len(names) >= 42                                            # (the library reads 42: a scan that finds fewer has lost its pattern)
    covered = M.matrix_names() | set(M.FLIPPED_ELSEWHERE) | set(M.EXEMPT)
    assert not sorted(set(names) - covered), "read by the library, flipped by no test and not exempt"
    assert not sorted(set(M.EXEMPT) & (M.matrix_names() | set(M.FLIPPED_ELSEWHERE)))
    assert all(reason.strip() for reason in M.EXEMPT.values())
    # a name listed as flipped by an existing test does occur in that test's module
    for name, where in M.FLIPPED_ELSEWHERE.items():
        module = where.split("::")[0].replace(".", os.sep) + ".py"
        text = open(os.path.join(ROOT, module)).read()
        assert name in text and (("::" not in where) or ("def " + where.split("::")[1] + "(") in text), (name, where)


def test_every_name_in_the_matrix_occurs_in_the_sources():
    """a misspelt setting would pass vacuously: its child is the default child"""
    names = _read_names()
    listed = M.matrix_names() | set(M.FLIPPED_ELSEWHERE) | set(M.EXEMPT)
    assert not sorted(listed - set(names))


def test_every_switch_is_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert not sorted(name for name in _read_names() if "`" + name not in doc)


def test_matrix_holds_every_setting_once():
    want = {"grid": 8, "voxel": 2, "icp": 5, "icp_edges": 5, "dense": 1, "frame": 7, "fps": 2}
    assert {fam: len(s) for fam, s in M.FAMILIES.items()} == want
    for fam in M.FAMILIES.values():
        for setting, env in fam.items():
            assert "+".join("%s=%s" % (k[4:], v) for k, v in env.items()) == setting


def test_sor_inputs_keep_their_distance_from_the_threshold(oracle):
    """No point's mean neighbour distance lies within relative SOR_MARGIN of the keep threshold, for every SOR input and (k, ratio) of
    the GPU module: two correct forms whose sums differ in the last bits then keep the same points."""
    inp = M.grid_inputs()
    for name, k, ratio in M.sor_cases():
        _, stats, avg = oracle.sor(inp[name], k, ratio)
        assert M.sor_margin(avg, stats[2]) > M.SOR_MARGIN, (name, k, ratio)


def test_sor_settings_reach_every_pass0_kernel():
    reached = {M.sor_pass0(k, env) for env in list(M.FAMILIES["grid"].values()) + [{}] for k in M.SOR_KS}
    assert reached == {None, "block<4>", "block<8>", "block<16>", "block<32>"}
