"""No GPU: the scratch registry covers every operator that takes device scratch, and the harness's guard logic reports what it should."""
import ast
import os

import pytest
import torch

import scratch_cases as SC
import scratch_harness as H

OPS_PY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kinectpy_amd", "ops.py")
ALLOWED_EXCLUSIONS = {"frame_step_sharded"}          # plus what the fault rule took out, named here with its reason when that happens


def _scratch_users():
    """module-level functions of ops.py whose body calls L.workspace("""
    tree = ast.parse(open(OPS_PY).read())
    out = []
    for f in tree.body:
        if isinstance(f, ast.FunctionDef) and any(
                isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "workspace"
                and isinstance(n.func.value, ast.Name) and n.func.value.id == "L" for n in ast.walk(f)):
            out.append(f.name)
    return out


def test_every_operator_that_takes_scratch_has_a_case_or_a_reason():
    users = _scratch_users()
    assert len(users) >= 71 and "median_i16" in users and "pointnet_train_step" in users
    missing = [u for u in users if u not in SC.CASES and u not in SC.EXCLUDED]
    assert not missing, f"operators that call L.workspace( without an entry in tests/scratch_cases.py: {missing}"
    both = [u for u in users if u in SC.CASES and u in SC.EXCLUDED]
    assert not both, both
    stale = [n for n in list(SC.CASES) + list(SC.EXCLUDED) if n not in users]
    assert not stale, f"entries for functions that take no scratch (any more): {stale}"
    assert set(SC.EXCLUDED) <= ALLOWED_EXCLUSIONS, set(SC.EXCLUDED) - ALLOWED_EXCLUSIONS
    assert all(isinstance(r, str) and len(r) > 10 for r in SC.EXCLUDED.values())


def test_every_case_is_complete():
    for name, c in SC.CASES.items():
        assert callable(c.make) and callable(c.run) and callable(c.check), name
        assert len(c.sizes) >= 2 and c.sizes[0] == "large" and "small" in c.sizes, (name, c.sizes)


def _arena(nbytes, pattern):
    buf = torch.empty(nbytes + 2 * H.GUARD + H.ALIGN + 7, dtype=torch.uint8)[7:]          # a base that needs aligning
    a = H.Arena(buf)
    assert a.base % H.ALIGN == 0 and a.lo >= H.GUARD and a.capacity >= nbytes
    a.paint(nbytes, pattern)
    return a


@pytest.mark.parametrize("pattern", [0x00, 0xFF, 0x7F])
def test_guard_logic_on_host_tensors(pattern):
    nbytes = 1000
    a = _arena(nbytes, pattern)
    assert pattern != H.CANARY and a.damage(nbytes) == []
    assert bool((a.buf[a.lo:a.lo + nbytes] == pattern).all())
    a.buf[a.lo:a.lo + nbytes] = 0x33                       # writes inside nbytes, first and last byte included: not reported
    assert a.damage(nbytes) == []
    a.buf[a.lo + nbytes] = 0x33                            # one byte past nbytes
    assert a.damage(nbytes) == [(nbytes, 0x33)]
    a.paint(nbytes, pattern)
    a.buf[a.lo - 1] = 0x00                                 # one byte before the base
    assert a.damage(nbytes) == [(-1, 0x00)]
    a.paint(nbytes, pattern)
    a.buf[a.lo + nbytes + H.GUARD - 1] = 0x01              # the guard's last byte
    assert a.damage(nbytes) == [(nbytes + H.GUARD - 1, 0x01)]


def test_leftover_paints_the_guards_only_and_a_smaller_hand_out_moves_the_back_guard():
    a = _arena(4096, 0x7F)
    a.paint(100, "leftover")
    assert a.damage(100) == [] and bool((a.buf[a.lo:a.lo + 100] == 0x7F).all())
    assert bool((a.buf[a.lo + 100:a.lo + 100 + H.GUARD] == H.CANARY).all())
    a.paint(0, 0xFF)                                       # a hand-out of no bytes: the two guards meet at the base
    assert a.damage(0) == []
    a.buf[a.lo] = 0x00
    assert a.damage(0) == [(0, 0x00)]
