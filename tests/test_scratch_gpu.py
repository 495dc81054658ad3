"""GPU suite (-m gpu): every operator of kinectpy_amd.ops that takes device scratch, run over poisoned, exact-size scratch and
poisoned outputs (tests/scratch_harness.py) on the cases of tests/scratch_cases.py -- the contract of DESIGN.md 5.4:

  * an operator reads from its scratch only what the same call wrote            (patterns 0xFF / 0x00 / 0x7F, small after large)
  * it writes nothing outside kpx_*_workspace_bytes(args)                       (exact size, guards before and after)
  * it writes every valid output element                                        (outputs filled with the pattern beforehand)

Per operator and size: the result under 0xFF is judged by the operator's CPU reference (check); the results under 0x00 and 0x7F equal
it bit for bit (the reductions are "deterministic run to run"; no operator is exempt so far); then the small case right
after the large one on the same untouched scratch ("leftover") equals its 0xFF result.  A damaged guard fails the run it happened in.
"""
import numpy as np
import pytest
import torch

import scratch_cases as SC
from scratch_harness import scratch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _bits(a):
    a = np.ascontiguousarray(a)
    return (a.shape, a.dtype.str, a.tobytes())


def same_bits(a, b, tag):
    assert len(a) == len(b), tag
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None or y is None:
            assert x is None and y is None, (tag, k)
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert _bits(x) == _bits(y), (tag, "output", k, x.shape, y.shape,
                                      np.argwhere(x.reshape(-1) != y.reshape(-1))[:5].tolist() if x.shape == y.shape else None)


def run_case(case, monkeypatch):
    inputs = {size: case.make(size) for size in case.sizes}
    ref = {}
    for size in case.sizes:
        with scratch(0xFF, exact=True, poison_outputs=True, monkeypatch=monkeypatch) as s:
            ref[size] = case.run(inputs[size])
        assert s.handouts > 0, "the case never asked for scratch"
        case.check(ref[size], inputs[size])
        for pattern in (0x00, 0x7F):
            with scratch(pattern, exact=True, poison_outputs=True, monkeypatch=monkeypatch):
                got = case.run(inputs[size])
            same_bits(got, ref[size], (case.name, size, hex(pattern)))
    # every smaller case right after the larger one, on what it left
    state = None
    for size in case.sizes:
        with scratch("leftover", exact=True, monkeypatch=monkeypatch, state=state) as state:
            got = case.run(inputs[size])
        same_bits(got, ref[size], (case.name, size, "leftover"))
    assert torch.empty is SC.torch.empty and not hasattr(torch.empty, "__wrapped__")


def run_or_stop(case, monkeypatch):
    """a HIP error (a fault among them) ends the session: nothing more is started on a device that has faulted"""
    try:
        run_case(case, monkeypatch)
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"{case.name}: {e}", returncode=99)
        raise


@pytest.mark.parametrize("name", sorted(n for n in SC.CASES if n != "frame_step"))
def test_operator_on_poisoned_exact_scratch(name, monkeypatch):
    run_or_stop(SC.CASES[name], monkeypatch)


def test_the_real_minimum_size_is_reported_without_exact(monkeypatch):
    """exact=False: the harness reports what _lib.Workspace.get would -- never less than 1 MiB -- over the same poisoned region; an
    operator's result does not depend on the slack"""
    from scratch_harness import MIN_REAL
    case = SC.CASES["bounds"]
    inputs = case.make("small")
    with scratch(0xFF, exact=True, poison_outputs=True, monkeypatch=monkeypatch):
        want = case.run(inputs)
    with scratch(0xFF, exact=False, poison_outputs=True, monkeypatch=monkeypatch) as s:
        got = case.run(inputs)
        assert s.workspace(1)[1].value == MIN_REAL and s.workspace(MIN_REAL + 1)[1].value == MIN_REAL + 1
    case.check(got, inputs)
    same_bits(got, want, "exact=False")


def test_frame_step_on_poisoned_exact_scratch(monkeypatch):
    """kpx_frame_step, the native one-call frame, on the smallest sensor ring of the parity suite at the small_xy resolution, against
    the oracle's step as test_native_frame_step_equals_python_pipeline_and_oracle judges it"""
    run_or_stop(SC.CASES["frame_step"], monkeypatch)
