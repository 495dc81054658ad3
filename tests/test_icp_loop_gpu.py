"""GPU suite (-m gpu) for the search -> sums -> solve loop of the registrations (icp_search_solve_loop in kpx_icp.hip) under
generalized ICP, coloured ICP and point-to-plane ICP, and for the screened search beneath it (nn_rowprep_kernel with aux,
nn_screen_kernel, nn_overflow_kernel, the candidate branch of nn_merge_kernel), on the scenes of tests/icp_loop_scenes.py against
the float64 restatements (gicp_ref, robust_ref, the oracle), on every engine.

Two comparisons, both from the existing suites:
  - with the restatement's run: iterations and fitness equal, inlier_rmse to 1e-8, the transform to TOL_T = 1e-8 (a case is admitted
    to it by the spread rule of icp_loop_scenes, asserted on the CPU by tests/test_icp_loop_cpu.py), the correspondences within
    max_dist equal;
  - with oracle.nn at the device's OWN returned transform: index and d2 of the run's last search bit for bit within max_dist, the
    mask beyond it (on the all-pairs engines, in the duplicate scenes, index and d2 of every row: their search has no reach), and
    count and fitness from them.  This pins each search exactly, whatever the order of any sum, and holds for the cases the
    spread rule does not admit as well.
Coloured ICP returns no correspondences: its last search is held to the count and the fitness."""
import numpy as np
import pytest

import icp_loop_scenes as S

pytestmark = pytest.mark.gpu
TOL_T = S.TOL_T          # absolute, 4x4 transform (rotation entries / mm), as test_parity_gpu.py
ENGINES = ("culled", "dense", "dense_fp64")


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


@pytest.fixture(params=ENGINES)
def engine(request, ops):
    prev = ops.nn_engine(request.param)
    yield request.param
    ops.nn_engine(prev)


@pytest.fixture(scope="module")
def cases(oracle, base_cloud):
    return S.all_cases(oracle, base_cloud)


def _npy(t):
    return t.cpu().numpy()


def run(ops, c, iters=None, poll=4):
    """the library on the case -> its result dict (idx, d2 as NumPy arrays where the entry point returns them)"""
    iters = c.iters if iters is None else iters
    loss = None if c.loss[0] == "l2" else c.loss
    if c.kind == "gicp":
        r = ops.generalized_icp(c.src, c.cs, c.tgt, c.ct, c.max_dist, c.init, iters, want_corr=True, poll_interval=poll, loss=loss)
    elif c.kind == "colored":
        r = ops.colored_icp(c.src, c.sc, c.tgt, c.tc, c.tn, c.max_dist, c.init, 0.968, iters, poll_interval=poll, tgt_gradient=c.grad, loss=loss)
    else:
        r = ops.icp(c.src, c.tgt, c.max_dist, c.init, "p2plane", c.tn, iters, want_corr=True, poll_interval=poll, loss=loss)
    if "idx" in r:
        r["idx"], r["d2"] = _npy(r["idx"]), _npy(r["d2"])
    return r


def profiled(ops, fn):
    """fn() between prof_begin / prof_end -> (its result, launches of the screening sweep)"""
    ops.prof_begin()
    try:
        r = fn()
    finally:
        prof = ops.prof_end()
    return r, prof["nn_screen"][1]


def check_search(oracle, c, r, what, every_row=False):
    """the run's last search against oracle.nn at the device's own transform"""
    T = r["transformation"]
    assert np.isfinite(T).all() and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]), what
    idx, d2, _ = oracle.nn(c.src, T, c.tgt, grid=True)
    ok = d2 < c.max_dist ** 2
    assert r["count"] == ok.sum() and r["fitness"] == ok.sum() / len(c.src), what
    if "idx" not in r:
        return
    assert np.array_equal(r["d2"] < c.max_dist ** 2, ok), what
    assert np.array_equal(r["idx"][ok], idx[ok]) and np.array_equal(r["d2"][ok].view(np.uint64), d2[ok].view(np.uint64)), what
    if every_row:
        bad = np.flatnonzero(r["idx"] != idx)
        assert not len(bad), (what, len(bad), bad[:8], r["idx"][bad[:8]], idx[bad[:8]])
        assert np.array_equal(r["d2"].view(np.uint64), d2.view(np.uint64)), what


def check_reference(oracle, c, r, what, iters=None):
    """the run against the restatement's (an admitted case: see icp_loop_scenes)"""
    key = c if iters is None or iters == c.iters else S.with_iters(c, iters)
    rT, rf, rr, rit, (ri, rd) = S.ref(oracle, key)
    diff = S.transform_error(c, r["transformation"], rT)
    print(f"\n{what}: iterations {r['iterations']} / {rit}  fitness {r['fitness']:.6f} / {rf:.6f}  |dT| {diff:.3g}")
    assert r["iterations"] == rit and r["fitness"] == rf and abs(r["inlier_rmse"] - rr) < 1e-8, what
    assert diff < TOL_T, (what, diff)
    if "idx" in r:
        ok = rd < c.max_dist ** 2
        assert np.array_equal(r["d2"] < c.max_dist ** 2, ok) and np.array_equal(r["idx"][ok], ri[ok]), what


def check(oracle, c, r, what, iters=None, every_row=False):
    check_search(oracle, c, r, what, every_row)
    if S.admitted(c):
        check_reference(oracle, c, r, what, iters)


# ---- 1. source-row edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SOURCE_NAMES)
def test_source_row_edges(ops, oracle, cases, engine, name):
    """1 .. 8193 source rows: the merge kernel's 64-row blocks with and without a tail, the solve kernel's 16 slices with one block
    each, with nothing, and with the unrolled loop plus a tail"""
    c = cases[name]
    r = run(ops, c)
    check(oracle, c, r, f"{name} [{engine}]")
    if c.iters == 0:
        rT, rf, rr, rit, (ri, rd) = S.ref(oracle, c)
        assert r["iterations"] == 0 and np.array_equal(r["transformation"], c.init), name
        assert r["fitness"] == rf and r["inlier_rmse"] == rr and r["count"] == (rd < c.max_dist ** 2).sum(), (name, r["inlier_rmse"], rr)


# ---- 2. target-column edges under screening ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.TARGET_NAMES)
def test_target_column_edges_screened(ops, oracle, cases, engine, name):
    """1 .. 2049 target points: a 16-column tile, the culled engine's group of 256, the fp64 stage of 512 columns, the float32 stage
    of 1024 with its padding, its second stage and its split; searches 2 .. 5 are screened on `dense`, never on `dense_fp64`"""
    c = cases[name]
    r, screens = profiled(ops, lambda: run(ops, c))
    print(f"\n{name} [{engine}]: nn_screen launches {screens}")
    assert (screens > 0) if engine == "dense" else (screens == 0), (name, engine, screens)
    check(oracle, c, r, f"{name} [{engine}]")
    if len(c.tgt) == 1:
        assert np.isin(r["idx"], (0, -1)).all() and (r["idx"][r["d2"] < c.max_dist ** 2] == 0).all()


# ---- 3. every search of a run ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", S.EVERY_SEARCH)
def test_every_search_of_a_run(ops, oracle, cases, engine, iters):
    """max_iteration = 0, 1, 2, 3, 4, 6: the correspondences each run returns are those of oracle.nn at the transform it returns --
    searches 0 and 1 by the fp64 sweep, 2 .. 6 screened"""
    c = cases["every-search"]
    r = run(ops, c, iters)
    assert r["iterations"] == iters
    check(oracle, c, r, f"every-search@{iters} [{engine}]", iters)


# ---- 4. unequal sizes, rows without partners ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.RANDOM_NAMES + S.NOTHING_NAMES)
def test_unequal_clouds_and_rows_without_partners(ops, oracle, cases, engine, name):
    c = cases[name]
    r = run(ops, c)
    check(oracle, c, r, f"{name} {len(c.src)} x {len(c.tgt)} max_dist {c.max_dist} [{engine}]")
    if name in S.NOTHING_NAMES:
        assert r["fitness"] == 0.0 and r["count"] == 0 and r["inlier_rmse"] == 0.0 and r["iterations"] == S.ref(oracle, c)[3] == 1
        assert np.array_equal(r["transformation"], c.init), name


# ---- 5. candidate-list overflow ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", S.DUP_TESTED)
@pytest.mark.parametrize("tag", S.DUP_TAGS)
def test_duplicated_target_point_gicp(ops, oracle, cases, engine, tag, iters):
    """60 .. 200 copies of one target point: full and overflowing candidate lists, rows whose answer is their bound's partner and rows
    that come to the copies from elsewhere at a screened search (icp_loop_scenes.duplicate_case)"""
    c = cases[f"{tag}-gicp"]
    r, screens = profiled(ops, lambda: run(ops, c, iters))
    print(f"\n{tag}-gicp@{iters} [{engine}]: nn_screen launches {screens}")
    assert (screens > 0) if engine == "dense" else (screens == 0), (tag, engine, screens)
    check(oracle, c, r, f"{tag}-gicp@{iters} [{engine}]", iters, every_row=engine != "culled")


@pytest.mark.parametrize("poll", (4, 1))
@pytest.mark.parametrize("tag", S.DUP_TAGS)
def test_duplicated_target_point_plain_icp_dense(ops, oracle, cases, tag, poll):
    """the same under plain point-to-plane ICP on `dense`: screened from the third search on at the default poll_interval, by
    ScreenPolicy where every iteration is polled"""
    c = cases[f"{tag}-p2plane"]
    prev = ops.nn_engine("dense")
    try:
        for iters in S.DUP_TESTED:
            r, screens = profiled(ops, lambda: run(ops, c, iters, poll))
            print(f"\n{tag}-p2plane@{iters} poll_interval {poll}: nn_screen launches {screens}")
            if poll != 1 or iters == 5:
                assert screens > 0, (tag, iters, poll)
            check(oracle, c, r, f"{tag}-p2plane@{iters} poll {poll}", iters, every_row=True)
    finally:
        ops.nn_engine(prev)


# ---- 6 .. 8. large rotation, pairs that contribute nothing, metres --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.ROTATION_NAMES + S.ZERO_NAMES + ["metres"])
def test_rotation_zero_covariances_metres(ops, oracle, cases, engine, name):
    """a 120 degree start (the source covariances are rotated by the current transform per pair, R Cs R^T), covariances that are
    exactly zero on a tenth of the points (pairs of two add nothing) under L2 and Tukey, and clouds in metres (the translation to
    TOL_T x 1e-3)"""
    c = cases[name]
    r = run(ops, c)
    assert S.admitted(c)
    check(oracle, c, r, f"{name} [{engine}]")


# ---- 9. polling changes nothing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.POLL_NAMES)
def test_poll_interval_changes_nothing_dense(ops, oracle, cases, name):
    """poll_interval 0, 1, 3, 4, 7 on `dense`: the same bits, whether the host sees the stop at once, later or never, and whichever
    sweep ScreenPolicy picks from what it polled"""
    c = cases[name]
    prev = ops.nn_engine("dense")
    try:
        runs = {}
        for poll in S.POLLS:
            runs[poll], screens = profiled(ops, lambda: run(ops, c, poll=poll))
            print(f"\n{name} poll_interval {poll}: iterations {runs[poll]['iterations']}, nn_screen launches {screens}")
    finally:
        ops.nn_engine(prev)
    first = runs[S.POLLS[0]]
    check(oracle, c, first, name)
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)
    for poll, r in runs.items():
        assert np.array_equal(bits(r["transformation"]), bits(first["transformation"])), (name, poll)
        assert bits(r["fitness"]) == bits(first["fitness"]) and bits(r["inlier_rmse"]) == bits(first["inlier_rmse"]), (name, poll)
        assert r["iterations"] == first["iterations"] and r["count"] == first["count"], (name, poll)
        if "idx" in r:
            assert np.array_equal(r["idx"], first["idx"]) and np.array_equal(bits(r["d2"]), bits(first["d2"])), (name, poll)
    assert (first["iterations"] < c.iters) == c.converges, name
