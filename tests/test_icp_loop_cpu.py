"""CPU checks of the scenes in tests/icp_loop_scenes.py, on the float64 restatements alone: every spread of the SPREAD table measured
again, and the condition each scene is built for -- the block and slice counts of the source sizes, rows with and without partners,
the isolation and the ties of the duplicated target point, the covariance rotation that the 120 degree scene tells apart, the pairs
that contribute nothing, the run that converges before max_iteration.  tests/test_icp_loop_gpu.py runs the library on these scenes."""
import numpy as np
import pytest

import gicp_ref as G
import icp_loop_scenes as S


@pytest.fixture(scope="module")
def cases(oracle, base_cloud):
    return S.all_cases(oracle, base_cloud)


def _cdiv(a, b):
    return -(-a // b)


def test_names_are_the_cases(cases):
    names = (S.SOURCE_NAMES + S.TARGET_NAMES + ["every-search"] + S.RANDOM_NAMES + S.NOTHING_NAMES
             + [f"{t}-{k}" for t in S.DUP_TAGS for k in ("gicp", "p2plane")] + S.ROTATION_NAMES + S.ZERO_NAMES + ["metres"] + S.POLL_NAMES)
    assert sorted(names) == sorted(cases)
    assert not set(S.SPREAD) - set(cases) and not set(S.EXACT_ONLY) - set(cases) and not set(S.SPREAD) & set(S.EXACT_ONLY)


def test_spreads_are_within_the_table(oracle, cases):
    """every case that iterates: its spread, measured now, is within its SPREAD entry, and the entry admits it (100 x entry <=
    TOL_T) -- or the case is in EXACT_ONLY and is compared through its correspondences only"""
    worst = 0.0
    for name, c in cases.items():
        T, fit, _, it, _ = S.ref(oracle, c)
        assert np.isfinite(T).all(), name
        iterates = c.iters > 0 and fit > 0
        if not iterates:
            assert name not in S.SPREAD and name not in S.EXACT_ONLY, name
            assert np.array_equal(T, c.init) and it == min(c.iters, 1), name               # nothing to sum: the start, exactly
            continue
        if name in S.EXACT_ONLY:
            assert not S.admitted(c), name
            continue
        sp = S.spread(oracle, c)
        worst = max(worst, sp)
        print(f"{name}: spread {sp:.2e} (entry {S.SPREAD[name]:.1e})")
        assert sp <= S.SPREAD[name], (name, sp)
        assert 100.0 * S.SPREAD[name] <= S.TOL_T and S.admitted(c), name
    print(f"largest spread {worst:.2e}")


def test_l2_references_are_the_named_restatements(oracle, cases):
    """reference() goes through robust_ref's loops for coloured and point-to-plane ICP (they keep the last search): with L2 they are
    oracle.registration_colored_icp and oracle.registration_icp bit for bit"""
    c = cases["src64-colored"]
    a = oracle.registration_colored_icp(c.src, c.sc, c.tgt, c.tc, c.tn, c.max_dist, c.init, 0.968, c.iters)
    b = S.ref(oracle, c)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:4]
    c = cases["dup66-p2plane"]
    a = oracle.registration_icp(c.src, c.tgt, c.max_dist, c.init, "p2plane", c.tn, c.iters)
    b = S.ref(oracle, c)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:4]


def test_source_edges(oracle, cases):
    """the counts are the merge kernel's blocks of 64 rows and the solve kernel's 16 slices; every case has partners, those that
    iterate keep most of them"""
    blocks = {n: _cdiv(n, 64) for n in S.SOURCE_COUNTS}
    per = {n: _cdiv(b, 16) for n, b in blocks.items()}
    assert blocks[63] == blocks[64] == 1 and blocks[65] == 2 and 63 % 64 and 65 % 64                     # a tail, none, a block of one row
    assert blocks[1024] == 16 and per[1024] == 1                                                          # one block per slice
    assert blocks[1025] == 17 and per[1025] == 2 and _cdiv(17, 2) < 16                                    # slices with nothing
    assert blocks[8193] == 129 and per[8193] == 9 and all(per[n] < 8 for n in S.SOURCE_COUNTS if n < 8193)   # first unrolled 8 + a tail
    for name in S.SOURCE_NAMES:
        c = cases[name]
        _, fit, _, it, (idx, d2) = S.ref(oracle, c)
        assert fit > 0 and len(c.src) == int(name[3:].split("-")[0]) and 2900 <= len(c.tgt) <= 3100, name
        if c.iters > 1:
            assert fit > 0.3 and it >= 4, name
        if c.iters == 0:
            assert it == 0, name
    assert set(S.TINY_DROPPED) == {(1, "gicp", 1), (1, "colored", 1), (2, "gicp", 1), (2, "colored", 1), (5, "colored", 1)}
    assert "src5-gicp@1" in cases and all(f"src{n}-{k}@0" in cases for n in (1, 2, 5) for k in ("gicp", "colored"))


def test_target_edges(oracle, cases):
    """the counts are one below, at and above a 16-column tile, the culled engine's 256-column group, the fp64 stage of 512 columns
    and the float32 stage of 1024 columns; every run iterates at least 4 times (searches 2, 3, ... are screened), rows with and
    without partners in each; one target point: that point or none"""
    assert {15, 16, 17, 255, 256, 257, 511, 513, 1023, 1024, 1025} <= set(S.TARGET_COUNTS) and max(S.TARGET_COUNTS) > 2 * 1024
    src = cases["tgt1"].src
    for m in S.TARGET_COUNTS:
        c = cases[f"tgt{m}"]
        _, fit, _, it, (idx, d2) = S.ref(oracle, c)
        ok = d2 < c.max_dist ** 2
        assert len(c.tgt) == m and c.src is src or np.array_equal(c.src, src)
        assert it >= 4 and fit > 0.15 and ok.sum() >= 90 and (~ok).sum() >= 20, (m, it, fit)
    assert (S.ref(oracle, cases["tgt1"])[4][0] == 0).all()


def test_every_search_runs_its_iterations(oracle, cases):
    c = cases["every-search"]
    assert max(S.EVERY_SEARCH) == c.iters and {0, 1, 2, 3} <= set(S.EVERY_SEARCH)
    for k in S.EVERY_SEARCH:
        assert S.reference(oracle, c, iters=k)[3] == k                       # no early stop: search k is the run's last


def test_random_problems(oracle, cases):
    rs = [cases[n] for n in S.RANDOM_NAMES]
    assert len(rs) == 8 and sum(c.partial for c in rs) >= 2 and {c.max_dist for c in rs} == {40.0, 100.0, 300.0}
    assert {c.cov for c in rs} == {"raw", "normals", "identity"}
    assert all(100 <= len(c.tgt) <= 3000 and len(c.src) != len(c.tgt) for c in rs)
    assert min(len(c.src) for c in rs) < 500 and max(len(c.src) for c in rs) > 2000
    for c in rs:
        _, fit, _, it, (idx, d2) = S.ref(oracle, c)
        without = (d2 >= c.max_dist ** 2).mean()
        assert fit > 0.1 and it >= 4, c.name
        if c.partial:
            assert without > 0.08, (c.name, without)                        # rows without a partner within max_dist
    for name in S.NOTHING_NAMES:
        c = cases[name]
        T, fit, rmse, it, (idx, d2) = S.ref(oracle, c)
        assert fit == 0.0 and rmse == 0.0 and it == 1 and np.array_equal(T, c.init) and (d2 >= c.max_dist ** 2).all()


def _trace(oracle, c):
    return [S.reference(oracle, c, iters=k) for k in range(c.iters + 1)]


def test_duplicates(oracle, cases):
    """P is isolated; the copies lie at both ends of the index range and in both float32 stages, with equal covariances; at every
    search of the run the cluster rows have a copy for their partner, always the lowest-index one, from the third search on at a
    few mm -- the other copies tie with the bound exactly: 64 candidates at 65 copies, 65 at 66.  The switching rows of search k
    change between Q and the lowest-index copy at search k, with a margin, and never come within
    max_dist: the transforms are those of the scene without them, bit for bit"""
    assert [d - 1 for d in S.DUPLICATES] == [59, S.K_CAND - 1, S.K_CAND, S.K_CAND + 1, 69, 199]
    assert S.MANY_ROWS > 1024 and S.MANY_COPIES > 2 * S.K_CAND and min(min(v) for v in S.SWITCH_AT.values()) >= 2
    assert [t for t in S.DUP_TAGS if S.DUP_SCENES[t][3] == "P"] == [f"dup{d}" for d in S.DUPLICATES]
    assert S.DUP_SCENES["dup64-last"][0] == S.K_CAND and S.ONE_STAGE <= 1024                 # 63 ties and Q: exactly full, one split
    for tag in S.DUP_TAGS:
        for c in (cases[f"{tag}-gicp"], cases[f"{tag}-p2plane"]):
            s = c.scene
            copies, rows, m, toward, q_last = S.DUP_SCENES[tag]
            assert (c.copies, c.rows, s.toward) == (copies, rows, toward) and s.q_at == (m - 1 if q_last else S.Q_AT)
            assert len(c.tgt) == m and len(s.at) == c.copies and s.cluster.sum() == c.rows
            others = np.setdiff1d(np.arange(len(c.tgt)), s.at)
            assert (c.tgt[s.at] == c.tgt[s.at[0]]).all() and np.array_equal(c.tgt[s.at[0]].astype(np.float64), s.P)
            assert np.array_equal(c.tgt[s.q_at].astype(np.float64), s.Q) and (not q_last or s.q_at // 16 > s.at[-1] // 16)
            assert np.linalg.norm(c.tgt[others].astype(np.float64) - s.P, axis=1).min() >= 500.0
            assert np.linalg.norm(c.tgt[np.setdiff1d(others, [s.q_at])].astype(np.float64) - s.Q, axis=1).min() >= 500.0
            assert s.at[0] == 0 and s.at[-1] >= len(c.tgt) - 18 and ((s.at < 1024).any() and (s.at >= 1024).any() or m == S.ONE_STAGE)
            if c.kind == "gicp":
                assert (c.ct[s.at] == S.P_COV).all()
            else:
                assert (c.tn[s.at] == np.array([0, 0, 1], np.float32)).all()
            trace = _trace(oracle, c)
            assert [r[3] for r in trace][:5] == [0, 1, 2, 3, 4] and c.iters == 5, c.name               # searches 2 .. 4 at the least are screened
            on_copy = [np.isin(r[4][0], s.at) for r in trace]
            for k, (T, fit, rmse, it, (idx, d2)) in enumerate(trace):
                assert on_copy[k][s.cluster].all() and (idx[on_copy[k]] == s.at[0]).all(), (c.name, k)
                assert not on_copy[k][~s.cluster & (d2 < c.max_dist ** 2)].any(), (c.name, k)
                assert d2[s.cluster].max() < (15.0 if k >= 2 else 0.9 * c.max_dist) ** 2 and fit > 0.3, (c.name, k, d2[s.cluster].max())
                if k in s.core_T:
                    assert np.array_equal(T, s.core_T[k]), (c.name, k)
            for k, rows in s.switching.items():
                assert rows.sum() == c.rows and s.margins[k] >= S.SWITCH_MARGIN, (c.name, k, s.margins[k])
                changes = [int((on_copy[j][rows] != on_copy[j - 1][rows]).sum()) for j in range(2, len(trace))]
                assert changes[k - 2] == c.rows, (c.name, k, changes)                          # (a later group may cross at an earlier search too)
                for j, r in enumerate(trace):
                    assert (r[4][1][rows] > (2.0 * c.max_dist) ** 2).all(), (c.name, k, j)                 # never in any sum
                    assert j < 2 or np.isin(r[4][0][rows], np.append(s.at[0], s.q_at)).all(), (c.name, k, j)
            if c.rows == S.MANY_ROWS:                                          # the oracle's grid search is the brute-force one out there too
                idx, d2 = trace[-1][4]
                bi, bd, _ = oracle.nn(c.src, trace[-1][0], c.tgt, grid=False)
                assert np.array_equal(idx, bi) and np.array_equal(d2, bd), c.name
            k0 = S.SWITCH_AT[c.kind][0]
            first = s.switching[k0]
            arrive = int((~on_copy[k0 - 1][first] & on_copy[k0][first]).sum())
            print(f"{c.name}: of the {c.rows} rows that switch at search {k0}, {arrive} come to P and {c.rows - arrive} leave it for Q")
            assert arrive == (c.rows if toward == "P" else 0), c.name
            if c.kind == "p2plane":
                # plain ICP with every iteration polled screens by ScreenPolicy: by the restatement's (fitness, rmse) it screens a
                # search at which a group switches
                allowed = S.screen_policy_allows([(r[1], r[2]) for r in trace])
                assert set(allowed) & set(S.SWITCH_AT[c.kind]), (c.name, allowed)


def test_large_rotation_tells_the_covariance_rotation_apart(oracle, cases):
    for name in S.ROTATION_NAMES:
        c = cases[name]
        R0 = c.init[:3, :3]
        angle = np.degrees(np.arccos((np.trace(R0) - 1) / 2))
        T, fit, _, it, _ = S.ref(oracle, c)
        assert 110.0 < angle < 130.0 and fit > 0.3, (name, angle)
        assert 8.0 < np.linalg.norm(c.init[:3, 3] - c.truth[:3, 3]) and np.abs(c.init[:3, :3] - c.truth[:3, :3]).max() < 1e-12
        assert np.abs(T[:3, 3] - c.truth[:3, 3]).max() < np.abs(c.init[:3, 3] - c.truth[:3, 3]).max(), name
    c = cases["rot120-aniso"]
    assert np.allclose(np.linalg.eigvalsh(S.ANISO), [1e-3, 1.0, 1.0]) and np.abs(S.ANISO - np.diag(np.diag(S.ANISO))).max() > 0.1
    idx, d2, _ = oracle.nn(c.src, c.init, c.tgt, grid=True)
    R0 = c.init[:3, :3]
    good = oracle.p2plane_from_sums(G.gicp_accumulate(oracle, c.src, c.init, c.tgt, idx, d2, c.max_dist, c.cs, c.ct))
    # R (R^T R^T Cs R R) R^T = R^T Cs R: the update of a library that rotated the covariances the wrong way
    wrong_cs = R0.T @ R0.T @ c.cs @ R0 @ R0
    wrong = oracle.p2plane_from_sums(G.gicp_accumulate(oracle, c.src, c.init, c.tgt, idx, d2, c.max_dist, wrong_cs, c.ct))
    assert np.array_equal(S.ref(oracle, c)[0], good @ c.init) and c.iters == 1
    print(f"first update, R Cs R^T against R^T Cs R: {np.abs(good - wrong).max():.3g}")
    assert np.abs(good - wrong).max() > 1e-4


def test_zero_covariance_pairs(oracle, cases):
    for name in S.ZERO_NAMES:
        c = cases[name]
        assert 0.05 < c.src_zero.mean() < 0.3 and 0.05 < c.tgt_zero.mean() < 0.3
        assert not c.cs[c.src_zero].any() and not c.ct[c.tgt_zero].any() and np.array_equal(c.cs[~c.src_zero], c.cs_full[~c.src_zero])
        idx, d2, _ = oracle.nn(c.src, c.init, c.tgt, grid=True)
        ok = d2 < c.max_dist ** 2
        both = ok & c.src_zero & c.tgt_zero[idx]
        W, good = G.pair_weights(c.init[:3, :3], c.cs[ok], c.ct[idx[ok]])
        assert both.sum() >= 30 and np.array_equal(~good, both[ok]) and good.sum() > 600        # exactly the zero-zero pairs drop out
        assert (ok & (c.src_zero ^ c.tgt_zero[idx])).sum() >= 30                              # pairs with one zero covariance stay
    c = cases["zero-cov-l2"]
    idx, d2, _ = oracle.nn(c.src, c.init, c.tgt, grid=True)
    some = oracle.p2plane_from_sums(G.gicp_accumulate(oracle, c.src, c.init, c.tgt, idx, d2, c.max_dist, c.cs, c.ct))
    every = oracle.p2plane_from_sums(G.gicp_accumulate(oracle, c.src, c.init, c.tgt, idx, d2, c.max_dist, c.cs_full, c.ct_full))
    assert np.abs(some - every).max() > 1e-4
    l2, tk = S.ref(oracle, cases["zero-cov-l2"]), S.ref(oracle, cases["zero-cov-tukey"])
    assert cases["zero-cov-tukey"].loss == ("tukey", S.TUKEY_K) and np.abs(l2[0] - tk[0]).max() > 1e-6 and l2[3] >= 4 and tk[3] >= 4


def test_metres(oracle, cases):
    c = cases["metres"]
    assert c.src.dtype == np.float32 and np.abs(c.src).max() < 10.0 and np.abs(c.tgt).max() < 10.0 and c.max_dist == 0.1 and c.t_scale == 1e-3
    assert len(c.src) == len(c.tgt) == 1000 and np.abs(c.cs).max() < 1.0                     # covariances of the scaled clouds (m^2)
    T, fit, rmse, it, _ = S.ref(oracle, c)
    assert fit > 0.3 and it >= 4 and rmse < 0.1
    moved = T.copy()
    moved[0, 3] += 2e-11                                                                      # 2e-8 mm: outside the tolerance
    assert S.transform_error(c, moved, T) > S.TOL_T > S.transform_error(c, T, T)


def test_polling_runs(oracle, cases):
    """of each estimation one run stops early (the restatement converges before max_iteration) and one runs out of iterations; the
    poll intervals include ones shorter than the run and ones whose polls do not fall on the stop"""
    for name in S.POLL_NAMES:
        c = cases[name]
        it = S.ref(oracle, c)[3]
        if c.converges:
            assert 2 <= it < c.iters - 7 and any(0 < p < it for p in S.POLLS) and any((it + 1) % p for p in S.POLLS if p), (name, it)
        else:
            assert it == c.iters == 4, (name, it)
    assert set(S.POLLS) == {0, 1, 3, 4, 7}
