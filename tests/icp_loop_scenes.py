"""Scenes for the search -> sums -> solve loop of the registrations (icp_search_solve_loop): generalized ICP, coloured ICP and
point-to-plane ICP at the size edges of the merge and solve kernels, the target-column edges of the screened search, unequal
clouds, rows without partners, duplicated target points that overflow the candidate list of the screened search, a large
rotation, pairs that contribute nothing, metres, and host polling.  tests/test_icp_loop_cpu.py asserts the conditions each scene
is built for on the float64 restatements alone; tests/test_icp_loop_gpu.py runs the library on the same inputs.

Everything here is host arithmetic: covariances, normals and colour gradients come from the oracle, once, and go to the
restatement and to the library alike.  `O` is the oracle module, `base` the rendered frame cloud (the session fixtures).

Tolerance rule (tests/test_robust_gpu.py's).  The transform tolerance is TOL_T = 1e-8, absolute.  A case is ADMITTED to the
comparison of transforms only if 100 x spread <= TOL_T, the spread being the largest difference in the restatement's T between
order=None and the order seeds 1..5 (robust_ref's `order`), measured on the CPU at every max_iteration the GPU suite runs the case
at.  The SPREAD table below holds an upper bound per case, three times the measured spread (the room for another BLAS or NumPy
build's order of sums); the rule is applied to the bound, and test_icp_loop_cpu.py measures each spread again and holds it to its
bound.  A case whose reference does not reproduce itself is in EXACT_ONLY with its measured spread: it runs on the device all the
same, and is held to what does not depend on any order of sums -- the correspondences of the search at the device's own returned
transform, bit for bit against oracle.nn, fitness and count from them exactly, and a finite transform.

What was reshaped or dropped because the reference did not reproduce itself, with the measured spreads: the one-iteration runs
of fewer than ten source rows (TINY_DROPPED), the target of one point (EXACT_ONLY), the fixed source of the target-column cases
(target_edge_cases: 500 rows, 100 of them sampled around the first target point, where 300 rows of the pair's source gave 4.5e4
at one target point) and the starts of the random problems (random_cases)."""
import types

import numpy as np

import gicp_ref as G
import robust_ref as R
from kinectpy_amd.utils import synth

TOL_T = 1e-8
ORDER_SEEDS = (1, 2, 3, 4, 5)
SOURCE_COUNTS = (1, 2, 5, 63, 64, 65, 1024, 1025, 8193)
TINY = 10                                   # fewer source rows than this: the 6x6 system is near singular (see TINY_DROPPED)
TARGET_COUNTS = (1, 15, 16, 17, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2049)
# copies of P.  A row whose bound is a copy lists the copies - 1 others: 65 copies = the list exactly full, 66 the first overflow;
# a row that comes to P from elsewhere lists all of them: 64 copies = the list exactly full, 65 the first overflow
DUPLICATES = (60, 64, 65, 66, 70, 200)
K_CAND = 64                                 # kCand (kpx_icpdefs.h)
EVERY_SEARCH = (0, 1, 2, 3, 4, 6)
DUP_TESTED = (2, 3, 5)                      # the duplicate scenes: compared after 2, 3 and 5 iterations
POLLS = (0, 1, 3, 4, 7)
TUKEY_K = 25.0

# Upper bounds of the restatement's spread per iterating case (see the module docstring): three times the spread measured on the
# CPU (at least 3e-12), rounded up; the largest measured one is 3.03e-11 (tgt1025).  Absent and not in EXACT_ONLY: the case does not
# iterate (max_iteration 0, or nothing within max_dist) and its transform is the start exactly.
SPREAD = {
    "src5-gicp@1": 3e-12, "src63-gicp": 2e-11, "src63-colored": 3e-12, "src64-gicp": 6e-12, "src64-colored": 3e-12,
    "src65-gicp": 1e-11, "src65-colored": 3e-12, "src1024-gicp": 8e-12, "src1024-colored": 3e-12, "src1025-gicp": 4e-12,
    "src1025-colored": 3e-12, "src8193-gicp": 3e-12, "src8193-colored": 3e-12, "tgt15": 2e-11, "tgt16": 2e-11,
    "tgt17": 2e-11, "tgt255": 4e-11, "tgt256": 4e-11, "tgt257": 4e-11, "tgt511": 6e-11, "tgt513": 2e-11, "tgt1023": 6e-11,
    "tgt1024": 6e-11, "tgt1025": 9.1e-11, "tgt2049": 3e-11, "every-search": 8e-12, "random0": 6e-11, "random1": 3e-12,
    "random2": 3e-12, "random3": 1e-11, "random4": 3e-12, "random5": 3e-12, "random6": 2e-11, "random7": 3e-12,
    "dup60-gicp": 2e-11, "dup60-p2plane": 3e-12, "dup64-gicp": 2e-11, "dup64-p2plane": 3e-12, "dup65-gicp": 5e-12,
    "dup65-p2plane": 3e-12, "dup66-gicp": 8e-12, "dup66-p2plane": 3e-12, "dup70-gicp": 5e-12, "dup70-p2plane": 3e-12,
    "dup200-gicp": 8e-12, "dup200-p2plane": 3e-12, "dup64-last-gicp": 1e-11, "dup64-last-p2plane": 3e-12,
    "dup200x1100-gicp": 1e-11, "dup200x1100-p2plane": 3e-12, "rot120-raw": 4e-11, "rot120-normals": 3e-12,
    "rot120-aniso": 3e-12, "zero-cov-l2": 5e-12, "zero-cov-tukey": 7e-12, "metres": 2e-11, "poll-gicp-converges": 5e-12,
    "poll-colored-converges": 3e-12, "poll-p2plane-converges": 3e-12, "poll-gicp-runs-out": 8e-12,
    "poll-colored-runs-out": 3e-12, "poll-p2plane-runs-out": 3e-12,
}
# The case whose reference does not reproduce itself, with its measured spread, compared through the correspondences only.  A
# target of one point leaves the rotation about that point to the anisotropy of the covariances alone: 4.7e-11 as committed, 9.8e-11
# from 7 mm off, 1.3e-10 with 300 rows -- at the limit of the rule whatever the knobs, so it is not admitted.
EXACT_ONLY = {"tgt1": 1.3e-10}

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def case(name, kind, src, tgt, max_dist, init, iters, loss=("l2", 0.0), **inputs):
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, dtype=np.float32).reshape(-1, 3)
    init = None if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    return types.SimpleNamespace(name=name, kind=kind, src=src, tgt=tgt, max_dist=float(max_dist), init=init, iters=int(iters), loss=loss,
                                 t_scale=1.0, **inputs)


def with_iters(c, iters, name=None):
    d = dict(vars(c))
    d.update(iters=int(iters), name=name or f"{c.name}@{iters}")
    return types.SimpleNamespace(**d)


def reference(O, c, order=None, iters=None):
    """the float64 restatement of the case -> T, fitness, rmse, iterations, (idx, d2) of the last search"""
    iters = c.iters if iters is None else iters
    kind, k = c.loss
    if c.kind == "gicp":
        if order is None and kind == "l2":
            return G.registration_generalized_icp(O, c.src, c.tgt, c.max_dist, c.cs, c.ct, c.init, iters)
        return R.registration_generalized_icp_robust(O, c.src, c.tgt, c.max_dist, c.cs, c.ct, kind, k, c.init, iters, order=order)
    if c.kind == "colored":
        # (with L2 and order=None: oracle.registration_colored_icp bit for bit, and it keeps the last search)
        return R.registration_colored_icp_robust(O, c.src, c.sc, c.tgt, c.tc, c.tn, c.max_dist, kind, k, c.init, 0.968, iters, order=order,
                                                 tgt_gradient=c.grad)
    if c.kind == "p2plane":
        # (with L2 and order=None: oracle.registration_icp bit for bit, and it keeps the last search)
        return R.registration_icp_robust(O, c.src, c.tgt, c.tn, c.max_dist, kind, k, c.init, iters, order=order)
    raise ValueError(c.kind)


def ref(O, c):
    return _once(("ref", c.name), lambda: reference(O, c))


def tested_iters(c):
    """the max_iteration values the GPU suite runs the case at"""
    return EVERY_SEARCH if c.name == "every-search" else DUP_TESTED if c.name.startswith("dup") else (c.iters,)


def spread(O, c):
    """largest |T(order=None) - T(order=seed)| over ORDER_SEEDS and over tested_iters (transform_error: in the units the tolerance
    is applied in)"""
    worst = 0.0
    for iters in tested_iters(c):
        if iters > 0:
            T0 = ref(O, c if iters == c.iters else with_iters(c, iters))[0]
            worst = max([worst] + [transform_error(c, reference(O, c, order=s, iters=iters)[0], T0) for s in ORDER_SEEDS])
    return worst


def admitted(c):
    return c.name not in EXACT_ONLY and 100.0 * SPREAD.get(c.name, 0.0) <= TOL_T


def rot(axis, deg):
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def near_start(T, mm=(15.0, -10.0, 5.0)):
    """the truth moved by `mm` in the source's frame (the perturbed start of the existing GICP tests)"""
    pert = np.linalg.inv(T).copy()
    pert[:3, 3] += mm
    return np.linalg.inv(pert)


def _normals(O, pts, radius=1e150, max_nn=20):
    return O.estimate_normals(pts, radius, max_nn)[0].astype(np.float32)


# ---- the shared clouds ------------------------------------------------------------------------------------------------------------
def pair3000(O, base):
    """synth.icp_pair(3000) with raw covariances (KNN 30) of both clouds and the target's normals (KNN 20)"""
    def make():
        src, tgt, T = synth.icp_pair(3000, base)
        return types.SimpleNamespace(src=src, tgt=tgt, T=T, cs=G.estimate_covariances(O, src, 1e150, 30),
                                     ct=G.estimate_covariances(O, tgt, 1e150, 30), tn=_normals(O, tgt))
    return _once("pair3000", make)


def source8193(O, base):
    """a second sampling of the surface, 8193 rows in the source's frame, with its raw covariances"""
    def make():
        src = synth.icp_pair(8193, base)[0]
        return src, G.estimate_covariances(O, src, 1e150, 30)
    return _once("source8193", make)


def coloured3000(O):
    def make():
        src, sc, tgt, tc, T = synth.coloured_pair(3000)
        tn = _normals(O, tgt, 70.0, 30)
        return types.SimpleNamespace(src=src, sc=sc, tgt=tgt, tc=tc, T=T, tn=tn, grad=O.color_gradient(tgt, tn, tc, 160.0, 30))
    return _once("coloured3000", make)


def coloured_source8193(O):
    """coloured_pair(8193)'s source: the same field and motion as coloured_pair(3000), another sampling"""
    return _once("coloured8193", lambda: synth.coloured_pair(8193)[:2])


# ---- 1. source-row edges -----------------------------------------------------------------------------------------------------------
SOURCE_ITERS = 6
# Counts below TINY iterate once only where the 6x6 system is determined and the restatement reproduces itself; dropped at one
# iteration, with the reason: one row gives 3 (GICP) or 2 (coloured) equations for 6 unknowns and two coloured rows 4 -- a singular
# system, where the device's rank test and np.linalg.solve need not agree -- two GICP rows give exactly 6 (spread 6.5e-2) and five
# coloured rows 10 (spread 1.1e-7).  Five GICP rows (15 equations) pass.
TINY_DROPPED = {(1, "gicp", 1): "singular", (1, "colored", 1): "singular", (2, "colored", 1): "singular", (2, "gicp", 1): 6.5e-2,
                (5, "colored", 1): 1.1e-7}


def source_edge_cases(O, base):
    """GICP and coloured ICP with 1 .. 8193 source rows against ~3000 target points: the merge kernel's 64-row blocks with and
    without a tail, the solve kernel's 16 slices (1024 rows: one block each; 1025: slices with nothing; 8193: 129 blocks, 9 per
    slice, the unrolled loop plus a tail).  Counts below TINY run at max_iteration 0, and at 1 where the spread admits it."""
    def make():
        p, col = pair3000(O, base), coloured3000(O)
        big, big_cs = source8193(O, base)
        csrc, csc = coloured_source8193(O)
        out = []
        for n in SOURCE_COUNTS:
            src, cs = (big, big_cs) if n > 3000 else (p.src[:n], p.cs[:n])
            s2, c2 = (csrc, csc) if n > 3000 else (col.src[:n], col.sc[:n])
            for iters in ((0, 1) if n < TINY else (SOURCE_ITERS,)):
                tag = f"@{iters}" if n < TINY else ""
                if (n, "gicp", iters) not in TINY_DROPPED:
                    out.append(case(f"src{n}-gicp{tag}", "gicp", src, p.tgt, 100.0, near_start(p.T), iters, cs=cs, ct=p.ct))
                if (n, "colored", iters) not in TINY_DROPPED:
                    out.append(case(f"src{n}-colored{tag}", "colored", s2, col.tgt, 80.0, near_start(col.T), iters, sc=c2, tc=col.tc, tn=col.tn,
                                    grad=col.grad))
        return out
    return _once("source_edges", make)


# ---- 2. target-column edges under screening ---------------------------------------------------------------------------------------------
TARGET_ROWS, TARGET_ITERS, TARGET_FIRST = 500, 5, 2


def target_edge_cases(O, base):
    """GICP, 300 source rows against the first 1 .. 2049 points of the target (counted from TARGET_FIRST, a point on the person's
    curved surface): a 16-column tile, the culled engine's 256-column group, the fp64 stage of 512 columns and the float32 stage of
    1024 columns with its second stage and split.  The 300 rows are fixed: 200 rows of the pair's source and 100 further samples of
    the surface within 60 mm of the first target point, so that the one-point target keeps ~100 partners (when the target has one
    point every row's partner is that point, or none)."""
    def make():
        p = pair3000(O, base)
        rng = np.random.default_rng(5)
        tgt, ct = p.tgt[TARGET_FIRST:], p.ct[TARGET_FIRST:]
        near = np.flatnonzero(np.linalg.norm(base.astype(np.float64) - tgt[0], axis=1) < 60.0)
        Ti = np.linalg.inv(p.T)
        dense = base[rng.choice(near, 100, replace=False)].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(scale=1.0, size=(100, 3))
        src = np.concatenate([p.src[:TARGET_ROWS - 100], dense.astype(np.float32)])[rng.permutation(TARGET_ROWS)]
        cs = G.estimate_covariances(O, src, 1e150, 30)
        return [case(f"tgt{m}", "gicp", src, tgt[:m], 100.0, near_start(p.T), TARGET_ITERS, cs=cs, ct=ct[:m]) for m in TARGET_COUNTS]
    return _once("target_edges", make)


# ---- 3. every search of a run ----------------------------------------------------------------------------------------------------------
def every_search_case(O, base):
    """1000 x 3000 from 15 mm off the truth; run at max_iteration = EVERY_SEARCH"""
    p = pair3000(O, base)
    return _once("every_search", lambda: case("every-search", "gicp", p.src[:1000], p.tgt, 100.0, near_start(p.T), 6, cs=p.cs[:1000], ct=p.ct))


# ---- 4. unequal sizes, rows without partners ------------------------------------------------------------------------------------------------
RANDOM_CASES, RANDOM_ITERS = 8, 8


def random_cases(O, base):
    """eight seeded GICP problems in the manner of test_icp_random_problems_match_oracle: n and m independent in 100 .. 3000, a third
    with partial overlap, max_dist from {40, 100, 300}, covariances raw / from normals / identity.  The motion is the truth of
    synth.icp_pair seen from a start up to ~1.5 deg / 20 mm off (a nearer start than the plain-ICP fuzz: the knob of the rule)."""
    def make():
        rng = np.random.default_rng(47)
        T = synth.t_star()
        Ti = np.linalg.inv(T)
        out = []
        for k in range(RANDOM_CASES):
            n, m = int(rng.integers(100, 3001)), int(rng.integers(100, 3001))
            tgt = base[rng.choice(len(base), m, replace=False)]
            src0 = base[rng.choice(len(base), n, replace=False)].astype(np.float64)
            partial = k % 3 == 0
            if partial:
                src0 = np.concatenate([src0[src0[:, 0] > np.median(src0[:, 0]) - 200],
                                       src0[:len(src0) // 8] + np.array([0.0, -900.0, 0.0])])      # and rows that see nothing
            src = (src0 @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(scale=1.0, size=src0.shape)).astype(np.float32)
            md = float(rng.choice([40.0, 100.0, 300.0]))
            cov = ("raw", "normals", "identity")[k % 3 if k < 6 else int(rng.integers(0, 3))]
            if cov == "raw":
                cs, ct = G.estimate_covariances(O, src, 1e150, 30), G.estimate_covariances(O, tgt, 1e150, 30)
            elif cov == "normals":
                cs, ct = G.covariances_from_normals(_normals(O, src)), G.covariances_from_normals(_normals(O, tgt))
            else:
                cs, ct = np.broadcast_to(np.eye(3), (len(src), 3, 3)).copy(), np.broadcast_to(np.eye(3), (m, 3, 3)).copy()
            init = synth.perturb(T, float(rng.uniform(0.2, 1.5)), float(rng.uniform(3.0, 20.0)), seed=100 + k)
            out.append(case(f"random{k}", "gicp", src, tgt, md, init, RANDOM_ITERS, cs=cs, ct=ct, partial=partial, cov=cov))
        return out
    return _once("random", make)


def nothing_in_reach_cases(O, base):
    """one GICP and one coloured run whose source lies 5 m from the target: fitness 0, the start returned"""
    def make():
        p, col = pair3000(O, base), coloured3000(O)
        off = np.array([0.0, -5000.0, 0.0], np.float32)
        init = near_start(p.T)
        return [case("nothing-gicp", "gicp", p.src[:700] + off, p.tgt[:900], 100.0, init, 5, cs=p.cs[:700], ct=p.ct[:900]),
                case("nothing-colored", "colored", col.src[:700] + off, col.tgt, 80.0, near_start(col.T), 5, sc=col.sc[:700], tc=col.tc, tn=col.tn,
                     grad=col.grad)]
    return _once("nothing", make)


# ---- 5. candidate-list overflow -------------------------------------------------------------------------------------------------------------
DUP_TARGET, DUP_ROWS, DUP_ITERS, DUP_REGULAR = 2000, 40, 5, 400
MANY_ROWS, MANY_COPIES = 1100, 200          # more overflowing rows than the overflow kernel has blocks (1024)
Q_AT = 777                                  # the index of Q, the lone target point the switching rows come from or go to
ONE_STAGE = 1000                            # a target within one float32 stage: one split, a row's candidates are listed in index order
# tag -> (copies, rows per group, target points, where the switching rows go, Q behind every copy in the index order).
# Rows that go to P need the LOWEST-index copy, which the sweep lists first; rows that go to Q need the candidate that is listed
# last where Q has the highest index: in the 64th slot of a list that is exactly full (dup64-last: 63 ties and Q, one split), and
# behind the first 64 of a list that overflows (the scene of many rows).
DUP_SCENES = {**{f"dup{d}": (d, DUP_ROWS, DUP_TARGET, "P", False) for d in DUPLICATES},
              "dup64-last": (64, DUP_ROWS, ONE_STAGE, "Q", True),
              f"dup{MANY_COPIES}x{MANY_ROWS}": (MANY_COPIES, MANY_ROWS, DUP_TARGET, "Q", True)}
# the (screened) searches at which a group of rows changes between Q and P.  GICP has converged too far by search 3: its cloud
# moves by 1e-3 mm at P then, too little to place rows by
SWITCH_AT = {"gicp": (2,), "p2plane": (2, 3)}
P_COV = np.diag([4.0, 9.0, 2.0])            # every copy's covariance
ROW_COV = np.diag([3.0, 2.0, 5.0])          # the cluster rows' (a few mm of noise around P) and the switching rows' (never used)


# The starts: far enough that the cloud still moves at P between the searches (the switching rows' margins: 0.2 mm for GICP from
# 1 deg / 20 mm, 0.8 and 0.3 mm for point-to-plane from 18 mm), near enough for the cluster to be within max_dist throughout and
# for ScreenPolicy to find the point-to-plane run calm at search 3
DUP_START = {"gicp": lambda T: synth.perturb(T, 1.0, 20.0, seed=3), "p2plane": near_start}
SWITCH_MARGIN = 1e-3                        # mm from the bisecting plane, at the least: ten times what a transform within TOL_T moves a row by


def duplicate_case(O, base, tag, kind):
    """The scene DUP_SCENES[tag]: a target of which `copies` points are exact copies of one point P, 900 mm beyond the cloud's
    bounding box, at indices spread evenly over the whole range (both ends included: with DUP_TARGET points different stages and
    splits of the screening sweep; where Q comes behind every copy it has the last index and the last 16-column tile to itself), and one is Q, 600 mm from P.  Every copy has the covariance P_COV and the normal (0, 0, 1).  The source:
      - DUP_REGULAR rows on the surface;
      - `rows` CLUSTER rows within a few mm of P under the truth.  From the third search on (the first screened one) such a row's
        bound is the exact metric of its previous partner, the lowest-index copy; the copies - 1 others tie with it exactly and
        are candidates whatever the float32 error term: 65 copies fill the 64 slots, 66 overflow.  The row's answer is its bound's
        partner again, so the cluster pins that an overflowing or full list does no harm, not what resolves it;
      - per search k of SWITCH_AT[kind] `rows` SWITCHING rows, 300 mm from P and from Q, that lie on one side of the bisecting plane at
        search k - 1 and on the other at search k (on Q's side first where they go to P).  They are beyond max_dist and add nothing to any sum, so the transforms of the
        run are those of the scene without them, and the rows are placed from these: the midpoint of each row's motion between
        the two searches lies on the plane.  A row that goes from Q to P has all `copies` copies below its bound: its answer, the
        lowest-index copy, comes from the candidate list (copies <= 64) or from the overflow kernel (copies > 64) and from nowhere
        else; a row that goes from P to Q has Q and the copies - 1 ties.  On the all-pairs engines the search returns the
        partners of rows beyond max_dist too, and the tests compare them.
    -> the case, with scene = namespace(P, Q, at, cluster, switching {k: mask})"""
    copies, rows, m, toward, q_last = DUP_SCENES[tag]

    def make():
        p = pair3000(O, base)
        rng = np.random.default_rng(1000 + copies + rows)
        tgt = p.tgt[:m].copy()
        ct, tn = p.ct[:m].copy(), p.tn[:m].copy()
        q_at = m - 1 if q_last else Q_AT
        at = np.unique(np.rint(np.linspace(0, m - 18 if q_last else m - 1, copies)).astype(np.int64))
        assert len(at) == copies and q_at not in at
        keep = np.setdiff1d(np.arange(m), np.append(at, q_at))
        lo, hi = tgt[keep].min(0).astype(np.float64), tgt[keep].max(0).astype(np.float64)
        P = np.array([hi[0] + 900.0, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])]).round()
        tgt[at] = P.astype(np.float32)
        ct[at], tn[at] = P_COV, np.array([0.0, 0.0, 1.0], np.float32)
        Ti = np.linalg.inv(p.T)
        cluster = (P + rng.normal(scale=2.0, size=(rows, 3))) @ Ti[:3, :3].T + Ti[:3, 3]
        src = np.concatenate([p.src[:DUP_REGULAR], cluster.astype(np.float32)])
        cs = np.concatenate([p.cs[:DUP_REGULAR], np.broadcast_to(ROW_COV, (rows, 3, 3))])
        mix = rng.permutation(len(src))
        src, cs, core_role = src[mix], cs[mix], np.where(np.arange(len(src)) < DUP_REGULAR, 0, 1)[mix]
        init = DUP_START[kind](p.T)
        inputs = dict(cs=cs, ct=ct) if kind == "gicp" else dict(tn=tn)

        # the transforms of searches 1, 2, 3 (Q where it disturbs nothing: no row comes near it)
        tgt[q_at] = (P + np.array([600.0, 0.0, 0.0])).astype(np.float32)
        switch_at = SWITCH_AT[kind]
        core = case("core", kind, src, tgt, 100.0, init, max(switch_at), **inputs)
        Ts = {k: reference(O, core, iters=k)[0] for k in range(min(switch_at) - 1, max(switch_at) + 1)}
        step = lambda k, w: w - (w @ np.linalg.inv(Ts[k])[:3, :3].T + np.linalg.inv(Ts[k])[:3, 3]) @ Ts[k - 1][:3, :3].T - Ts[k - 1][:3, 3]
        d = step(min(switch_at), P[None])[0]                      # how a point near P moves from search 1 to search 2
        u = (-d if toward == "P" else d) / np.linalg.norm(d)        # Q lies behind the rows (they go to P) or ahead of them
        Q = (P + 600.0 * u).round()
        u = (Q - P) / np.linalg.norm(Q - P)
        tgt[q_at] = Q.astype(np.float32)
        groups, margins = [], {}
        for k in switch_at:
            lateral = rng.uniform(-40.0, 40.0, size=(rows, 3))
            w = 0.5 * (P + Q) + lateral - (lateral @ u)[:, None] * u                       # on the bisecting plane
            for _ in range(3):                                                                # ... the midpoint of the motion k - 1 -> k
                w += ((0.5 * step(k, w) - (w - 0.5 * (P + Q))) @ u)[:, None] * u
            margins[k] = float(np.abs(step(k, w) @ u).min() / 2)
            groups.append((w @ np.linalg.inv(Ts[k])[:3, :3].T + np.linalg.inv(Ts[k])[:3, 3]).astype(np.float32))
        # (the rows that enter the sums keep their order: the transforms stay those the groups were placed from, bit for bit)
        role = np.concatenate([np.full(rows, 10 + switch_at[0]), core_role] + [np.full(rows, 10 + k) for k in switch_at[1:]])
        src = np.concatenate([groups[0], src] + groups[1:])
        fill = np.broadcast_to(ROW_COV, (rows, 3, 3))
        cs = np.concatenate([fill, cs] + [fill] * (len(switch_at) - 1))
        order = np.arange(len(src))
        scene = types.SimpleNamespace(P=P, Q=Q, at=at, q_at=q_at, toward=toward, cluster=role == 1, switching={k: role == 10 + k for k in switch_at}, margins=margins,
                                      core_T=Ts)
        inputs = dict(cs=cs[order], ct=ct) if kind == "gicp" else dict(tn=tn)
        return case(f"{tag}-{kind}", kind, src[order], tgt, 100.0, init, DUP_ITERS, scene=scene, copies=copies, rows=rows, **inputs)
    return _once(("dup", tag, kind), make)


def duplicate_cases(O, base):
    """GICP and plain point-to-plane ICP on the scenes of DUP_SCENES: DUPLICATES copies with DUP_ROWS rows per group, the full list
    whose last slot decides, and MANY_COPIES copies with MANY_ROWS rows per group (the overflow kernel's blocks each take more
    than one listed row)"""
    return [duplicate_case(O, base, tag, kind) for tag in DUP_SCENES for kind in ("gicp", "p2plane")]


# ---- 6. large rotation ---------------------------------------------------------------------------------------------------------------------------
ROT120 = rot([1.0, 1.0, 1.0], 120.0)
FRAME = rot([0.3, -0.5, 0.8], 40.0)
ANISO = FRAME @ np.diag([1e-3, 1.0, 1.0]) @ FRAME.T           # a hand-made covariance: thin along FRAME's first axis


def rotation_cases(O, base):
    """the 1000-row source turned by 120 deg about (1, 1, 1) / sqrt 3 about its centroid BEFORE its covariances are estimated; the
    start is the inverse rotation (composed with the truth) plus 10 mm.  Raw covariances, covariances from normals, and one
    iteration with ANISO on every source point (the scene that tells R Cs R^T from R^T Cs R: test_icp_loop_cpu.py)."""
    def make():
        p = pair3000(O, base)
        s0 = p.src[:1000].astype(np.float64)
        c = s0.mean(0).round()
        src = ((s0 - c) @ ROT120.T + c).astype(np.float32)
        U = np.eye(4)                                            # src -> the original source frame
        U[:3, :3] = ROT120.T
        U[:3, 3] = c - ROT120.T @ c
        init = near_start(p.T, (6.0, -5.0, 6.0)) @ U             # ~10 mm from the truth p.T @ U
        ctn = G.covariances_from_normals(p.tn)
        aniso = np.broadcast_to(ANISO, (1000, 3, 3)).copy()
        return [case("rot120-raw", "gicp", src, p.tgt, 100.0, init, 6, cs=G.estimate_covariances(O, src, 1e150, 30), ct=p.ct, truth=p.T @ U),
                case("rot120-normals", "gicp", src, p.tgt, 100.0, init, 6, cs=G.covariances_from_normals(_normals(O, src)), ct=ctn,
                     truth=p.T @ U),
                case("rot120-aniso", "gicp", src, p.tgt, 100.0, init, 1, cs=aniso, ct=ctn, truth=p.T @ U)]
    return _once("rotation", make)


# ---- 7. some pairs contribute nothing ------------------------------------------------------------------------------------------------------------
def zero_covariance_cases(O, base):
    """1000 x 3000 with the covariances exactly zero on ~10 % of the target points and on the source rows whose first partner is
    one of them (and as many other rows): a pair of two zero covariances has M == 0 under any rotation and adds nothing, on both
    sides; a pair with one keeps the other's.  L2 and Tukey."""
    def make():
        p = pair3000(O, base)
        rng = np.random.default_rng(77)
        src, init = p.src[:1000], near_start(p.T)
        tz = np.zeros(len(p.tgt), bool)
        tz[rng.choice(len(p.tgt), 300, replace=False)] = True
        idx, d2, _ = O.nn(src, init, p.tgt, grid=True)
        sz = tz[idx] & (d2 < 100.0 ** 2)
        others = np.flatnonzero(~sz)
        sz[rng.choice(others, int(sz.sum()), replace=False)] = True
        cs, ct = p.cs[:1000].copy(), p.ct.copy()
        cs[sz], ct[tz] = 0.0, 0.0
        extra = dict(src_zero=sz, tgt_zero=tz, cs_full=p.cs[:1000], ct_full=p.ct)
        return [case("zero-cov-l2", "gicp", src, p.tgt, 100.0, init, 6, cs=cs, ct=ct, **extra),
                case("zero-cov-tukey", "gicp", src, p.tgt, 100.0, init, 6, ("tukey", TUKEY_K), cs=cs, ct=ct, **extra)]
    return _once("zero_cov", make)


# ---- 8. metres -------------------------------------------------------------------------------------------------------------------------------------
def metres_case(O, base):
    """the 1000-row pair scaled by 1e-3 as float32, max_dist 0.1, covariances estimated on the scaled clouds; the translation is held
    to TOL_T x 1e-3 (t_scale), the same physical length"""
    def make():
        p = pair3000(O, base)
        src, tgt = (p.src[:1000].astype(np.float64) * 1e-3).astype(np.float32), (p.tgt[:1000].astype(np.float64) * 1e-3).astype(np.float32)
        T = p.T.copy()
        T[:3, 3] *= 1e-3
        c = case("metres", "gicp", src, tgt, 0.1, near_start(T, (0.015, -0.010, 0.005)), 10, cs=G.estimate_covariances(O, src, 1e150, 30),
                 ct=G.estimate_covariances(O, tgt, 1e150, 30))
        c.t_scale = 1e-3
        return c
    return _once("metres", make)


def transform_error(c, T, T_ref):
    """|dT| with the translation column scaled to the rotation entries' tolerance (t_scale: 1 in millimetres, 1e-3 in metres)"""
    d = np.abs(np.asarray(T) - T_ref)
    d[:3, 3] /= c.t_scale
    return float(d.max())


# ---- 9. polling ------------------------------------------------------------------------------------------------------------------------------------------
def polling_cases(O, base):
    """GICP, coloured ICP and point-to-plane ICP, each once so that the restatement converges before max_iteration (30) and once so
    that it does not (4)"""
    def make():
        p, col = pair3000(O, base), coloured3000(O)
        out = []
        for tag, iters in (("converges", 30), ("runs-out", 4)):
            out.append(case(f"poll-gicp-{tag}", "gicp", p.src[:1000], p.tgt, 100.0, near_start(p.T), iters, cs=p.cs[:1000], ct=p.ct, converges=iters == 30))
            out.append(case(f"poll-colored-{tag}", "colored", col.src[:1000], col.tgt, 80.0, near_start(col.T), iters, sc=col.sc[:1000], tc=col.tc,
                            tn=col.tn, grad=col.grad, converges=iters == 30))
            out.append(case(f"poll-p2plane-{tag}", "p2plane", p.src[:1000], p.tgt, 100.0, near_start(p.T), iters, tn=p.tn, converges=iters == 30))
        return out
    return _once("polling", make)


def screen_policy_allows(trace):
    """ScreenPolicy (kpx_icp.hip) where every iteration is polled, restated: `trace` = (fitness, rmse) of searches 0, 1, ...; ->
    the searches k >= 2 that may take the screened sweep (calm: the poll after search k - 1 saw fitness move by <= 0.02 and rmse by
    <= 5 % against search k - 2)"""
    out = []
    for k in range(2, len(trace)):
        (f0, r0), (f1, r1) = trace[k - 2], trace[k - 1]
        if abs(f1 - f0) <= 0.02 and abs(r1 - r0) <= 0.05 * max(r0, 1e-12):
            out.append(k)
    return out


# the names of the cases per group, known without building anything (for parametrised tests)
SOURCE_NAMES = [f"src{n}-{kind}" + (f"@{it}" if n < TINY else "") for n in SOURCE_COUNTS for it in ((0, 1) if n < TINY else (SOURCE_ITERS,))
                for kind in ("gicp", "colored") if (n, kind, it) not in TINY_DROPPED]
TARGET_NAMES = [f"tgt{m}" for m in TARGET_COUNTS]
RANDOM_NAMES = [f"random{k}" for k in range(RANDOM_CASES)]
NOTHING_NAMES = ["nothing-gicp", "nothing-colored"]
DUP_TAGS = list(DUP_SCENES)
ROTATION_NAMES = ["rot120-raw", "rot120-normals", "rot120-aniso"]
ZERO_NAMES = ["zero-cov-l2", "zero-cov-tukey"]
POLL_NAMES = [f"poll-{kind}-{tag}" for tag in ("converges", "runs-out") for kind in ("gicp", "colored", "p2plane")]


def all_cases(O, base):
    """every case that is compared with the restatement (name -> case)"""
    cs = (source_edge_cases(O, base) + target_edge_cases(O, base) + [every_search_case(O, base)] + random_cases(O, base)
          + nothing_in_reach_cases(O, base) + duplicate_cases(O, base) + rotation_cases(O, base) + zero_covariance_cases(O, base)
          + [metres_case(O, base)] + polling_cases(O, base))
    out = {c.name: c for c in cs}
    assert len(out) == len(cs)
    return out
