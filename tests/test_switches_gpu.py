"""GPU suite (-m gpu): every KPX_* form switch of tests/switch_matrix.py against INTEGRATION.md's contract that the switches "never
change results".

The switches are read once per process, so each setting runs tests/switch_workers.py in a fresh child (one after another; one
parametrized test per setting) and is compared with its family's default child, which a module-scoped fixture runs once and which
is itself held against the CPU oracle -- otherwise the children would only agree with each other.  Integer and index outputs, voxel
and fused clouds, bounds, nearest-neighbour distances, the culled ICP's and the frame step's results: bit for bit.  Other floats:
the constant of the suite's existing test of that operator, imported from where it is defined.

Evidence that a forced form ran: the library's own launch counters where it has them (prof_begin / prof_end, icp_chain(-2)),
otherwise the dispatch conditions restated in switch_matrix.py, asserted per input.

A child that times out, dies on a signal or reports a GPU fault ends the session (pytest.exit): nothing further starts on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gicp_ref as G
from tests import dbscan_ref, fps_ref
from tests import switch_matrix as M
from tests.test_boundaries_gpu import TOL_STATS, _normals_vs_oracle, voxel_key_bits, voxel_sort_form
from tests.test_parity_gpu import TOL_T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
SOR_AVG_RTOL = 1e-13                      # test_sor_block_kernel_fuzz_ties_duplicates_clusters' bound on the mean distances


def run_child(family, setting, env, tmp):
    """one fresh process for one setting -> its arrays.  Any sign of a GPU fault ends the whole session."""
    out = os.path.join(str(tmp), "%s_%s.npz" % (family, "".join(ch if ch.isalnum() else "_" for ch in setting)))
    full = {**os.environ, **M.FAMILY_ENV.get(family, {}), **env}
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_workers.py"), family, out], cwd=ROOT, env=full,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        tail = (e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or ""))[-2000:]
        pytest.exit("switch child %s [%s] timed out after %d s; nothing further runs on the GPU\n%s" % (family, setting, CHILD_TIMEOUT, tail), returncode=3)
    if r.returncode in (134, 139, -6, -11) or "illegal memory access" in (r.stderr + r.stdout):
        pytest.exit("switch child %s [%s] faulted (exit %d); nothing further runs on the GPU\n%s" % (family, setting, r.returncode, r.stderr[-2000:]), returncode=3)
    assert r.returncode == 0, (family, setting, r.stderr[-3000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def defaults(tmp_path_factory):
    """family -> the arrays of its default child (every switch unset), run once on first use"""
    tmp, got = tmp_path_factory.mktemp("switch_defaults"), {}

    def get(family):
        if family not in got:
            got[family] = run_child(family, "default", {}, tmp)
        return got[family]
    return get


def _same_keys(a, b, ctx):
    assert sorted(a) == sorted(b), (ctx, sorted(set(a) ^ set(b)))


def _bitwise(a, b, keys, ctx):
    bad = []
    for key in keys:
        if not (a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8))):
            same_shape = a[key].shape == b[key].shape
            bad.append((key, float(np.abs(a[key].astype(np.float64) - b[key].astype(np.float64)).max()) if same_shape else (a[key].shape, b[key].shape)))
    for item in bad:
        print("not bit-identical:", ctx, *item)                          # every figure before the assertion
    assert not bad, (ctx, bad[:8])


def _params(family):
    return pytest.mark.parametrize("setting", list(M.FAMILIES[family]))


# ---------------------------------------------------------------------------------------------------------------- grid, SOR, bounds
@pytest.fixture(scope="module")
def grid_oracle(oracle):
    inp = M.grid_inputs()
    ref = {"inputs": inp}
    for name, k, ratio in M.sor_cases():
        ref["sor", name, k] = oracle.sor(inp[name], k, ratio)
    for name in ("halo", "c70k"):
        ref["normals", name] = oracle.estimate_normals(inp[name], *M.NORMALS_ARGS)
    return ref


def _check_normals(got, ref):
    rn, cov, cnt = ref
    _normals_vs_oracle(got.astype(np.float64), rn, cov, cnt, 0.5)


def _grid_floats_vs(z, other_avg, other_stats, other_normals, ctx):
    for name, k, _ in M.sor_cases():
        assert np.allclose(z["sor_%s_%d_avg" % (name, k)], other_avg(name, k), rtol=SOR_AVG_RTOL, atol=0), (ctx, name, k)
        assert np.allclose(z["sor_%s_%d_stats" % (name, k)], other_stats(name, k), rtol=TOL_STATS, atol=0), (ctx, name, k)
    for name in ("halo", "c70k"):
        other_normals(name, z["normals_" + name])


def test_sor_inputs_keep_their_distance_from_the_threshold(grid_oracle):
    """the precondition of comparing keep lists between forms whose sums may differ in the last bits (oracle values alone)"""
    for name, k, ratio in M.sor_cases():
        _, rs, ra = grid_oracle["sor", name, k]
        assert M.sor_margin(ra, rs[2]) > M.SOR_MARGIN, (name, k, ratio)


def test_grid_default_matches_the_oracle(defaults, grid_oracle, oracle):
    z, inp = defaults("grid"), grid_oracle["inputs"]
    for name, k, _ in M.sor_cases():
        ri, _, _ = grid_oracle["sor", name, k]
        assert np.array_equal(z["sor_%s_%d_keep" % (name, k)], ri), (name, k)
    _grid_floats_vs(z, lambda n, k: grid_oracle["sor", n, k][2], lambda n, k: grid_oracle["sor", n, k][1],
                    lambda n, got: _check_normals(got, grid_oracle["normals", n]), "oracle")
    halo = inp["halo"]
    nb, radius = M.RADIUS_ARGS
    indptr, indices = dbscan_ref.oracle_neighbours(oracle, halo, radius, 1024)
    assert np.array_equal(z["radius_halo"], np.flatnonzero(dbscan_ref.counts(indptr) > nb))
    eps, min_points = M.DBSCAN_ARGS
    labels = dbscan_ref.dbscan_loop(*dbscan_ref.oracle_neighbours(oracle, halo, eps, 1024), min_points)
    assert np.array_equal(z["dbscan_halo_labels"], labels) and int(z["dbscan_halo_count"][0]) == labels.max(initial=-1) + 1
    assert labels.max() >= 1 and (labels < 0).any()                     # several clusters and noise: the labels carry information
    box = lambda p: np.concatenate([p.min(0), p.max(0)]).astype(np.float64)
    assert np.array_equal(z["bounds_halo"], box(halo)) and np.array_equal(z["bounds_c70k"], box(inp["c70k"]))
    assert np.array_equal(z["bounds_c66k_aligned"], box(inp["c66k"])) and np.array_equal(z["bounds_c66k_view"], box(inp["c66k"][1:]))


@_params("grid")
def test_grid_sor_bounds_switches(defaults, grid_oracle, tmp_path, setting):
    env, inp = M.FAMILIES["grid"][setting], grid_oracle["inputs"]
    # the inputs sit where the switch matters
    if "KPX_GRID_SORT" in env:
        assert M.grid_build_form(len(inp["halo"]), {}) == "count" and M.grid_build_form(len(inp["halo"]), env) == "sort"
        assert M.grid_build_form(len(inp["c70k"]), {}) == "sort"
    if "KPX_RADIX" in env:
        assert M.grid_build_form(len(inp["c70k"]), {}) == "sort"         # the build that sorts: by the own radix sort unless switched off
    if "KPX_BBOX_VEC" in env:
        assert M.bbox_form(len(inp["c70k"]), True, {}) == "vec" and M.bbox_form(len(inp["c70k"]), True, env) == "scalar"
    if any(name.startswith("KPX_SOR_") and name != "KPX_SOR_OCC" for name in env):
        changed = [k for k in M.SOR_KS if M.sor_pass0(k, env) != M.sor_pass0(k, {})]
        assert changed, setting
    if "KPX_SOR_OCC" in env:
        assert all(M.grid_occupancy(k, env) != M.grid_occupancy(k, {}) for k in M.SOR_KS[1:])
    base, z = defaults("grid"), run_child("grid", setting, env, tmp_path)
    _same_keys(base, z, setting)
    assert list(z["c66k_misalignment"]) == [0, 12] and M.bbox_form(len(inp["c66k"]) - 1, False, {}) == "scalar"
    exact = [key for key in base if key.endswith("_keep") or key.startswith(("radius_", "dbscan_", "bounds_"))]
    assert len(exact) == len(M.sor_cases()) + 7
    _bitwise(base, z, exact, setting)
    _grid_floats_vs(z, lambda n, k: base["sor_%s_%d_avg" % (n, k)], lambda n, k: base["sor_%s_%d_stats" % (n, k)],
                    lambda n, got: _check_normals(got, grid_oracle["normals", n]), setting)
    _grid_floats_vs(z, lambda n, k: grid_oracle["sor", n, k][2], lambda n, k: grid_oracle["sor", n, k][1], lambda n, got: None, (setting, "oracle"))


def test_the_sor_settings_reach_every_pass0_kernel():
    """between them the settings launch every sor_block_kernel<S> and the wave-per-query passes alone (kpx_knn.hip)"""
    reached = {M.sor_pass0(k, env) for env in list(M.FAMILIES["grid"].values()) + [{}] for k in M.SOR_KS}
    assert reached == {None, "block<4>", "block<8>", "block<16>", "block<32>"}
    assert {M.sor_pass0(k, {}) for k in M.SOR_KS} == {None, "block<8>", "block<16>", "block<32>"}       # what the default reaches


# ---------------------------------------------------------------------------------------------------------------- voxel
def test_voxel_default_matches_the_oracle(defaults, oracle):
    z = defaults("voxel")
    inputs, rng = M.voxel_inputs()
    assert voxel_key_bits(inputs["v140k"], M.VOXEL_SIZE) <= 32 and len(inputs["v140k"][0]) > M.VOXEL_READBACK_MIN
    assert voxel_sort_form(inputs["v140k"], M.VOXEL_SIZE) == "own-32" and voxel_sort_form(inputs["ragged"], M.VOXEL_SIZE) == "own-32"
    assert voxel_sort_form(inputs["v20k"], M.VOXEL_SIZE) == "vendor-64"
    for name, clouds in inputs.items():
        cols, nrms = M.voxel_attrs(clouds, rng)
        if name == "fused":
            for tag, c in (("plain", None), ("col", cols)):
                rp, rc = oracle.fuse_voxel_downsample(clouds, c, M.fused_transforms(), M.VOXEL_SIZE)[:2]
                assert np.array_equal(z["fused_%s_p" % tag], rp), tag
                assert c is None or np.array_equal(z["fused_%s_c" % tag], rc), tag
        elif len(clouds) == 1:
            for tag, c, n in (("plain", None, None), ("col", cols[0], None), ("nrm", None, nrms[0])):
                rp, rc, rn = oracle.voxel_downsample(clouds[0], M.VOXEL_SIZE, c, n)
                assert np.array_equal(z["%s_%s_p" % (name, tag)], rp), (name, tag)
                assert c is None or np.array_equal(z["%s_%s_c" % (name, tag)], rc), (name, tag)
                assert n is None or np.array_equal(z["%s_%s_n" % (name, tag)], rn), (name, tag)
        else:
            for tag, c in (("plain", None), ("col", cols)):
                for i, cloud in enumerate(clouds):
                    rp, rc, _ = oracle.voxel_downsample(cloud, M.VOXEL_SIZE, None if c is None else c[i])
                    assert np.array_equal(z["%s_%s_p%d" % (name, tag, i)], rp), (name, tag, i)
                    assert c is None or np.array_equal(z["%s_%s_c%d" % (name, tag, i)], rc), (name, tag, i)


@_params("voxel")
def test_voxel_switches(defaults, tmp_path, setting):
    """KPX_RADIX=0: the vendor sort where the library's own radix sort serves (more than 131072 points, keys of <= 32 bits: v140k and the
    ragged batch); KPX_VOXEL_SINGLE=0: a single cloud without normals through voxel_impl instead of the one-pass batch form"""
    env = M.FAMILIES["voxel"][setting]
    base, z = defaults("voxel"), run_child("voxel", setting, env, tmp_path)
    _same_keys(base, z, setting)
    _bitwise(base, z, list(base), setting)


# ---------------------------------------------------------------------------------------------------------------- culled ICP launch forms
def test_icp_default_matches_the_oracle(defaults, oracle):
    from kinectpy_amd.pipeline import PipelineParams
    from kinectpy_amd.utils import synth
    P, z = PipelineParams(), defaults("icp")
    assert int(z["engine"][0]) == 0                                     # the culled engine
    assert int(z["chains"][0]) == 4                                     # "small" and "alone" of both estimators; the full batches ran launches
    downs = [z["down%d" % i] for i in range(4)]
    blocks = lambda clouds: sum(-(-len(c) // 64) for c in clouds)
    assert blocks(downs[1:]) > M.ICP_CHAIN_BLOCKS >= blocks([downs[1][:9000], downs[2][:7001], downs[3][:12000]])
    for mode in ("p2plane", "p2p"):
        for i in range(3):
            rT, rf, rr, rit = oracle.registration_icp(downs[i + 1], downs[0], P.icp_max_dist, z["inits"][i], mode, z["tn"], P.icp_max_iteration)
            fit, rmse, its, _ = z[mode + "_full_s"][i]
            assert its == rit and fit == rf and abs(rmse - rr) < 1e-9 * max(rr, 1), (mode, i)
            assert np.abs(z[mode + "_full_T"][i] - rT).max() < TOL_T, (mode, i)
        assert z[mode + "_full_s"][:, 2].max() >= 6, mode
    src, sc, tgt, tc, _ = synth.coloured_pair(M.DENSE_N)
    rT, rf, rr, rit = oracle.registration_colored_icp(src, sc, tgt, tc, z["coloured_tn"], 80.0, None, 0.968, 25)
    assert z["coloured_s"][2] == rit and z["coloured_s"][0] == rf and np.abs(z["coloured_T"] - rT).max() < TOL_T
    src, tgt, _ = synth.icp_pair(M.DENSE_N)
    rT, rf, _, rit, _ = G.registration_generalized_icp(oracle, src, tgt, 100.0, z["gicp_cs"], z["gicp_ct"], None, 30)
    assert z["gicp_s"][2] == rit and z["gicp_s"][0] == rf and np.abs(z["gicp_T"] - rT).max() < TOL_T


@_params("icp")
def test_icp_launch_form_switches(defaults, tmp_path, setting):
    """transforms, fitness, rmse, iterations and counts bit for bit (the exact-sum contract of
    test_icp_update_placements_and_light_skip_are_bit_identical), and with them the clouds and normals that went in."""
    env = M.FAMILIES["icp"][setting]
    base, z = defaults("icp"), run_child("icp", setting, env, tmp_path)
    _same_keys(base, z, setting)
    _bitwise(base, z, [key for key in base if key != "chains"], setting)
    # the form did run: without the grouped driver (FUSE / BATCH_LAUNCH 0) and with the chain off no one-launch chain starts; the
    # launch windows (WINDOW) keep the default's four
    grouped = not ({"KPX_ICP_FUSE", "KPX_ICP_BATCH_LAUNCH"} & set(env)) and env.get("KPX_ICP_CHAIN") != "0"
    assert int(z["chains"][0]) == (4 if grouped else 0), setting


# ---------------------------------------------------------------------------------------------------------------- culled ICP, edge sizes
def test_icp_edges_default_matches_the_oracle(defaults, oracle):
    """the default child of the edge-size family: a one-launch chain for every call of at most seven sources, none for eight (the
    per-registration driver), and its 2000-row registrations against the oracle.  The one- and few-row registrations are compared
    among the forms only: their solves are singular."""
    from kinectpy_amd.utils import synth
    z = defaults("icp_edges")
    src, tgt, _ = synth.icp_pair(M.ICP_EDGES_N)
    cases = M.icp_edges_cases(src)
    assert int(z["engine"][0]) == 0                                     # the culled engine
    assert [[len(s) for s in srcs] for srcs, _ in cases[:2]] == [[1], [17, 64, 65, 129]]
    assert [len(srcs) for srcs, _ in cases[2:4]] == [M.ICP_GROUP_MAX, M.ICP_GROUP_MAX + 1] and len(cases[3][0][-1]) == 300 + 7 * M.ICP_GROUP_MAX
    assert z["chains"].tolist() == [[1, 1] if len(srcs) <= M.ICP_GROUP_MAX else [0, 0] for srcs, _ in cases]
    checked = 0
    for ci, (srcs, iters) in enumerate(cases):
        if [len(s) for s in srcs] != [2000]:
            continue
        for mode in ("p2p", "p2plane"):
            rT, rf, _, rit = oracle.registration_icp(srcs[0], tgt, M.ICP_EDGES_MAX_DIST, None, mode, z["tn"], iters)
            fit, _, its, _ = z["%s_%d_s" % (mode, ci)][0]
            err = np.abs(z["%s_%d_T" % (mode, ci)][0] - rT).max()
            print("icp_edges", mode, "max_iteration", iters, "iterations", its, rit, "fitness", fit, rf, "transform error", err)
            assert its == rit and fit == rf, (mode, iters)
            assert err < TOL_T, (mode, iters)
            checked += 1
    assert checked == 4


@_params("icp_edges")
def test_icp_edge_size_switches(defaults, tmp_path, setting):
    """every transform, fitness, rmse, iteration number and count of the edge-size cases bit for bit between the grouped driver's
    default and the setting's form; no setting of the family starts a one-launch chain (per-registration drivers, KPX_ICP_CHAIN=0)"""
    env = M.FAMILIES["icp_edges"][setting]
    assert {"KPX_ICP_BATCH_LAUNCH", "KPX_ICP_CHAIN"} & set(env), setting
    base, z = defaults("icp_edges"), run_child("icp_edges", setting, env, tmp_path)
    _same_keys(base, z, setting)
    _bitwise(base, z, [key for key in base if key != "chains"], setting)
    assert z["chains"].shape == base["chains"].shape and not z["chains"].any(), setting


# ---------------------------------------------------------------------------------------------------------------- dense engine
def _dense_plan(env):
    """the kernels a dense-engine child's searches go through (switch_matrix.dense_sweep): first searches have no bound from a previous
    one, later ones may be screened"""
    return {M.dense_sweep(prev, scr, env) for prev, scr in ((False, False), (True, False), (True, True))}


def test_dense_default_matches_the_oracle(defaults, oracle):
    from kinectpy_amd.utils import synth
    z = defaults("dense")
    assert int(z["engine"][0]) == 1 and int(z["engine_before"][0]) == 1      # chosen by KPX_NN_ENGINE=dense before nn_engine("dense") asked
    src, tgt, T = synth.icp_pair(M.DENSE_N)
    for tag, T0 in (("eye", np.eye(4)), ("T", T)):
        ri, rd, _ = oracle.nn(src, T0, tgt, grid=True)
        assert np.array_equal(z["nn_%s_idx" % tag], ri) and np.array_equal(z["nn_%s_d2" % tag], rd), tag
    for mode in ("p2p", "p2plane"):
        rT, rf, rr, rit = oracle.registration_icp(src, tgt, 100.0, None, mode, z["tn"] if mode == "p2plane" else None, M.DENSE_ITERS)
        assert z[mode + "_s"][2] == rit >= 6 and z[mode + "_s"][0] == rf and np.abs(z[mode + "_T"] - rT).max() < TOL_T, mode
    rT, rf, _, rit, _ = G.registration_generalized_icp(oracle, src, tgt, 100.0, z["gicp_cs"], z["gicp_ct"], None, M.DENSE_ITERS)
    assert z["gicp_s"][2] == rit and z["gicp_s"][0] == rf and np.abs(z["gicp_T"] - rT).max() < TOL_T
    csrc, csc, ctgt, ctc, _ = synth.coloured_pair(M.DENSE_N)
    rT, rf, _, rit = oracle.registration_colored_icp(csrc, csc, ctgt, ctc, z["coloured_tn"], 80.0, None, 0.968, M.DENSE_ITERS)
    assert z["coloured_s"][2] == rit and z["coloured_s"][0] == rf and np.abs(z["coloured_T"] - rT).max() < TOL_T
    screen, mfma, local = (int(v) for v in z["launches"])
    assert screen > 0 and mfma > 0 and local == 0                        # the all-pairs engine, screening from the third search on


@_params("dense")
def test_dense_engine_switches(defaults, tmp_path, setting):
    env = M.FAMILIES["dense"][setting]
    base, z = defaults("dense"), run_child("dense", setting, env, tmp_path)
    _same_keys(base, z, setting)
    assert int(z["engine"][0]) == 1
    exact = [key for key in base if key.startswith("nn_") or key in ("tn", "coloured_tn", "gicp_cs", "gicp_ct")]
    _bitwise(base, z, exact, setting)
    for reg in ("p2p", "p2plane", "gicp", "coloured"):
        assert z[reg + "_s"][2] == base[reg + "_s"][2] and z[reg + "_s"][0] == base[reg + "_s"][0] and z[reg + "_s"][3] == base[reg + "_s"][3], (setting, reg)
        assert np.abs(z[reg + "_T"] - base[reg + "_T"]).max() < TOL_T, (setting, reg)
    for reg in ("p2p", "p2plane", "gicp"):                              # the last search's correspondences, where both found one in reach
        ok = base[reg + "_d2"] < 100.0 ** 2
        assert np.array_equal(z[reg + "_d2"] < 100.0 ** 2, ok) and np.array_equal(z[reg + "_idx"][ok], base[reg + "_idx"][ok]), (setting, reg)
    # the forced form ran: the library's launch counts, and the kernels the dispatch rule gives
    screen, mfma, local = (int(v) for v in z["launches"])
    b_screen, b_mfma, _ = (int(v) for v in base["launches"])
    assert local == 0 and mfma > 0
    plan, plan0 = _dense_plan(env), _dense_plan({})
    if "KPX_NN_SCREEN" in env:
        assert screen == 0 and b_screen > 0 and mfma == b_mfma + b_screen and "screen" not in plan
    else:
        assert screen == b_screen and mfma == b_mfma
    assert plan0 == {"mfma", "screen"}
    want = {"NN_SCREEN=0": {"mfma"}}[setting]
    assert plan == want, (setting, plan)


# ---------------------------------------------------------------------------------------------------------------- frame step
def test_frame_default_matches_the_oracle(defaults, oracle):
    from kinectpy_amd.pipeline import PipelineParams
    from kinectpy_amd.utils import synth
    z = defaults("frame")
    xy, depth, rgb, inits, _ = synth.sensor_ring(4, 3)
    ref = [oracle.pipeline_step(xy, depth[f], rgb[f], inits, PipelineParams()) for f in range(3)]

    def same(prefix, f):
        rp, rc, rT, _ = ref[f]
        assert np.array_equal(z[prefix + "_p"], rp) and np.array_equal(z[prefix + "_c"], rc), prefix
        assert np.abs(z[prefix + "_T"] - np.stack(rT)).max() < TOL_T, prefix
    for f in range(3):
        same("step%d" % f, f)
        aux = ref[f][3]
        assert list(z["step%d_n" % f][:4]) == [len(x) for x in aux["downs"]] and list(z["step%d_n" % f][-3:]) == [it for it, _, _ in aux["icp"]]
        for r in range(2):
            same("shard_r%d_f%d" % (r, f), f)
    for i, f in enumerate(z["stream_seq"]):
        same("stream%d" % i, int(f))
        for r in range(2):
            same("shardstream_r%d_%d" % (r, i), int(f))


@_params("frame")
def test_frame_step_switches(defaults, tmp_path, setting):
    """fused clouds, colours, transforms and counts of every frame, on every path and rank, bit for bit."""
    env = M.FAMILIES["frame"][setting]
    if "KPX_ORDER_LOOKAHEAD" in env:                                    # the ends of what the stream accepts, and neither is the default
        assert int(env["KPX_ORDER_LOOKAHEAD"]) in (0, M.FRAME_SLOTS - 1) and int(env["KPX_ORDER_LOOKAHEAD"]) != 2
    base, z = defaults("frame"), run_child("frame", setting, env, tmp_path)
    _same_keys(base, z, setting)
    _bitwise(base, z, [key for key in base if key != "chains"], setting)
    if "KPX_ICP_CHAIN_ALONE" not in env:
        assert int(z["chains"][0]) == int(base["chains"][0]), setting


# ---------------------------------------------------------------------------------------------------------------- FPS
@pytest.fixture(scope="module")
def fps_reference():
    one, batch = M.fps_inputs()
    for p in list(one.values()) + batch:
        fps_ref.assert_squares_exact(p)
        assert M.FPS_K <= len(p) <= M.FPS_BATCH_BLOCK_MAX_N            # both forms are written for these sizes (kinectpx.h)
    return {n: fps_ref.fps(p, M.FPS_K, M.FPS_START) for n, p in one.items()}, [fps_ref.fps(p, M.FPS_K, M.FPS_START) for p in batch]


def _fps_vs_reference(z, ref, ctx):
    one, batch = ref
    for n, (rs, rc) in one.items():
        assert np.array_equal(z["fps_%d_sel" % n], rs) and np.array_equal(z["fps_%d_cover" % n].view(np.int64), rc.view(np.int64)), (ctx, n)
    for i, (rs, rc) in enumerate(batch):
        assert np.array_equal(z["fps_batch_sel"][i], rs) and np.array_equal(z["fps_batch_cover"][i].view(np.int64), rc.view(np.int64)), (ctx, i)


def test_fps_default_matches_the_reference(defaults, fps_reference):
    sizes = M.FPS_SIZES
    assert sizes[0] <= M.FPS_REG_N < sizes[1] <= M.FPS_LDS_N < sizes[2] <= M.FPS_BLOCK_MAX_N < sizes[3]
    _fps_vs_reference(defaults("fps"), fps_reference, "default")


@_params("fps")
def test_fps_form_switches(defaults, fps_reference, tmp_path, setting):
    env = M.FAMILIES["fps"][setting]
    mid = sum(M.FPS_BLOCK_MAX_N < n <= M.FPS_BATCH_BLOCK_MAX_N for n in M.FPS_BATCH_SIZES)
    forms = lambda e: [M.fps_form(n, 0, e) for n in M.FPS_SIZES] + [M.fps_form(n, mid, e) for n in M.FPS_BATCH_SIZES]
    assert set(forms({})) == {"block", "chain"} and set(forms(env)) == {env["KPX_FPS_FORM"]}      # the default takes both; the child one
    base, z = defaults("fps"), run_child("fps", setting, env, tmp_path)
    _same_keys(base, z, setting)
    _bitwise(base, z, list(base), setting)
    _fps_vs_reference(z, fps_reference, setting)
