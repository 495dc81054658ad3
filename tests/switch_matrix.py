"""The KPX_* form switches that tests/test_switches_gpu.py flips, one fresh child process per setting, and what each one selects.

INTEGRATION.md promises that the switches never change results.  FAMILIES lists, per family of operators, the settings whose child
is compared with the family's default child; FLIPPED_ELSEWHERE the names an existing test already flips; EXEMPT the names that select
no kernel form.  tests/test_switches_cpu.py holds the three lists against the names the sources read.

The functions below restate the library's dispatch conditions (kpx_knn.hip kpx_sor / grid_build, kpx_container.hip bbox_f32, kpx_icp.hip
nn_search_launch, kpx_fps.hip fps_use_block); the GPU test asserts from them that each input sits on the side where its switch
matters.  They must be moved with the library's.  The inputs are built here, from NumPy alone, so that the children, the parent's
oracle runs and the CPU precondition see the same arrays."""
import os
import re

import numpy as np

from kinectpy_amd.utils import synth

_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kinectpx.h")).read()
_define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, _HEADER).group(1))
FPS_BLOCK_MAX_N, FPS_BATCH_BLOCK_MAX_N, FPS_BATCH_MIN_CLOUDS = _define("KPX_FPS_BLOCK_MAX_N"), _define("KPX_FPS_BATCH_BLOCK_MAX_N"), _define("KPX_FPS_BATCH_MIN_CLOUDS")
FPS_REG_N, FPS_LDS_N = _define("KPX_FPS_REG_N"), _define("KPX_FPS_LDS_N")
GRID_SORT_MIN = 65536                     # kpx_knn.hip grid_build: the radix-sort build above 65536 points, the counting build up to there
BBOX_SMALL_MAX = 65536                    # kpx_container.hip bbox_f32: one block up to 65536 points, partial boxes (vector / scalar loads) above
VOXEL_READBACK_MIN = 128 * 1024           # kpx_voxel.hip voxel_batch_impl: the key width is read back above 131072 points
ICP_CHAIN_BLOCKS = 512                    # the one-launch ICP chain's budget on the MI355X: (blocks per CU - 1) x CUs


def _settings(*specs):
    """"A=1+B=2" -> {"A=1+B=2": {"KPX_A": "1", "KPX_B": "2"}}"""
    return {s: {"KPX_" + kv.split("=")[0]: kv.split("=")[1] for kv in s.split("+")} for s in specs}


# Not here: KPX_CURVE=z, KPX_VOXEL_CURVE=z and KPX_FRAME_ZORDER=0.  Their children gave the same clouds, counts, iterations and fitness
# but other last bits in the culled ICP's transforms (up to 9.7e-12, 6.8e-14 and 4.5e-13 on an MI355X) and rmse (3.4e-13): they reorder
# the rows, and the ICP's sums are a tree per 16-row tile.  No default path reached the forms, all three had measured slower, and sums
# free of the row order are no small change: the forms and their switches were removed from the library.
# Nor the wave-per-16-queries pass-0 forms of kpx_sor and their switches KPX_SOR_BLOCK, KPX_SOR_BLOCK_MINK and KPX_SOR_CELL_SMALL: removed
# as superseded by sor_block_kernel.
# Nor the all-pairs engine's chunked fp64 sweep and caller-order operands and their switches KPX_NN_FAST and KPX_NN_DENSE_SORT: removed
# as superseded by the per-trip sweep over curve-ordered operands (profiles/r04/nn_dense_sorted.txt).
# Nor the grouped ICP driver's update placements 0 and 1 (next sweep's prologue, own kernel) and the 16- and 32-row widths of
# icp_rows_kernel, with their switches KPX_ICP_SPLIT and KPX_ICP_ROWS_R: removed.  No default path had reached them since round 2, the
# per-registration drivers keep both placements (KPX_ICP_BATCH_LAUNCH=0, with KPX_ICP_FUSE=0), and neither narrower width measured
# ahead of 64 (profiles/r06/exp_env_KPX_ICP_ROWS_R.txt).
FAMILIES = {
    # RADIX=0: the grid build above GRID_SORT_MIN points sorts with the vendor sort (kpx_sort.h reads the switch for every site)
    "grid": _settings("GRID_SCAN=0", "GRID_SORT=1", "SOR_CELL=0", "SOR_CELL=1", "SOR_OCC=0.2", "SOR_OCC=1.0", "BBOX_VEC=0", "RADIX=0"),
    "voxel": _settings("RADIX=0", "VOXEL_SINGLE=0"),
    # the launch-per-iteration chains of icp_rows_kernel: the rows form forced and the one-launch chain off
    "icp": _settings("ICP_FUSE=0", "ICP_BATCH_LAUNCH=0", "ICP_WINDOW=1", "ICP_WINDOW=64", "ICP_ROWS=2+ICP_CHAIN=0"),
    # the grouped driver's update in the sweep's last block (one-launch chains by default) against the per-registration drivers (update
    # in the next sweep's prologue; behind the kernel boundary) and against its own launch-per-iteration forms, at the edge sizes
    "icp_edges": _settings("ICP_BATCH_LAUNCH=0", "ICP_BATCH_LAUNCH=0+ICP_FUSE=0", "ICP_CHAIN=0", "ICP_ROWS=0+ICP_CHAIN=0", "ICP_ROWS=2+ICP_CHAIN=0"),
    "dense": _settings("NN_SCREEN=0"),
    # KPX_ICP_CHAIN_ALONE=0 admits one-launch chains with frames in flight (the streams below); KPX_ORDER_LOOKAHEAD: any value >= 0 is accepted and cut to slots - 1; FRAME_SLOTS = 4 slots, so 0 and 3 are its ends (default 2)
    "frame": _settings("FRAME_SPECULATE=0", "FRAME_SPIN=0", "SHARD_NORMALS=1", "SHARD_FIXED_CAP=1",
                       "ORDER_LOOKAHEAD=0", "ORDER_LOOKAHEAD=3", "ICP_CHAIN_ALONE=0"),
    "fps": _settings("FPS_FORM=block", "FPS_FORM=chain"),
}
# every culled-ICP child: this suite's own process may hold the device's chain lock (it is idle meanwhile), as
# test_icp_update_placements_and_light_skip_are_bit_identical sets it
# the dense children: the environment chooses the engine at the library's first use, and ops.nn_engine("dense") then reports it
FAMILY_ENV = {"icp": {"KPX_ICP_CHAIN_LOCK": "0"}, "icp_edges": {"KPX_ICP_CHAIN_LOCK": "0"}, "frame": {"KPX_ICP_CHAIN_LOCK": "0"}, "dense": {"KPX_NN_ENGINE": "dense"}}
FRAME_SLOTS = 4

FLIPPED_ELSEWHERE = {
    "KPX_ONEPASS": "tests.test_compaction_gpu::test_forced_forms_agree_and_match_the_oracle",
    "KPX_ONEPASS_BATCH": "tests.test_compaction_gpu::test_forced_forms_agree_and_match_the_oracle",
    "KPX_MEDIAN_FRAME": "tests.test_parity_gpu::test_median_exact",
    "KPX_PLANE_MFMA": "tests.test_parity_gpu::test_segment_plane_ties_thresholds_and_sequential_path",
    "KPX_ICP_LIGHT_SKIP": "tests.test_parity_gpu::test_icp_update_placements_and_light_skip_are_bit_identical",
    "KPX_ICP_CERT": "tests.test_parity_gpu::test_icp_update_placements_and_light_skip_are_bit_identical",
    "KPX_ICP_CERT_CHECK": "tests.test_parity_gpu::test_icp_certificates_never_contradict_the_search",
    "KPX_ICP_CHAIN": "tests.test_parity_gpu::test_icp_update_placements_and_light_skip_are_bit_identical",
    "KPX_ICP_CHAIN_BUDGET": "tests.test_parity_gpu::test_icp_chain_that_cannot_be_resident_fails_loudly",
    "KPX_ICP_CHAIN_LOCK": "tests.test_parity_gpu::test_icp_update_placements_and_light_skip_are_bit_identical",
    "KPX_ICP_ROWS": "tests.test_parity_gpu::test_icp_update_placements_and_light_skip_are_bit_identical",
    "KPX_ICP_ROWS_SHARE": "tests.test_parity_gpu::test_icp_update_placements_and_light_skip_are_bit_identical",
}
EXEMPT = {
    "KPX_LIBRARY": "path of the shared library to load: no kernel form",
    "KPX_ICP_STALL_SECONDS": "watchdog period of the ICP launch windows: no kernel form",
    "KPX_ICP_CHAIN_WAIT_SECONDS": "bound of the waits inside a one-launch chain: no kernel form",
    "KPX_ICP_CHAIN_STAMPS": "development aid, the chain's clock: no kernel form",
    "KPX_ICP_CHAIN_DUMP": "development aid, the chain's records on stderr: no kernel form",
    "KPX_FRAME_EXTRA_DISPATCHES": "measurement hook, empty kernels per frame: no kernel form",
    "KPX_CERT_CALM": "certificate skin policy, a number: no kernel form",
    "KPX_CERT_FACTOR": "certificate skin policy, a number: no kernel form",
    "KPX_CERT_SKIN_MIN": "certificate skin policy, a number: no kernel form",
    "KPX_CERT_SKIN_MAX": "certificate skin policy, a number: no kernel form",
    "KPX_DIST_BACKEND": "torch.distributed backend of the Python ranks: no kernel form",
}


def matrix_names():
    return {name for fam in FAMILIES.values() for env in fam.values() for name in env} | {n for env in FAMILY_ENV.values() for n in env}


# ---------------------------------------------------------------------------------------------------------------- grid, SOR, bounds
SOR_KS = (8, 24, 25, 32, 33, 64, 65, 128, 129, 300)
SOR_MARGIN = 1e-9                         # no point's mean distance within this (relative) of the keep threshold: see sor_margin()
NORMALS_ARGS = (70.0, 30)
RADIUS_ARGS = (10, 40.0)                  # nb_points, radius
DBSCAN_ARGS = (30.0, 10)                  # eps, min_points


def sor_ratio(k):
    return 1.0 if k % 2 else 2.0          # (test_sor_k_boundaries' rule)


def halo_cloud():
    """test_boundaries_gpu.halo_cloud's recipe: a 30k sample of the rendered frame (the block kernel's dense cells) plus a sparse
    halo of 400 points around it (queries whose k-th neighbour lies many cells away: the fall-back passes)"""
    rng = np.random.default_rng(41)
    base = synth.frame_cloud()
    p = base[rng.choice(len(base), 30000, replace=False)]
    lo, hi = p.min(0), p.max(0)
    halo = rng.uniform(lo - 500, hi + 500, size=(400, 3)).astype(np.float32)
    q = np.concatenate([p, halo])
    return np.ascontiguousarray(q[rng.permutation(len(q))])


def grid_inputs():
    """halo: below the 65536 build switch; c70k: above it; c66k: above bbox_f32's one-block form, passed aligned and as a view one row in"""
    c = synth.filter_cloud(70_000, seed=17)
    return {"halo": halo_cloud(), "c70k": c, "c66k": np.ascontiguousarray(synth.filter_cloud(66_001, seed=19))}


def sor_cases():
    """(input, k, ratio): every k on the frame-density cloud, the ends of the cascade on the cloud above the build switch"""
    return [("halo", k, sor_ratio(k)) for k in SOR_KS] + [("c70k", k, sor_ratio(k)) for k in (24, 33, 129)]


def sor_margin(avg, thr):
    """smallest relative distance of a point's mean neighbour distance from the keep threshold (from oracle values alone): with a mean
    within rounding of the threshold, two correct forms whose sums differ in the last bit could keep different points"""
    return float(np.min(np.abs(avg - thr)) / abs(thr))


def sor_pass0(k, env):
    """kpx_sor's pass 0 at k under `env`: None (every query starts at the wave-per-query passes) or "block<S>" """
    cell = env.get("KPX_SOR_CELL")
    mode = 1 if cell is None else (0 if cell[0] == "0" else 2)
    if not ((mode == 2 or (mode == 1 and k > 32)) and k <= 1024):
        return None
    return "block<%d>" % (4 if k <= 32 else 8 if k <= 64 else 16 if k <= 128 else 32)


def grid_occupancy(k, env):
    occ = float(env.get("KPX_SOR_OCC", "0")) or 0.4
    return min(240.0, max(6.0, occ * k))


def grid_build_form(n, env):
    return "sort" if env.get("KPX_GRID_SORT", "")[:1] == "1" or n > GRID_SORT_MIN else "count"


def bbox_form(n, aligned, env):
    if n <= BBOX_SMALL_MAX:
        return "small"
    return "vec" if aligned and env.get("KPX_BBOX_VEC", "")[:1] != "0" else "scalar"


# ---------------------------------------------------------------------------------------------------------------- voxel
VOXEL_SIZE = 10.0


def voxel_inputs():
    """name -> list of clouds; one cloud: kpx_voxel_downsample, several: kpx_voxel_downsample_batch; "fused": two clouds and their
    transforms through kpx_fuse_voxel_downsample.  Each with colours, with normals (single clouds: the only form that takes them)
    and with neither."""
    big = synth.filter_cloud(140_000, seed=7)
    rng = np.random.default_rng(23)
    ragged = [np.ascontiguousarray(big[:60_001]), np.ascontiguousarray(big[60_001:110_000] + np.float32(11.0)), np.ascontiguousarray(big[110_000:145_000] - np.float32(7.0))]
    pair = [np.ascontiguousarray(big[:9_000]), np.ascontiguousarray(big[9_000:20_001])]
    return {"v140k": [big], "v20k": [np.ascontiguousarray(big[:20_000])], "ragged": ragged, "fused": pair}, rng


def voxel_attrs(clouds, rng):
    cols = [rng.random(c.shape).astype(np.float32) for c in clouds]
    nrms = [rng.standard_normal(c.shape).astype(np.float32) for c in clouds]
    return cols, nrms


def fused_transforms():
    T = synth.t_star()
    return [np.eye(4), T]


# ---------------------------------------------------------------------------------------------------------------- culled ICP, edge sizes
ICP_EDGES_N = 4000                        # synth.icp_pair(4000): the target, and the cloud the sources are cut from
ICP_EDGES_NORMALS = (70.0, 40)            # the target's normals (test_icp_chain_edge_sizes_equal_launch_per_iteration's)
ICP_EDGES_MAX_DIST = 100.0
ICP_GROUP_MAX = 7                         # kpx_icp.hip kpx_icp_batch: the batch sort takes the target and seven sources; from eight on the
                                          # clouds stay in caller order and the per-registration driver (drive_windowed) serves


def icp_edges_cases(src):
    """(sources, max_iteration): where a ticket count or a block range can be off by one -- a single row; partial waves, a full block,
    one row and one block beyond it; all the grouped driver takes and one more; no iteration and one"""
    ramp = lambda count: [src[i * 300:(i + 1) * 300 + 7 * i] for i in range(count)]
    return [([src[:1]], 5), ([src[:17], src[:64], src[:65], src[:129]], 5), (ramp(ICP_GROUP_MAX), 6), (ramp(ICP_GROUP_MAX + 1), 6),
            ([src[:2000]], 0), ([src[:2000]], 1)]


# ---------------------------------------------------------------------------------------------------------------- dense engine
DENSE_N = 6000
DENSE_ITERS = 10


def dense_sweep(have_prev, screened, env):
    """nn_search_launch, all-pairs engine: which kernel serves a search -> "screen" | "mfma" """
    return "screen" if have_prev and screened and env.get("KPX_NN_SCREEN", "")[:1] != "0" else "mfma"


# ---------------------------------------------------------------------------------------------------------------- FPS
FPS_K, FPS_START = 64, 5
FPS_SIZES = (700, 15_000, 22_000, 30_000)          # registers / LDS / global running distances of the block form; above its default ceiling
FPS_BATCH_SIZES = (5_000, 26_000, 13_001)


def fps_inputs():
    """integer-millimetre clouds (tests/fps_ref.py: there the library's distance equals Open3D's sum bit for bit)"""
    base = synth.frame_cloud()
    rng = np.random.default_rng(29)
    one = {n: np.ascontiguousarray(base[rng.choice(len(base), n, replace=False)]) for n in FPS_SIZES}
    batch = [np.ascontiguousarray(base[rng.choice(len(base), n, replace=False)]) for n in FPS_BATCH_SIZES]
    return one, batch


def fps_form(n, mid, env):
    f = env.get("KPX_FPS_FORM")
    if f in ("block", "chain"):
        return f
    return "block" if n <= FPS_BLOCK_MAX_N or (mid >= FPS_BATCH_MIN_CLOUDS and n <= FPS_BATCH_BLOCK_MAX_N) else "chain"
