"""farthest_point_sample / farthest_point_down_sample on the MI355X against the restated Open3D loop (tests/fps_ref.py), bit for bit.
Every input is integer millimetres (tests/fps_ref.py: squares_exact), where the library's AC3 distance equals Open3D's sum.
The form switches are read from include/kinectpx.h; each case asserts which side of them it sits on."""
import os
import re

import numpy as np
import pytest
import torch

from kinectpy_amd import ops
from kinectpy_amd.geometry import PointCloud
from kinectpy_amd.utils import synth
from tests import fps_ref as R

pytestmark = pytest.mark.gpu

_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kinectpx.h")).read()
_define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, _HEADER).group(1))
REG_N, LDS_N, BLOCK_MAX_N = _define("KPX_FPS_REG_N"), _define("KPX_FPS_LDS_N"), _define("KPX_FPS_BLOCK_MAX_N")
BATCH_BLOCK_MAX_N, BATCH_MIN_CLOUDS = _define("KPX_FPS_BATCH_BLOCK_MAX_N"), _define("KPX_FPS_BATCH_MIN_CLOUDS")


@pytest.fixture(scope="module")
def frame():
    return synth.frame_cloud()


def _subset(base, n, seed=0):
    rng = np.random.default_rng(seed)
    reps = -(-n // len(base))
    pool = np.concatenate([base + np.float32([0, 0, 5000 * r]) for r in range(reps)]) if reps > 1 else base
    return np.ascontiguousarray(pool[rng.choice(len(pool), n, replace=False)])


def _gpu(pts, k, start=0):
    sel, cover = ops.farthest_point_sample(np.ascontiguousarray(pts, dtype=np.float32), k, start, want_cover=True)
    return sel.cpu().numpy(), cover.cpu().numpy()


def _check(pts, k, start=0):
    R.assert_squares_exact(pts)
    sel, cover = _gpu(pts, k, start)
    rs, rc = R.fps(pts, k, start)
    assert np.array_equal(sel, rs), (len(pts), k, start, int(np.argmax(sel != rs)) if len(sel) == len(rs) else None)
    assert np.array_equal(cover.view(np.int64), rc.view(np.int64)), (len(pts), k, start)
    return sel, cover


def test_lattices_where_ties_dominate():
    g = np.stack(np.meshgrid(np.arange(24), np.arange(20), np.arange(16), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 10
    assert len(g) <= BLOCK_MAX_N
    rng = np.random.default_rng(2)
    for pts in (g, g[rng.permutation(len(g))]):
        n = len(pts)
        for start in (0, n // 2, n - 1):
            _check(pts, 300, start)
    rnd = rng.integers(0, 40, size=(3000, 3)).astype(np.float32)        # random lattice points, many duplicates
    _check(rnd, 1500, 11)


def test_frame_cloud_k4096_chain(frame):
    assert len(frame) > BLOCK_MAX_N
    sel, cover = _check(frame, 4096)
    assert np.all(np.diff(cover) <= 0)


def test_filter_cloud_subset():
    pts = np.round(synth.filter_cloud(200_000, seed=4)).astype(np.float32)      # integer millimetres
    assert len(pts) > BLOCK_MAX_N
    _check(pts, 400, 123)
    _check(pts[:BLOCK_MAX_N], 400, 0)


def test_duplicates_and_one_outlier_repeat_and_shrink():
    for n in (5000, BLOCK_MAX_N + 5000):
        pts = np.tile(np.float32([[12, -40, 1500]]), (n, 1))
        pts[n // 3] = (400, -40, 1500)
        sel, cover = _check(pts, 6, n - 1)
        assert sel.tolist() == [n - 1, n // 3] + [n // 3] * 4 and cover[1:].tolist() == [0.0] * 5
        pc = PointCloud()
        pc.points = pts
        assert len(pc.farthest_point_down_sample(6, n - 1).points) == 2


def test_k_edges():
    pts = _subset(synth.frame_cloud(), 700, seed=3)
    n = len(pts)
    for k in (1, n - 1, n):
        _check(pts, k, 5)
    sel, cover = ops.farthest_point_sample(pts, 0, 0, want_cover=True)
    assert sel.numel() == 0 and cover.numel() == 0
    pc = PointCloud()
    pc.points = pts
    assert len(pc.farthest_point_down_sample(0).points) == 0
    cp = pc.farthest_point_down_sample(n, start_index=n + 5)            # k == n: Open3D copies before checking start_index
    assert np.array_equal(np.asarray(cp.points), pts)


def test_every_form_switch(frame):
    for n in (REG_N, REG_N + 1, LDS_N, LDS_N + 1, BLOCK_MAX_N, BLOCK_MAX_N + 1, BATCH_BLOCK_MAX_N + 1):
        pts = _subset(frame, n, seed=n)
        _check(pts, 64, n // 7)


def test_more_than_4m_points(frame):
    n = 4 * 1024 * 1024 + 4321
    pts = _subset(frame, n, seed=9)
    _check(pts, 5, n - 2)


def test_batch_across_switches_equals_single_calls(frame):
    sizes = [1, 9, 2000, REG_N, REG_N + 1, LDS_N, LDS_N + 1, BLOCK_MAX_N, BLOCK_MAX_N + 1, 70000]
    clouds = [_subset(frame, n, seed=i) for i, n in enumerate(sizes)]
    for k, cl in ((1, clouds), (48, clouds[2:])):
        bs, bc = ops.farthest_point_sample_batch(cl, k, 0)
        bs, bc = bs.cpu().numpy(), bc.cpu().numpy()
        for i, c in enumerate(cl):
            s, cv = _gpu(c, k, 0)
            assert np.array_equal(bs[i], s) and np.array_equal(bc[i].view(np.int64), cv.view(np.int64)), (k, len(c))
            rs, rc = R.fps(c, k, 0)
            assert np.array_equal(s, rs) and np.array_equal(cv, rc), (k, len(c))
    # clouds between the two limits join the block launch only when the batch has BATCH_MIN_CLOUDS of them
    mid = [BLOCK_MAX_N + 1, 30000, 40000, BATCH_BLOCK_MAX_N][:BATCH_MIN_CLOUDS]
    for sizes in (mid + [BATCH_BLOCK_MAX_N + 1, 500], mid[1:] + [500]):
        cl = [_subset(frame, n, seed=n) for n in sizes]
        bs, bc = ops.farthest_point_sample_batch(cl, 40, 2)
        bs, bc = bs.cpu().numpy(), bc.cpu().numpy()
        for i, c in enumerate(cl):
            s, cv = _gpu(c, 40, 2)
            assert np.array_equal(bs[i], s) and np.array_equal(bc[i].view(np.int64), cv.view(np.int64)), (sizes, i)
        rs, rc = R.fps(cl[0], 40, 2)
        assert np.array_equal(bs[0], rs) and np.array_equal(bc[0], rc)
    many = [_subset(frame, 300 + i, seed=100 + i) for i in range(70)]     # more block-form clouds than one launch carries
    bs, bc = ops.farthest_point_sample_batch(many, 20, 3)
    bs, bc = bs.cpu().numpy(), bc.cpu().numpy()
    for i in (0, 1, 63, 64, 69):
        rs, rc = R.fps(many[i], 20, 3)
        assert np.array_equal(bs[i], rs) and np.array_equal(bc[i], rc), i
    bs, bc = ops.farthest_point_sample_batch([np.zeros((0, 3), np.float32), clouds[2]], 0, 0)
    assert tuple(bs.shape) == (2, 0) and tuple(bc.shape) == (2, 0)


def test_two_runs_are_bit_identical(frame):
    small = _subset(frame, 15000, seed=1)
    for pts, k in ((frame, 512), (small, 1024)):
        a, b = _gpu(pts, k, 17), _gpu(pts, k, 17)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def test_down_sample_carries_colours_and_normals(frame):
    from kinectpy_amd import o3d
    pts = _subset(frame, 5000, seed=6)
    rng = np.random.default_rng(6)
    pc = o3d.geometry.PointCloud()
    pc.points = o3d.utility.Vector3dVector(pts)
    pc.colors = o3d.utility.Vector3dVector(rng.random((len(pts), 3)).astype(np.float32))
    pc.normals = o3d.utility.Vector3dVector(rng.normal(size=(len(pts), 3)).astype(np.float32))
    down = pc.farthest_point_down_sample(800, 10)
    sel, _ = R.fps(pts, 800, 10)
    ref = pc.select_by_index(sel)
    keep = np.unique(sel)
    for attr in ("points", "colors", "normals"):
        got = np.asarray(getattr(down, attr))
        assert np.array_equal(got, np.asarray(getattr(ref, attr))) and len(got) == len(keep)
    assert np.array_equal(np.asarray(down.points), pts[keep].astype(np.float64))


def test_error_messages():
    pts = np.float32([[0, 0, 0], [1, 2, 3], [4, 5, 6]])
    pc = PointCloud()
    pc.points = pts
    with pytest.raises(RuntimeError, match=r"Illegal number of samples: 4, must <= point size: 3"):
        pc.farthest_point_down_sample(4)
    with pytest.raises(RuntimeError, match=r"Illegal start index: 3, must <= point size: 3"):
        pc.farthest_point_down_sample(2, start_index=3)
    with pytest.raises(RuntimeError, match=r"Illegal number of samples: 4, must <= point size: 3"):
        ops.farthest_point_sample(pts, 4)
    with pytest.raises(RuntimeError, match=r"Illegal start index: 3, must <= point size: 3"):
        ops.farthest_point_sample(pts, 2, 3)


def test_select_points_farthest_returns_exactly_k_rows(frame):
    from kinectpy_amd.utils.processing import select_points_farthest
    pts = np.tile(np.float32([[1, 2, 3]]), (50, 1))
    pts[7] = (30, 2, 3)
    pc = PointCloud()
    pc.points = pts
    out = select_points_farthest(pc, 10)
    assert out.shape == (10, 3) and out.dtype == np.float64
    assert np.array_equal(out, pts[[0, 7] + [7] * 8].astype(np.float64))
    pc.points = _subset(frame, 20000, seed=8)
    out = select_points_farthest(pc, 1024, 3)
    sel, _ = R.fps(np.asarray(pc.points), 1024, 3)
    assert out.shape == (1024, 3) and np.array_equal(out, np.asarray(pc.points)[sel])
