"""The helpers of tests/compaction_ref.py, without a GPU: compact_form on both sides of every boundary of the forms table (DESIGN.md,
"Stream compaction: the forms"), the input builders' promises counted per tile with the oracle, and three planted faults that the
comparison of the GPU tests has to catch."""
import numpy as np
import pytest

from tests import compaction_ref as CR

T = CR.TILE


# ------------------------------------------------------------------------------------------------ compact_form
def test_constants_restate_the_library():
    """the restated constants against the sources they restate"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kinectpy_amd", "csrc")
    common, scans, extract = (open(os.path.join(src, f)).read() for f in ("kpx_compact.h", "kpx_compact.hip", "kpx_extract.hip"))
    num = lambda pat, text: int(re.search(pat, text).group(1))
    assert num(r"kCompactThreads = (\d+);", common) * num(r"kCompactItems = (\d+);", common) == CR.TILE
    assert num(r"kOnePassTiles = (\d+);", common) == CR.ONE_PASS_TILES
    m = re.search(r"compact_scan_threads\(int64_t tiles\) \{ return tiles > (\d+) \? (\d+) : (\d+); \}", common)
    assert [int(g) for g in m.groups()] == [CR.SCAN_WIDE_ABOVE, 1024, 256]
    assert re.search(r"b0 \+= (\d+) \* \(int32_t\)blockDim\.x", scans).group(1) == str(CR.SCAN_ITEMS)
    m = re.search(r"frame_major = !small && batch_onepass && frames >= (\d+) && frames <= (\d+) && tiles <= (\d+);", extract)
    assert [int(g) for g in m.groups()] == [CR.FRAME_MAJOR_MIN, CR.FRAME_MAJOR_MAX, CR.FRAME_MAJOR_MAX_TILES]


def test_scan_shapes():
    assert CR.scan_shape(1) == (256, False) and CR.scan_shape(2048) == (256, False)          # 256 threads never carry: 8 x 256 = 2048
    assert CR.scan_shape(2049) == (1024, False) and CR.scan_shape(8192) == (1024, False)
    assert CR.scan_shape(8193) == (1024, True)
    assert CR.tiles_of(0) == 1 and CR.tiles_of(1) == 1 and CR.tiles_of(T) == 1 and CR.tiles_of(T + 1) == 2
    assert CR.tiles_of(8192 * T) == 8192 and CR.tiles_of(8192 * T + 1) == 8193


def test_form_generic_boundaries():
    f = lambda n, frames=1, kind="generic": CR.compact_form(n, frames, False, kind=kind)
    assert f(2048 * T) == (CR.GENERIC_ONEPASS, None)
    assert f(2048 * T + 1) == (CR.GENERIC_THREE, (1024, False))
    assert f(8192 * T) == (CR.GENERIC_THREE, (1024, False)) and f(8192 * T + 1) == (CR.GENERIC_THREE, (1024, True))
    # frames: the limit is on tiles x frames; the scan's shape on the tiles of one frame
    assert f(256 * T, 8, "extract") == (CR.GENERIC_ONEPASS, None)
    assert f(256 * T + 1, 8, "extract") == (CR.GENERIC_THREE, (256, False))
    assert f(293 * T - 2047, 7, "extract") == (CR.GENERIC_THREE, (256, False))
    assert f(293 * T - 2047, 6, "extract") == (CR.GENERIC_ONEPASS, None)
    assert f(368639, 11, "extract") == (CR.GENERIC_ONEPASS, None) and f(368639, 12, "extract") == (CR.GENERIC_THREE, (256, False))


def test_form_px8_boundaries():
    f = lambda n, frames, **kw: CR.compact_form(n, frames, True, **kw)
    n = 293 * T - 2040
    assert CR.tiles_of(n) == 293 and n % 8 == 0
    assert f(n, 6) == (CR.PX8_TILE_MAJOR, None)                         # 1758 tiles
    assert f(n, 7) == (CR.PX8_THREE, (256, False))                     # 2051 tiles, frames 7 | 8
    assert f(n, 8) == (CR.PX8_FRAME_MAJOR, None)
    assert f(256 * T, 8) == (CR.PX8_TILE_MAJOR, None)                  # tiles x frames 2048 | 2049
    assert f(256 * T + 8, 8) == (CR.PX8_FRAME_MAJOR, None)
    assert f(2048 * T, 1) == (CR.PX8_TILE_MAJOR, None)
    assert f(2049 * T - 2040, 1) == (CR.PX8_THREE, (1024, False))
    assert f(8193 * T - 2040, 1) == (CR.PX8_THREE, (1024, True))
    assert f(8, 65535) == (CR.PX8_FRAME_MAJOR, None) and f(8, 65536) == (CR.PX8_THREE, (256, False))
    # the tiles are the frame-major grid's y dimension
    assert f(65535 * T, 8) == (CR.PX8_FRAME_MAJOR, None) and f(65536 * T, 8) == (CR.PX8_THREE, (1024, True))
    # the switches: KPX_ONEPASS forces either side at any size, KPX_ONEPASS_BATCH=0 sends a batch above the limit to three launches
    assert f(n, 9, onepass=0) == (CR.PX8_FRAME_MAJOR, None) and f(n, 3, onepass=0) == (CR.PX8_THREE, (256, False))
    assert f(n, 9, onepass=1) == (CR.PX8_TILE_MAJOR, None)
    assert f(257 * T, 8, onepass_batch=False) == (CR.PX8_THREE, (256, False)) and f(257 * T, 8) == (CR.PX8_FRAME_MAJOR, None)
    assert f(n, 6, onepass_batch=False) == (CR.PX8_TILE_MAJOR, None)


def test_form_vector_condition():
    assert CR.extract_is_vec(8) and CR.extract_is_vec(8, 0, 0) and CR.extract_is_vec(8, 16, 8)
    assert not CR.extract_is_vec(9) and not CR.extract_is_vec(8, 2) and not CR.extract_is_vec(8, 0, 1)
    assert CR.extract_is_vec(8, 0, None)


def test_form_points_boundaries():
    f = lambda n, lists=1, **kw: CR.compact_form(n, 1, False, lists=lists, kind="points", **kw)
    assert f(2048 * T) == (CR.POINTS_ONEPASS, None) and f(2048 * T + 1) == (CR.POINTS_FLAGS, (1024, False))
    assert f(8192 * T) == (CR.POINTS_FLAGS, (1024, False)) and f(8192 * T + 1) == (CR.POINTS_FLAGS, (1024, True))
    assert f(1, 2) == (CR.POINTS_FLAGS, (256, False)) and f(2048 * T, 2) == (CR.POINTS_FLAGS, (256, False))     # two lists: always
    assert f(2048 * T + 1, 2) == (CR.POINTS_FLAGS, (1024, False)) and f(8192 * T + 1, 2) == (CR.POINTS_FLAGS, (1024, True))
    assert f(300 * T, onepass=0) == (CR.POINTS_FLAGS, (256, False)) and f(2049 * T, onepass=1) == (CR.POINTS_ONEPASS, None)
    assert f(300 * T, 2, onepass=1) == (CR.POINTS_FLAGS, (256, False))


# ------------------------------------------------------------------------------------------------ builders
@pytest.mark.parametrize("rag", [1, 8, 2047, 0])
def test_extract_batch_keeps_its_promises(oracle, rag):
    tiles = 24
    n = (tiles - 1) * T + rag if rag else tiles * T
    b = CR.extract_batch(n, 6, seed=rag)
    assert b["kinds"] == ["lead", "empty", "late", "full", "lead", "late"]
    assert b["depth"].shape == (6, n) and b["xy"].shape == (n, 2) and b["rgb"].shape == (6, n, 3)
    nan_tiles = np.unique(np.flatnonzero(b["nan_px"]) // T)
    assert list(nan_tiles) == [8, tiles // 2 + 1] and np.isnan(b["xy"]).any(1).sum() == b["nan_px"].sum() == 74
    xyz = CR.xyz_images(b, oracle.unproject_u16)
    last = n - (tiles - 1) * T                                           # items of the ragged tile
    per_tile = []
    for f in range(6):
        d2c = CR.tile_counts(oracle.rgbd_compact(oracle.unproject_u16(b["depth"][f], b["xy"]))[2], n)
        img = CR.tile_counts(oracle.rgbd_compact(xyz[f])[2], n)
        if b["kinds"][f] != "full":
            assert np.array_equal(d2c, img)
        per_tile.append((d2c, img))
    c = per_tile[0][0]                                                   # "lead": three empty tiles first, then a full one; the tail keeps items
    assert list(c[:4]) == [0, 0, 0, T] and c[tiles // 2] == T and 0 < c[-1] < max(last, 2)
    assert oracle.rgbd_compact(xyz[0])[2][-1] == n - 1                   # the very last item is kept
    assert per_tile[1][0].sum() == 0 and per_tile[0][0].sum() > 0 and per_tile[2][0].sum() > 0       # an empty frame between non-empty ones
    c = per_tile[2][0]                                                   # "late": items in tile 1, an empty run inside and one with the last tile
    assert 0 < c[1] < T and list(c[4:8]) == [0, 0, 0, T] and list(c[-4:]) == [T, 0, 0, 0]
    full_d2c, full_img = per_tile[3]
    assert full_img.sum() == n and full_d2c.sum() == n - 74              # the full frame: every pixel (XYZ entry), every pixel with a table entry
    assert full_d2c[3] == T and full_d2c[8] == T - 37
    assert not np.array_equal(per_tile[0][0], per_tile[4][0])            # frames of one kind differ
    zero = (b["rgb"] == 0).all(2).mean(1)
    assert (zero > 0.04).all() and (zero < 0.65).all()


@pytest.mark.parametrize("rag", [1, 8, 2047])
def test_clustered_cloud_keeps_its_promises(rag):
    tiles = 40
    n = (tiles - 1) * T + rag
    p, neg = CR.clustered_cloud(n, seed=rag)
    assert p.dtype == np.float32 and p.shape == (n, 3) and np.array_equal(p, np.round(p))
    assert np.abs(p[:, [0, 2]]).max() <= 100 and np.abs(p[:, 1]).min() >= 100 and np.abs(p[:, 1]).max() <= 1000
    keep = CR.halfspace_ref(p, CR.HALF_PLANE)
    assert np.array_equal(keep, np.flatnonzero(neg)) and np.array_equal(keep, np.flatnonzero(p[:, 1] < 0))
    c = CR.tile_counts(keep, n)
    assert list(c[:4]) == [0, 0, 0, T] and list(c[-4:]) == [T, 0, 0, 0] and c[tiles // 2] == T
    assert ((c > 0) & (c < T)).sum() > tiles // 2 and 0.3 < len(keep) / n < 0.7
    assert len(CR.halfspace_ref(p, CR.NONE_PLANE)) == 0 and len(CR.halfspace_ref(p, CR.ALL_PLANE)) == n
    lo, up = CR.slab_ref(p, float(p[:, 1].max()))                        # cut = 0: the lower list is y >= 0
    assert np.array_equal(up, keep) and len(lo) + len(up) == n and np.array_equal(np.sort(np.concatenate([lo, up])), np.arange(n))
    lo, up = CR.slab_ref(p, -1.0)
    assert len(lo) == 0 and len(up) == n
    lo, up = CR.slab_ref(p, 1e9)
    assert len(lo) == n and len(up) == 0
    assert np.array_equal(CR.mask_select_ref(p, keep), p[neg]) and np.array_equal(CR.mask_select_ref(p, keep[::-1], invert=True), p[~neg])


# ------------------------------------------------------------------------------------------------ planted faults
def _scatter(keeps, n, offsets=None, shift_tile=None, drop=None):
    """a model of the compaction's output stage: per frame the kept indices of each tile written at the tile's offset into a padded
    (F, n) buffer that starts as -1.  offsets: per frame the tiles' exclusive offsets (default: the right ones); shift_tile = (f, t): that
    tile writes one slot late; drop = (f, t): that tile loses its first kept item (the later items and tiles close the gap)."""
    F, tiles = len(keeps), CR.tiles_of(n)
    out = np.full((F, n + 1), -1, np.int32)
    cnt = np.zeros(F, np.int32)
    for f, k in enumerate(keeps):
        k = np.asarray(k)
        if drop is not None and drop[0] == f:
            i = np.flatnonzero(k // T == drop[1])[0]
            k = np.delete(k, i)
        per = np.bincount(k // T, minlength=tiles)
        right = np.concatenate([[0], np.cumsum(per)[:-1]])
        off = right if offsets is None else offsets[f]
        for t in range(tiles):
            mine = k[right[t]:right[t] + per[t]]
            o = off[t] + (1 if shift_tile == (f, t) else 0)
            out[f, o:o + len(mine)] = mine
        cnt[f] = len(k)
    return out[:, :n], cnt


def test_planted_faults_are_caught(oracle):
    tiles = 24
    n = (tiles - 1) * T + 8
    b = CR.extract_batch(n, 5, seed=5)
    xyz = CR.xyz_images(b, oracle.unproject_u16)
    want = [oracle.rgbd_compact(xyz[f]) for f in range(5)]               # (points, None, idx)
    keeps = [w[2] for w in want]
    pts_of = lambda idx_buf: np.stack([xyz[f][np.maximum(idx_buf[f], 0)].astype(np.float32) for f in range(5)])

    def check(**fault):
        idx, cnt = _scatter(keeps, n, **fault)
        CR.compare_padded(pts_of(idx), None, idx, cnt, want, tag=tuple(fault))
        CR.compare_frames([(pts_of(idx)[f, :k], None, idx[f, :k]) for f, k in enumerate(cnt)], want, tag=tuple(fault))

    check()                                                              # the model itself is right
    assert CR.tile_counts(keeps[2], n)[1] > 1
    with pytest.raises(AssertionError, match="count"):                   # one kept item dropped in tile 1 of frame 2
        check(drop=(2, 1))
    # ... and with the device count left as it was (the comparison may not lean on the count alone): the rows differ from the drop on
    idx, cnt = _scatter(keeps, n, drop=(2, 1))
    with pytest.raises(AssertionError, match="'frame', 2, 'array', 0, 'first differing row', %d," % np.flatnonzero(keeps[2] // T == 1)[0]):
        CR.compare_padded(pts_of(idx), None, idx, cnt + np.int32([0, 0, 1, 0, 0]), want)
    with pytest.raises(AssertionError, match="'frame', 0, 'array', 0, 'first differing row'"):       # one tile's output one slot late
        check(shift_tile=(0, tiles // 2))
    with pytest.raises(AssertionError, match="'frame', 3"):
        check(shift_tile=(3, 5))
    per = [np.bincount(k // T, minlength=tiles) for k in keeps]
    right = [np.concatenate([[0], np.cumsum(p)[:-1]]) for p in per]
    for f in range(4):                                                   # frame f's offsets applied to frame f + 1
        wrong = list(right)
        wrong[f + 1] = right[f]
        if b["kinds"][f + 1] == "empty":                                 # (an empty frame writes nothing wherever its offsets point)
            check(offsets=wrong)
            continue
        with pytest.raises(AssertionError, match="'frame', %d" % (f + 1)):
            check(offsets=wrong)
    # the index arrays alone (no points) and the points alone catch the same faults
    idx, cnt = _scatter(keeps, n, shift_tile=(0, tiles // 2))
    with pytest.raises(AssertionError):
        CR.compare_padded(pts_of(idx), None, None, cnt, want)
    with pytest.raises(AssertionError):
        CR.compare_frames([(None, None, idx[f, :k]) for f, k in enumerate(cnt)], want)
