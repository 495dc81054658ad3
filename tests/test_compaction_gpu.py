"""GPU suite (-m gpu): the order-preserving stream compaction in every form of DESIGN.md's table ("Stream compaction: the forms"),
bit for bit against the C oracle (extract) and NumPy (point selections).

Each case first asserts, through tests/compaction_ref.compact_form, which form and which scan shape its own inputs select; the sizes are
the smallest that reach each form.  The inputs (compaction_ref.extract_batch, clustered_cloud) keep their items in whole tiles: runs of
empty tiles at either end, full tiles, a ragged last tile, an empty and a full frame, NaN table entries.  The last test runs every
caller of the compaction in child processes with KPX_ONEPASS / KPX_ONEPASS_BATCH forced either way."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import compaction_ref as CR

pytestmark = pytest.mark.gpu
T = CR.TILE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


def npy(t):
    return t.cpu().numpy() if t is not None else None


def _view(host, off):
    """a contiguous device view of `host` (flattened) that starts `off` elements after a 16-byte boundary"""
    flat = np.ascontiguousarray(host).reshape(-1)
    pad = np.zeros(flat.size + 16, flat.dtype)
    pad[off:off + flat.size] = flat
    t = torch.as_tensor(pad).cuda()[off:off + flat.size]
    assert t.data_ptr() % 16 == (off * flat.itemsize) % 16 and t.is_contiguous()
    return t


# ------------------------------------------------------------------------------------------------ extract
_REFS = {}


def _batch_with_refs(oracle, n, frames, seed):
    """the batch, its XYZ images and a reference per (entry, colour mask, depth gate), computed once per distinct frame and kept for
    the cases that share the batch (one batch at a time)"""
    key = (n, frames, seed)
    if key not in _REFS:
        _REFS.clear()
        b = CR.extract_batch(n, frames, seed)
        raw = np.stack([oracle.unproject_u16(d, b["xy"]) for d in b["depth"]])
        xyz = CR.xyz_images(b, oracle.unproject_u16)
        _REFS[key] = dict(b=b, raw=raw, xyz=xyz, ref={})
    e = _REFS[key]

    def ref(entry, cm, dg):
        if (entry, cm, dg) not in e["ref"]:
            img = e["raw"] if entry == "d2c" else e["xyz"]
            out = []
            for f in range(frames):
                same = entry == "xyz" and e["b"]["kinds"][f] != "full" and ("d2c", cm, dg) in e["ref"]
                out.append(e["ref"][("d2c", cm, dg)][f] if same else
                           oracle.rgbd_compact(img[f], e["b"]["rgb"][f], cm, dg, (oracle.median_z(img[f]) + CR.GATE_MM) if dg else 0.0))
            e["ref"][(entry, cm, dg)] = out
        return e["ref"][(entry, cm, dg)]
    return e["b"], e["xyz"], ref


N293 = 293 * T - 2040                  # 293 tiles, a multiple of 8, ragged tile of 8: 7 frames are 2051 tiles
N180 = 180 * T - 2040                  # Kinect-sized (576 x 640 is 180 tiles), ragged tile of 8
# id: n, frames, depth / XYZ offset (elements), rgb offset (bytes), form with colours, form without, scan shape, extras (the four flag
# combinations and sync=False: once per form)
EXTRACT_SHAPES = {
    "px8 three-launch, 256-thread scan": (N293, 7, 0, 0, CR.PX8_THREE, CR.PX8_THREE, (256, False), True),
    "generic three-launch, depth 2 bytes off, 7 frames": (N293, 7, 1, 0, CR.GENERIC_THREE, CR.GENERIC_THREE, (256, False), False),
    "generic three-launch, rgb 1 byte off, 7 frames": (N293, 7, 0, 1, CR.GENERIC_THREE, CR.PX8_THREE, (256, False), False),
    "px8 three-launch, 1024-thread scan": (2049 * T - 2040, 1, 0, 0, CR.PX8_THREE, CR.PX8_THREE, (1024, False), False),
    "px8 frames 7|8: frame-major": (N293, 8, 0, 0, CR.PX8_FRAME_MAJOR, CR.PX8_FRAME_MAJOR, None, True),
    "px8 2048 tiles: tile-major": (256 * T, 8, 0, 0, CR.PX8_TILE_MAJOR, CR.PX8_TILE_MAJOR, None, True),
    "px8 2049 tiles: frame-major": (256 * T + 8, 8, 0, 0, CR.PX8_FRAME_MAJOR, CR.PX8_FRAME_MAJOR, None, False),
    "generic three-launch, odd n, 7 frames": (293 * T - 2047, 7, 0, 0, CR.GENERIC_THREE, CR.GENERIC_THREE, (256, False), True),
    "generic three-launch, odd n, 12 Kinect frames": (180 * T - 1, 12, 0, 0, CR.GENERIC_THREE, CR.GENERIC_THREE, (256, False), False),
    "generic three-launch, depth 2 bytes off, 12 frames": (N180, 12, 1, 0, CR.GENERIC_THREE, CR.GENERIC_THREE, (256, False), False),
    "generic three-launch, rgb 1 byte off, 12 frames": (N180, 12, 0, 1, CR.GENERIC_THREE, CR.PX8_FRAME_MAJOR, (256, False), False),
    "generic one-pass, odd n, 3 frames": (150 * T + 1, 3, 0, 0, CR.GENERIC_ONEPASS, CR.GENERIC_ONEPASS, None, True),
}


@pytest.mark.parametrize("shape", list(EXTRACT_SHAPES))
def test_extract_forms_match_oracle(ops, oracle, shape):
    """depth -> cloud and the int16-XYZ compaction over the four <COL, IDX> instantiations (colours or none x index output or none); on
    one shape per form also the four flag combinations and the padded sync=False outputs with their device counts"""
    n, F, d_off, r_off, form_rgb, form_plain, scan, extras = EXTRACT_SHAPES[shape]
    assert n % T in (0, 1, 8, 2047)
    for use_rgb, want_form in ((True, form_rgb), (False, form_plain)):         # which side of each threshold this case sits on
        vec = CR.extract_is_vec(n, 2 * d_off, r_off if use_rgb else None)
        form, sc = CR.compact_form(n, F, vec)
        assert form == want_form and (sc is None or sc == scan), (shape, use_rgb, form, sc)
    b, xyz, ref = _batch_with_refs(oracle, n, F, seed=F * 1000 + n % 1000)
    depth, xyz_d, rgb = _view(b["depth"], d_off), _view(xyz, d_off), _view(b["rgb"], r_off)
    xy = torch.as_tensor(b["xy"]).cuda()
    assert depth.data_ptr() % 16 == 2 * d_off and xyz_d.data_ptr() % 16 == 2 * d_off and rgb.data_ptr() % 8 == r_off and xy.data_ptr() % 16 == 0

    def run(entry, use_rgb, cm, dg, wi, sync=True):
        if entry == "d2c":
            return ops.depth_to_cloud(depth, xy, rgb if use_rgb else None, F, cm, dg, want_idx=wi, sync=sync)
        return ops.rgbd_compact(xyz_d, rgb if use_rgb else None, F, cm, dg, want_idx=wi, sync=sync)

    for entry in ("d2c", "xyz"):
        want = ref(entry, False, False)
        kept = [len(w[0]) for w in want]
        full = b["kinds"].index("full") if "full" in b["kinds"] else None
        if full is not None:                                                   # the promised frames: empty between non-empty, and full
            assert kept[1] == 0 and kept[0] > 0 and kept[2] > 0
            assert kept[full] == (n if entry == "xyz" else n - int(b["nan_px"].sum()))
        for use_rgb in (False, True):
            for wi in (False, True):
                got = run(entry, use_rgb, False, False, wi)
                assert (got[0][1] is not None) == use_rgb and (got[0][2] is not None) == wi
                CR.compare_frames([[npy(a) for a in fr] for fr in got], want, (shape, entry, use_rgb, wi))
        if extras:
            for cm, dg in ((True, False), (False, True), (True, True)):
                got = run(entry, True, cm, dg, True)
                CR.compare_frames([[npy(a) for a in fr] for fr in got], ref(entry, cm, dg), (shape, entry, "flags", cm, dg))
            pts, col, idx, cnt = run(entry, True, True, True, True, sync=False)
            assert pts.shape == (F, n, 3) and col.shape == (F, n, 3) and idx.shape == (F, n) and cnt.shape == (F,)
            CR.compare_padded(npy(pts), npy(col), npy(idx), npy(cnt), ref(entry, True, True), (shape, entry, "sync=False"))
    del depth, xyz_d, rgb, xy


def test_extract_refuses_frame_counts_beyond_the_grid(ops):
    """the frame count becomes gridDim.y, for which the device reports a limit (65536 on the MI355X): both entries refuse a batch beyond
    it on the host, before any launch.  65535 frames, the largest frame-major batch, still run."""
    from kinectpy_amd._lib import KinectPxError
    F = 65537
    depth = torch.zeros((F, 8), dtype=torch.uint16, device="cuda")
    xy = torch.ones(16, dtype=torch.float32, device="cuda")
    with pytest.raises(KinectPxError, match="kpx_depth_to_cloud: 65537 frames exceed the device's grid limit"):
        ops.depth_to_cloud(depth, xy, None, F, False, False)
    with pytest.raises(KinectPxError, match="kpx_rgbd_compact: 65537 frames exceed the device's grid limit"):
        ops.rgbd_compact(torch.zeros((F, 8, 3), dtype=torch.int16, device="cuda"), None, F, False, False)
    depth[5] = 1000                                                            # one frame keeps its 8 pixels, the others nothing
    got = ops.depth_to_cloud(depth[:65535], xy, None, 65535, False, False)
    assert CR.compact_form(8, 65535, True)[0] == CR.PX8_FRAME_MAJOR and len(got) == 65535
    assert [g[0].shape[0] for g in (got[0], got[5], got[-1])] == [0, 8, 0] and np.array_equal(npy(got[5][0]), np.tile(np.float32([1000, 1000, 1000]), (8, 1)))


# ------------------------------------------------------------------------------------------------ point selections
POINT_SIZES = {
    "2048 tiles": (2048 * T, 0, CR.POINTS_ONEPASS, CR.GENERIC_ONEPASS, (256, False)),
    "2048 tiles + 1": (2048 * T + 1, 0, CR.POINTS_FLAGS, CR.GENERIC_THREE, (1024, False)),
    "2048 tiles + 1, view one row in": (2048 * T + 1, 1, CR.POINTS_FLAGS, CR.GENERIC_THREE, (1024, False)),
    "8192 tiles": (8192 * T, 0, CR.POINTS_FLAGS, CR.GENERIC_THREE, (1024, False)),
    "8192 tiles + 1": (8192 * T + 1, 0, CR.POINTS_FLAGS, CR.GENERIC_THREE, (1024, True)),
}


@pytest.mark.parametrize("size", list(POINT_SIZES))
def test_point_selections_match_numpy(ops, size):
    """half space (one list), slab split with and without bounds (two lists) and mask selection, inverted and not (the generic kernels),
    on a cloud whose kept points come in whole tiles: about one half kept, nothing kept, everything kept"""
    n, off, one_list, generic, scan = POINT_SIZES[size]
    form, sc = CR.compact_form(n, 1, False, lists=1, kind="points")
    assert form == one_list and (sc is None or sc == scan), (size, form, sc)
    assert CR.compact_form(n, 1, False, lists=2, kind="points") == (CR.POINTS_FLAGS, scan)
    gform, gsc = CR.compact_form(n, 1, False, kind="generic")
    assert gform == generic and (gsc is None or gsc == scan)
    host, _ = CR.clustered_cloud(n + off, seed=n % 97 + off)
    dev = torch.as_tensor(host).cuda()[off:]
    p = host[off:]
    assert dev.data_ptr() % 16 == (12 * off) % 16 and len(p) == n
    ymax = float(p[:, 1].max())
    keep = CR.halfspace_ref(p, CR.HALF_PLANE)
    rest = np.flatnonzero(p[:, 1] >= 0).astype(np.int32)
    c = CR.tile_counts(keep, n)
    assert 0.4 < len(keep) / n < 0.6 and (c == 0).sum() > 3 and (c[:-1] == T).sum() > 3
    every, none = np.arange(n, dtype=np.int32), np.zeros(0, np.int32)
    for plane, want in ((CR.HALF_PLANE, keep), (CR.NONE_PLANE, none), (CR.ALL_PLANE, every)):
        got = npy(ops.halfspace_select(dev, plane))
        assert got.shape == want.shape and np.array_equal(got, want), (size, "half space", plane)
    bb = ops.bounds(dev)
    for slab, (wlo, wup) in ((ymax, (rest, keep)), (-1.0, (none, every)), (1e9, (every, none))):
        for bounds in (None, bb):
            lo, up = ops.slab_split(dev, slab, bounds=bounds)
            lo, up = npy(lo), npy(up)
            assert lo.shape == wlo.shape and up.shape == wup.shape, (size, "slab counts", slab, lo.shape, up.shape)
            assert np.array_equal(lo, wlo) and np.array_equal(up, wup), (size, "slab", slab, bounds is not None)
    del lo, up, got
    keep_d = torch.as_tensor(keep).cuda()
    for idx, invert, want in ((keep_d, False, p[keep]), (keep_d, True, p[rest]), (keep_d[:0], False, p[:0]), (keep_d[:0], True, p),
                              (torch.arange(n, dtype=torch.int32, device="cuda"), False, p), (torch.arange(n, dtype=torch.int32, device="cuda"), True, p[:0])):
        got = npy(ops.select_by_index([dev], idx, invert=invert)[0])
        assert got.shape == want.shape and np.array_equal(got, want), (size, "mask", invert, len(idx))
    del dev, keep_d, idx, got
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ forced forms
_WORKER = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, os.getcwd())
from kinectpy_amd import ops
from oracle import oracle as O
from tests import compaction_ref as CR
I = CR.forced_inputs()
out = {}
npy = lambda t: t.cpu().numpy()
def frames(tag, res):
    out[tag + "_cnt"] = np.array([len(r[0]) for r in res])
    for j, name in enumerate(("pts", "col", "idx")):
        out[tag + "_" + name] = np.concatenate([npy(r[j]) for r in res])
for name, b in I["ext"].items():
    F = len(b["depth"])
    frames("d2c_" + name, ops.depth_to_cloud(b["depth"], b["xy"], b["rgb"], F, True, True, want_idx=True))
    frames("xyz_" + name, ops.rgbd_compact(CR.xyz_images(b, O.unproject_u16), b["rgb"], F, True, True, want_idx=True))
c = torch.as_tensor(I["cloud"]).cuda()
out["half"] = npy(ops.halfspace_select(c, CR.HALF_PLANE))
out["half_2049"] = npy(ops.halfspace_select(I["cloud_2049"], CR.HALF_PLANE))
lo, up = ops.slab_split(c, float(I["cloud"][:, 1].max()))
out["slab_lo"], out["slab_up"] = npy(lo), npy(up)
out["mask"] = npy(ops.select_by_index([c], out["half"])[0])
out["mask_inv"] = npy(ops.select_by_index([c], out["half"], invert=True)[0])
vp, vc, vn = ops.voxel_downsample(I["big"], 10.0, I["big_col"], I["big_nrm"])
out["vox_n_p"], out["vox_n_c"], out["vox_n_n"] = npy(vp), npy(vc), npy(vn)
vp, vc, _ = ops.voxel_downsample(I["big"], 10.0, I["big_col"])
out["vox_p"], out["vox_c"] = npy(vp), npy(vc)
for i, (vp, _) in enumerate(ops.voxel_downsample_batch(I["batch"], 10.0)):
    out["vox_b%d" % i] = npy(vp)
fp, fc = ops.fuse_voxel_downsample(I["fuse"], [I["big_col"][: len(I["fuse"][0])], I["big_col"][: len(I["fuse"][1])]], I["fuse_T"], 10.0)
out["fuse_p"], out["fuse_c"] = npy(fp), npy(fc)
keep, stats, _ = ops.sor(I["room"], 20, 2.0)
out["sor"], out["sor_stats"] = npy(keep), npy(stats)
out["radius"] = npy(ops.remove_radius_outlier(I["room"], 8, 25.0))
lab, ncl = ops.cluster_dbscan(I["room"], 25.0, 9)
out["dbscan"], out["dbscan_n"] = npy(lab), npy(ncl)
plane, inl = ops.segment_plane(I["room"], 30.0, 3, 300, seed=7)
out["plane"], out["plane_inl"] = plane, npy(inl)
src, tgt, corr = I["ransac"]
r = ops.ransac_corres(src, tgt, corr, 20.0, 3, 0.95, 70000, 1.0, 5)
out["ransac_T"] = r["transformation"]
out["ransac_s"] = np.array([r["fitness"], r["inlier_rmse"], r["iterations"], r["validations"]])
np.savez(sys.argv[1], **out)
"""

# the children: the default, both forced sides of kOnePassTiles, and batches above the limit sent to count -> scan -> scatter
_SETTINGS = (("default", {}), ("onepass0", {"KPX_ONEPASS": "0"}), ("onepass1", {"KPX_ONEPASS": "1"}), ("batch0", {"KPX_ONEPASS_BATCH": "0"}))


def test_forced_forms_agree_and_match_the_oracle(tmp_path, oracle):
    """KPX_ONEPASS=0 / 1 and KPX_ONEPASS_BATCH=0 (read once per process: a fresh child per setting) over every caller of compact(),
    compact_points() and px8_compact(): every array identical across the children, the default child's equal to the oracle"""
    I = CR.forced_inputs()
    # what the settings move: each form is taken by some child at these sizes
    forms = {name: {k: CR.compact_form(b["depth"].shape[1], len(b["depth"]), k.startswith("vec"),
                                       onepass={"onepass0": 0, "onepass1": 1}.get(name), onepass_batch=name != "batch0")[0]
                    for k, b in I["ext"].items()} for name, _ in _SETTINGS}
    assert forms["default"] == {"vec3": CR.PX8_TILE_MAJOR, "odd3": CR.GENERIC_ONEPASS, "vec8": CR.PX8_FRAME_MAJOR, "odd9": CR.GENERIC_ONEPASS}
    assert forms["onepass0"] == {"vec3": CR.PX8_THREE, "odd3": CR.GENERIC_THREE, "vec8": CR.PX8_FRAME_MAJOR, "odd9": CR.GENERIC_THREE}
    assert forms["onepass1"] == {"vec3": CR.PX8_TILE_MAJOR, "odd3": CR.GENERIC_ONEPASS, "vec8": CR.PX8_TILE_MAJOR, "odd9": CR.GENERIC_ONEPASS}
    assert forms["batch0"]["vec8"] == CR.PX8_THREE and forms["batch0"]["vec3"] == CR.PX8_TILE_MAJOR
    n, n2 = len(I["cloud"]), len(I["cloud_2049"])
    assert CR.compact_form(n, 1, False, kind="points")[0] == CR.POINTS_ONEPASS and CR.compact_form(n, 1, False, kind="points", onepass=0)[0] == CR.POINTS_FLAGS
    assert CR.compact_form(n2, 1, False, kind="points")[0] == CR.POINTS_FLAGS and CR.compact_form(n2, 1, False, kind="points", onepass=1)[0] == CR.POINTS_ONEPASS
    assert all(150 <= CR.tiles_of(len(I[k])) <= 400 for k in ("cloud", "room", "big")) and all(150 <= CR.tiles_of(b["depth"].shape[1]) <= 400 for b in I["ext"].values())
    got = {}
    for name, env in _SETTINGS:
        f = str(tmp_path / (name + ".npz"))
        r = subprocess.run([sys.executable, "-c", _WORKER, f], cwd=ROOT, capture_output=True, text=True, timeout=300, env={**os.environ, **env})
        assert r.returncode == 0, (name, r.stderr[-2000:])
        got[name] = dict(np.load(f))
    base = got["default"]
    for name, _ in _SETTINGS[1:]:
        assert set(got[name]) == set(base)
        for key, v in base.items():
            assert v.shape == got[name][key].shape and np.array_equal(v, got[name][key], equal_nan=True), (name, key)
    # the default child against the oracle
    for name, b in I["ext"].items():
        for entry, imgs in (("d2c", np.stack([oracle.unproject_u16(d, b["xy"]) for d in b["depth"]])), ("xyz", CR.xyz_images(b, oracle.unproject_u16))):
            want = [oracle.rgbd_compact(im, c, True, True, oracle.median_z(im) + CR.GATE_MM) for im, c in zip(imgs, b["rgb"])]
            tag = entry + "_" + name
            assert base[tag + "_cnt"].tolist() == [len(w[0]) for w in want], tag
            for j, key in enumerate(("pts", "col", "idx")):
                assert np.array_equal(base[tag + "_" + key], np.concatenate([w[j] for w in want])), (tag, key)
    c = I["cloud"]
    keep = CR.halfspace_ref(c, CR.HALF_PLANE)
    lo, up = CR.slab_ref(c, float(c[:, 1].max()))
    assert np.array_equal(base["half"], keep) and np.array_equal(base["half_2049"], CR.halfspace_ref(I["cloud_2049"], CR.HALF_PLANE))
    assert np.array_equal(base["slab_lo"], lo) and np.array_equal(base["slab_up"], up)
    assert np.array_equal(base["mask"], CR.mask_select_ref(c, keep)) and np.array_equal(base["mask_inv"], CR.mask_select_ref(c, keep, invert=True))
    rp, rc, rn = oracle.voxel_downsample(I["big"], 10.0, I["big_col"], I["big_nrm"])
    assert np.array_equal(base["vox_n_p"], rp) and np.array_equal(base["vox_n_c"], rc) and np.array_equal(base["vox_n_n"], rn)
    assert np.array_equal(base["vox_p"], rp) and np.array_equal(base["vox_c"], rc)
    for i, x in enumerate(I["batch"]):
        assert np.array_equal(base["vox_b%d" % i], oracle.voxel_downsample(x, 10.0)[0]), i
    cols = [I["big_col"][: len(x)] for x in I["fuse"]]
    fp, fc = oracle.fuse_voxel_downsample(I["fuse"], cols, I["fuse_T"], 10.0)
    assert np.array_equal(base["fuse_p"], fp) and np.array_equal(base["fuse_c"], fc)
    rk, rs, _ = oracle.sor(I["room"], 20, 2.0)
    assert np.array_equal(base["sor"], rk) and np.allclose(base["sor_stats"], rs, rtol=1e-11, atol=0)
    from tests import dbscan_ref as R
    max_nn = 256
    while oracle.hybrid_knn(I["room"], 25.0, max_nn)[1].max() >= max_nn:
        max_nn *= 2
    nbrs = R.oracle_neighbours(oracle, I["room"], 25.0, max_nn)
    assert np.array_equal(base["radius"], np.flatnonzero(R.counts(nbrs[0]) > 8))
    lab = R.dbscan_closed_form(*nbrs, 9)
    assert np.array_equal(base["dbscan"], lab) and int(base["dbscan_n"][0]) == lab.max(initial=-1) + 1
    oplane, oinl = oracle.segment_plane(I["room"], 30.0, 3, 300, seed=7)
    assert np.array_equal(base["plane_inl"], oinl) and np.allclose(base["plane"], oplane, atol=1e-10)
    src, tgt, corr = I["ransac"]
    oT, ost = oracle.ransac_corres(src, tgt, corr, 20.0, 3, 0.95, 70000, 1.0, 5)
    assert base["ransac_s"][0] == ost["fitness"] and (int(base["ransac_s"][2]), int(base["ransac_s"][3])) == (ost["iterations"], ost["validations"])
    assert ost["iterations"] == 70000 and np.abs(base["ransac_T"] - oT).max() < 1e-6
