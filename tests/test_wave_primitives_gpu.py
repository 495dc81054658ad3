"""csrc/kpx_wave.h: the whole-wave reductions, the scan, the broadcast and the fixed-tree floating-point sums that run on the vector ALU
(DPP row moves, v_permlane16_swap / v_permlane32_swap, v_readlane) where the shuffles went through ds_bpermute.  kpx_wave_selftest
applies one primitive to rows of 64 values -- one block of four waves, wave w takes rows w, w + 4, ... -- and returns what every lane
holds; each is compared bit for bit against its restatement in NumPy.  For the floating-point sums that is the explicit tree of
`for (o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64)`: at step o lane i < o adds the value of lane i + o, in IEEE arithmetic of
the value's own width; only lane 0 is defined."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUM_I32, MIN_U32, MAX_U32, MAX_U64, MAX_F64, INCL_SCAN_I32, BCAST, SUM_DOWN_F64, SUM_DOWN_F32, SUM_DOWN_F64X9 = range(10)
ROWS = 256


def run(kind, words):
    """words: u64 (rows, 64) -> u64 (rows, 64)"""
    import torch
    from kinectpy_amd import _lib as L
    words = np.ascontiguousarray(words, dtype=np.uint64)
    assert words.ndim == 2 and words.shape[1] == 64
    src = torch.as_tensor(words.view(np.int64)).cuda()
    dst = torch.full_like(src, -1)
    L.check(L.load().kpx_wave_selftest(kind, L.ptr(src), words.shape[0], L.ptr(dst), L.stream_ptr()))
    return dst.cpu().numpy().view(np.uint64)


def int_rows(rng, bits):
    """random rows plus the edge patterns: zeros, the largest value(s), INT_MAX, a single non-zero lane, all lanes equal"""
    top = (1 << bits) - 1
    w = rng.integers(0, top, (ROWS, 64), dtype=np.uint64, endpoint=True)
    w[0] = 0
    w[1] = top
    w[2] = 0x7FFFFFFF
    w[3] = 0; w[3, 37] = top
    w[4] = 0; w[4, 0] = 0x7FFFFFFF; w[4, 63] = 1                     # the sum wraps like int
    w[5] = top; w[5, 16] = 0                                          # the minimum in one lane
    w[6] = rng.integers(0, 8, 64)                                     # many equal values
    w[7] = np.arange(64)
    w[8] = np.arange(64)[::-1]
    if bits == 64:
        w[9] = 0xFFFFFFFF00000000; w[9, 5] = 0xFFFFFFFF00000001       # equal high words: the low word decides
        w[10] = 0x00000000FFFFFFFF; w[10, 50] = 0x0000000100000000    # a larger low word under a smaller high word
        w[11] = 0xFFFFFFFFFFFFFFFF; w[11, 1] = 0xFFFFFFFFFFFFFFFE
    for r in range(12, 76):                                           # a single distinct lane, every position
        w[r] = 5; w[r, r - 12] = 9 if r % 2 else 2
    return w


def f64_rows(rng):
    v = rng.normal(0.0, 1.0, (ROWS, 64)) * 10.0 ** rng.integers(-8, 8, (ROWS, 64))
    v[0] = 0.0
    v[1] = -0.0
    v[2] = 0.0; v[2, ::2] = -0.0
    v[3] = 5e-324 * rng.integers(1, 1000, 64)                         # denormals
    v[4] = 1e-300; v[4, ::3] = 1e300                                  # 1e300 next to 1e-300
    v[5] = 1e300; v[5, 1::2] = -1e300; v[5, 7] = 1e-300
    v[6] = 0.1                                                        # all equal
    v[7] = 1.0 / 3.0
    for r in range(8, 72):                                            # a single non-zero lane, every position
        v[r] = 0.0; v[r, r - 8] = np.pi * (r + 1)
    v[72] = 2.0 ** np.arange(64) * (1.0 + 2.0 ** -52)                 # every addition rounds
    v[73] = v[72, ::-1]
    v[74] = 1.7e308; v[74, 32:] = -1.7e308                            # overflows in another association, not in this one
    return v


def down_tree(v):
    """lane 0 of the __shfl_down tree, in the dtype of v"""
    v = v.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v[:, :o] = v[:, :o] + v[:, o:2 * o]
    return v[:, 0]


def test_integer_reductions_in_every_lane():
    rng = np.random.default_rng(1)
    w = int_rows(rng, 32)
    for kind, ref in ((SUM_I32, w.sum(1) & 0xFFFFFFFF), (MIN_U32, w.min(1)), (MAX_U32, w.max(1))):
        got = run(kind, w)
        assert np.array_equal(got, np.repeat(ref.astype(np.uint64)[:, None], 64, 1)), kind
    w = int_rows(rng, 64)
    assert np.array_equal(run(MAX_U64, w), np.repeat(w.max(1)[:, None], 64, 1))


def test_inclusive_scan_and_broadcast():
    rng = np.random.default_rng(2)
    w = int_rows(rng, 32)
    w[1] = 0x01FFFFFF                                                  # 64 of them stay below 2^31
    assert np.array_equal(run(INCL_SCAN_I32, w), np.cumsum(w, axis=1) & 0xFFFFFFFF)
    assert np.array_equal(run(BCAST, w), np.repeat(w[np.arange(ROWS), np.arange(ROWS) % 64][:, None], 64, 1))


def test_f64_maximum_in_every_lane():
    rng = np.random.default_rng(3)
    v = np.abs(f64_rows(rng))                                          # squared distances: no NaN, no negative zero
    v[1] = 0.0; v[2] = 0.0
    got = run(MAX_F64, v.view(np.uint64))
    assert np.array_equal(got, np.repeat(v.max(1).view(np.uint64)[:, None], 64, 1))
    s = f64_rows(rng)                                                  # signed values; zeros of both signs compare equal (the sign is open)
    s[1] = -3.0; s[2] = -1e-300
    got = run(MAX_F64, s.view(np.uint64)).view(np.float64)
    assert np.array_equal(got, np.repeat(s.max(1)[:, None], 64, 1))


def test_f64_and_f32_sums_keep_the_shuffle_tree():
    rng = np.random.default_rng(4)
    v = f64_rows(rng)
    assert np.array_equal(run(SUM_DOWN_F64, v.view(np.uint64))[:, 0], down_tree(v).view(np.uint64))
    with np.errstate(over="ignore", under="ignore"):
        f = v.astype(np.float32)                                       # (values beyond float32 become inf and 0: still one defined tree)
    f[72] = (2.0 ** np.arange(64) * (1.0 + 2.0 ** -23)).astype(np.float32)
    got = run(SUM_DOWN_F32, f.view(np.uint32).astype(np.uint64))[:, 0]
    ref = down_tree(f)
    ok = ~np.isnan(ref)                                                # inf - inf: NaN either way, the payload is not specified
    assert np.array_equal(got[ok], ref.view(np.uint32).astype(np.uint64)[ok]) and np.isnan(got[~ok].astype(np.uint32).view(np.float32)).all()


def test_nine_sums_at_once_keep_each_tree():
    rng = np.random.default_rng(5)
    v = np.concatenate([f64_rows(rng), f64_rows(rng)[:5]])            # 261 rows = 29 groups of nine: rows of every kind in every slot
    assert len(v) % 9 == 0
    got = run(SUM_DOWN_F64X9, v.view(np.uint64))
    assert np.array_equal(got[:, 0], down_tree(v).view(np.uint64))
