"""GPU suite: what the library keeps per host thread (pinned read-back blocks, the lanes of a batch that forks) belongs to ONE owner per
thread and goes away with the thread -- kpx_host_resources / ops.host_resources() counts it.  One rendered frame of a two-sensor ring:
one registration is the smallest rig whose frame reaches the ICP batch (progress words) and the voxel grids' width read-back."""
import threading
import time

import numpy as np
import pytest
import torch

from kinectpy_amd import ops
from kinectpy_amd.utils import synth

pytestmark = pytest.mark.gpu

TOL_T = 1e-8           # absolute, ICP 4x4 (rotation entries / mm), as test_parity_gpu.py


def npy(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def frame():
    """the frame on the device, a pipeline over it, and its serial step on the test's own thread (whose resources then exist and stay)"""
    from kinectpy_amd.pipeline import NativeFramePipeline, PipelineParams
    xy, depth, rgb, inits, _ = synth.sensor_ring(2, 1)
    d, c = torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda()
    nat = NativeFramePipeline(xy, 2, inits, PipelineParams())
    gp, gc, gT = nat.step(d, c)
    assert gp.shape[0] > 1000
    return nat, d, c, (npy(gp), npy(gc), gT.copy())


def _after_thread_exit(want):
    """Thread.join() returns once the thread's interpreter state is gone -- an instant BEFORE the OS thread has run its C++ thread_local
    destructors (CPython < 3.13 does not join the OS thread).  Poll, without sleeping, until the counts have settled; the bound only
    matters when they never do."""
    deadline = time.monotonic() + 5.0
    got = ops.host_resources()
    while got != want and time.monotonic() < deadline:
        got = ops.host_resources()
    return got


def test_stream_cycles_give_back_what_their_workers_took(frame):
    """six create / destroy cycles of a four-deep kpx_stream, eight frames each: every popped frame equals the serial step; while the
    stream is open its workers hold pinned memory of their own; after every close() the process holds exactly what it held before --
    kpx_stream_destroy joins the workers, and a worker's owner is destroyed before the join returns"""
    from kinectpy_amd.pipeline import NativeFrameStream
    nat, d, c, (sp, sc, sT) = frame
    r0 = ops.host_resources()
    assert r0["threads"] >= 1 and r0["pinned_bytes"] > 0

    def check(res):
        gp, gc, gT = res
        assert np.array_equal(npy(gp), sp) and np.array_equal(npy(gc), sc) and np.abs(gT - sT).max() < TOL_T

    for cycle in range(6):
        fs = NativeFrameStream(nat, 4)
        popped = 0
        for k in range(8):
            if fs.full():
                check(fs.pop())
                popped += 1
            fs.submit(d, c)
        check(fs.pop())
        popped += 1
        held = ops.host_resources()
        assert held["pinned_bytes"] > r0["pinned_bytes"] and held["threads"] > r0["threads"], (cycle, held, r0)
        while fs.pending:
            check(fs.pop())
            popped += 1
        assert popped == 8
        fs.close()
        assert ops.host_resources() == r0, cycle


def test_python_thread_gives_back_at_exit(frame):
    """a threading.Thread steps the frame once and ends: the same cloud as the serial step, and nothing of the thread's is left -- three
    times in a row"""
    nat, d, c, (sp, sc, sT) = frame
    r0 = ops.host_resources()
    for _ in range(3):
        seen = {}

        def work():
            gp, gc, gT = nat.step(d, c)
            seen["same"] = np.array_equal(npy(gp), sp) and np.array_equal(npy(gc), sc) and np.abs(gT - sT).max() < TOL_T
            seen["held"] = ops.host_resources()

        th = threading.Thread(target=work)
        th.start()
        th.join()
        assert seen["same"]
        assert seen["held"]["pinned_bytes"] > r0["pinned_bytes"] and seen["held"]["threads"] == r0["threads"] + 1
        assert _after_thread_exit(r0) == r0


def test_lanes_appear_only_when_a_batch_forks():
    """one source cloud is one group and runs on the caller's stream: a fresh thread gains no stream and no event, and registers bit for
    bit as the main thread (which has its lanes) does; nine sources are nine chains on the lanes: 4 streams and 5 events, given back
    when the thread ends"""
    rng = np.random.default_rng(5)
    tgt = (rng.random((4000, 3)) * np.array([800.0, 600.0, 30.0])).astype(np.float32)      # a slab: the registration is well posed
    a = 0.02
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    src = ((tgt[:3000].astype(np.float64) - 400.0) @ R.T + 400.0 + np.array([3.0, -2.0, 1.0])).astype(np.float32)
    many = [src[200 * i:200 * i + 500] for i in range(9)]
    tgt_d, src_d, many_d = torch.as_tensor(tgt).cuda(), torch.as_tensor(src).cuda(), [torch.as_tensor(m).cuda() for m in many]
    eye = np.eye(4)

    def single():
        return ops.icp_batch([src_d], tgt_d, 50.0, [eye])[0]

    def forked():
        return ops.icp_batch(many_d, tgt_d, 50.0, [eye] * 9)

    forked()                                     # the main thread has lanes (from here, if no earlier test made them)
    ref = single()
    assert ref["fitness"] > 0.5 and ref["iterations"] >= 1
    before = ops.host_resources()
    assert before["streams"] >= 4 and before["events"] >= 5
    seen = {}

    def work():
        seen["fresh"] = ops.host_resources()
        seen["one"] = single()
        seen["after_one"] = ops.host_resources()
        seen["many"] = forked()
        seen["after_many"] = ops.host_resources()

    th = threading.Thread(target=work)
    th.start()
    th.join()
    fresh, one, many_held = seen["fresh"], seen["after_one"], seen["after_many"]
    assert fresh == before
    assert (one["streams"], one["events"]) == (fresh["streams"], fresh["events"])
    assert one["threads"] == fresh["threads"] + 1 and one["pinned_bytes"] > fresh["pinned_bytes"]      # (its progress words)
    assert (many_held["streams"], many_held["events"]) == (fresh["streams"] + 4, fresh["events"] + 5)
    assert np.array_equal(seen["one"]["transformation"], ref["transformation"])
    assert (seen["one"]["fitness"], seen["one"]["inlier_rmse"], seen["one"]["iterations"], seen["one"]["count"]) == \
           (ref["fitness"], ref["inlier_rmse"], ref["iterations"], ref["count"])
    assert len(seen["many"]) == 9 and all(r["fitness"] > 0.5 for r in seen["many"])
    assert _after_thread_exit(before) == before
