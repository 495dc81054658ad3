"""Share of the queries the group pass of the neighbour search (knn_group_kernel) settles in the bench's frame: one frame set of the
four-sensor ring through the Python frame loop (the same operators with the same parameters as the native loop), ops.knn_group_last()
read after the master's normals and after the fused cloud's outlier filter.    python tools/knn_group_share.py"""
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
from kinectpy_amd import ops
from kinectpy_amd.pipeline import PipelineParams, SensorGroupPipeline
from kinectpy_amd.utils import synth

seen = []


def noting(fn, what):
    def call(*a, **k):
        out = fn(*a, **k)
        seen.append((what, a[1:], ops.knn_group_last()))
        return out
    return call


ops.estimate_normals = noting(ops.estimate_normals, "estimate_normals (radius, max_nn)")
ops.sor = noting(ops.sor, "remove_statistical_outlier (k, ratio)")
xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
SensorGroupPipeline(xy, inits, PipelineParams()).step(torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda())
for what, args, (given, handed) in seen:
    print(f"{what} {args}: {given} queries, {given - handed} settled by the group pass ({100.0 * (given - handed) / max(given, 1):.1f} %), {handed} handed on")
