"""Farthest-point sampling: microseconds per sample of one form against cloud size (the KPX_FPS_BLOCK_MAX_N crossover).
HIP events around each call, median of --reps after a warm-up; clouds are random subsets of the synthetic frame cloud (tiled
beyond its 283k points).  One JSON line per size.

    python tools/fps_probe.py --form block|chain [--k 256] [--sizes 20000,40000,...]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=("block", "chain", "auto"), default="auto")
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="8000,19456,30000,40000,49152,65536,100000,283000")
    a = ap.parse_args()
    if a.form != "auto":
        os.environ["KPX_FPS_FORM"] = a.form          # read once, at the library's first FPS call
    import torch
    from kinectpy_amd import ops
    from kinectpy_amd.utils import synth
    base = synth.frame_cloud()
    rng = np.random.default_rng(0)
    for n in (int(s) for s in a.sizes.split(",")):
        reps = -(-n // len(base))
        pool = np.concatenate([base + np.float32([0, 0, 5000 * r]) for r in range(reps)])
        pts = torch.as_tensor(pool[rng.choice(len(pool), n, replace=False)]).cuda()
        for _ in range(2):
            ops.farthest_point_sample(pts, a.k, 0, True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.farthest_point_sample(pts, a.k, 0, True)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = float(np.median(ts))
        print(json.dumps({"form": a.form, "n": n, "k": a.k, "ms": round(ms, 4), "us_per_sample": round(1e3 * ms / a.k, 3)}), flush=True)


if __name__ == "__main__":
    main()
