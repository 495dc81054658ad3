"""Writes knn_wave_parent_<case>.npz and knn_wave_parent_frame.npz next to this file: the SOR mean distances, keep lists and statistics,
the normals and the covariances of every cloud of tests/knn_wave_cases.py, and the fused points, colours and transforms of one
four-sensor frame, as the library computed them BEFORE the wave-per-query neighbour kernels took their reductions, scans and broadcasts
from kpx_wave.h and the frame's voxel keys were formed in 32-bit words.  Run on an MI355X with that commit's build loaded through KPX_LIBRARY, or with a built checkout
of that commit first on PYTHONPATH (the files were recorded that way; this script and the cases are taken from where the script lies), and
the commit's id on the command line:

    KPX_LIBRARY=<parent build>/libkinectpx.so python tests/golden/make_knn_wave_golden.py <parent commit id> [output directory]
    PYTHONPATH=<parent checkout> python tests/golden/make_knn_wave_golden.py <parent commit id> [output directory]

tests/test_knn_wave_identity_gpu.py compares the current library against the files bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                            # knn_wave_cases
sys.path.append(os.path.dirname(os.path.dirname(HERE)))             # this checkout's package, unless PYTHONPATH names another


def main(commit, out):
    import knn_wave_cases as S
    from kinectpy_amd import _lib, ops
    os.makedirs(out, exist_ok=True)
    sets = {name: S.run_case(ops, name) for name in S.CASES}
    sets["frame"] = S.run_frame()
    for name, arrays in sets.items():
        path = os.path.join(out, "knn_wave_parent_%s.npz" % name)
        np.savez_compressed(path, parent_commit=np.array(commit), **arrays)
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print(name, {k: v.shape for k, v in arrays.items()}, "->", path, size, "bytes")
    print("library", _lib.SO_PATH)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
