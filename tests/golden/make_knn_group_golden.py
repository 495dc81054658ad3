"""Writes knn_group_parent_<case>.npz next to this file: the SOR mean distances, keep lists and statistics, the kpx_sor_partial slabs, the
normals and the covariances of every cloud of tests/knn_group_cases.py, as the library computed them BEFORE the group pass
(knn_group_kernel: four queries per wave, settle or hand on) stood in front of the wave-per-query neighbour passes.  Run on an MI355X with
that commit's build loaded through KPX_LIBRARY and the commit's full id on the command line (this script and the cases are taken from
where the script lies; the loader lets the older build lack kpx_knn_group_last):

    KPX_LIBRARY=<parent build>/libkinectpx.so python tests/golden/make_knn_group_golden.py <parent commit id> [output directory]

tests/test_knn_group_gpu.py compares the current library against the files bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                            # knn_group_cases, knn_wave_cases
sys.path.append(os.path.dirname(os.path.dirname(HERE)))             # this checkout's package


def main(commit, out):
    import knn_group_cases as S
    from kinectpy_amd import _lib, ops
    assert len(commit) == 40, "the parent's FULL commit id"
    os.makedirs(out, exist_ok=True)
    for name in S.CASES:
        arrays = S.run_case(ops, name)
        path = os.path.join(out, "knn_group_parent_%s.npz" % name)
        np.savez_compressed(path, parent_commit=np.array(commit), **arrays)
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print(name, {k: v.shape for k, v in arrays.items()}, "->", path, size, "bytes")
    print("library", _lib.SO_PATH)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
