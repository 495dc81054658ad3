"""Writes icp_wave_leave_parent.npz next to this file: transform, fitness, inlier rmse, iterations and count of every case of
tests/icp_wave_leave_cases.py, as the library computed them BEFORE the waves of the block form (icp_iter_body) ended with their rows
and the last one to arrive closed the block.  Run on an MI355X with that commit's build loaded through KPX_LIBRARY and its id on the
command line:

    KPX_LIBRARY=<parent build>/libkinectpx.so python tests/golden/make_icp_wave_leave_golden.py <parent commit id> [out.npz]

tests/test_icp_wave_leave_gpu.py compares the current library against the file bit for bit, in every form of the iteration."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                            # icp_wave_leave_cases
sys.path.append(os.path.dirname(os.path.dirname(HERE)))             # this checkout's package (the library: KPX_LIBRARY)


def main(commit, path):
    import icp_wave_leave_cases as S
    from kinectpy_amd import _lib, ops
    arrays = S.run(ops)
    assert arrays.pop("unstable")[0] == 0.0, "the recording build does not repeat itself"
    for mode in S.MODES:
        print(mode, "iterations of the batch:", [int(arrays["%s.it30.batch.%s.s" % (mode, n)][2]) for n in S.BATCH],
              "far", arrays["%s.it30.icp.far.s" % mode], "mixed", arrays["%s.it30.icp.mixed.s" % mode])
    arrays["parent_commit"] = np.array(commit)
    np.savez_compressed(path, **arrays)
    print(len(arrays), "arrays ->", path, os.path.getsize(path), "bytes; library", _lib.SO_PATH)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "icp_wave_leave_parent.npz"))
