"""Child of tests/test_gpu_unitigs.py::test_mega_block_layout: started with SBWTGPU_LIB naming the test build whose mega blocks
hold 2^12 columns (sbwt_amd/build.py), it exports the unitigs of the index in in.npz -- from the default image (relative
counts + mega table) and from the "big_path" 2 image (absolute counts) -- and stores them in out.npz.

    python unitig_mega_worker.py in.npz out.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbwt_amd import capi  # noqa: E402


def main():
    inp = np.load(sys.argv[1], allow_pickle=False)
    n, k, nk = (int(x) for x in inp["meta"])
    out = {"version": np.array(capi.lib().sbwtgpu_version().decode())}
    for name, big in (("rel", 1), ("big", 2)):
        capi.set_tuning("big_path", big)
        for marks in (1, 0):
            idx = capi.Index.create(inp["A"], inp["C"], inp["G"], inp["T"], inp["ssup"] if marks else None, n, k, nk, 0)
            b, o, f = idx.unitigs()
            out["%s%d/bases" % (name, marks)], out["%s%d/off" % (name, marks)], out["%s%d/first" % (name, marks)] = b, o, f
            idx.close()
    capi.set_tuning("big_path", 1)
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
