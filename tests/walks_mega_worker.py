"""Child of tests/test_gpu_walks.py::test_mega_block_layout: started with SBWTGPU_LIB naming the test build whose mega blocks
hold 2^12 columns (sbwt_amd/build.py), it threads the reads of in.npz through the unitig graph of the index in in.npz -- the
plain graph and the coloured one under the colour-set arrays given, from the default image (relative counts + mega table) and
from the "big_path" 2 image (absolute counts), with the marks given and derived -- and stores every array in out.npz.

    python walks_mega_worker.py in.npz out.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbwt_amd import capi  # noqa: E402


def store(out, tag, idx, u, bases, off):
    out[tag + "step_off"], out[tag + "steps"], out[tag + "coverage"] = u.walks(idx, bases, off, coverage=True)


def main():
    inp = np.load(sys.argv[1], allow_pickle=False)
    n, k, nk, n_colors = (int(x) for x in inp["meta"])
    out = {"version": np.array(capi.lib().sbwtgpu_version().decode())}
    for name, big in (("rel", 1), ("big", 2)):
        capi.set_tuning("big_path", big)
        for marks in (1, 0):
            idx = capi.Index.create(inp["A"], inp["C"], inp["G"], inp["T"], inp["ssup"] if marks else None, n, k, nk, 0)
            with idx.unitig_graph_dev(links=False, column_map=True) as u:
                store(out, "%s%d/plain/" % (name, marks), idx, u, inp["bases"], inp["off"])
            with capi.ColorSets.from_arrays(idx, n_colors, inp["ids"], inp["table"]) as s, \
                    s.unitig_graph_dev(links=False, column_map=True) as u:
                store(out, "%s%d/colored/" % (name, marks), idx, u, inp["bases"], inp["off"])
            idx.close()
    capi.set_tuning("big_path", 1)
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
