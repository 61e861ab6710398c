"""Child of tests/test_gpu_unitig_links.py::test_mega_block_layout: started with SBWTGPU_LIB naming the test build whose mega
blocks hold 2^12 columns (sbwt_amd/build.py), it makes the unitig graph of the index in in.npz -- the plain run and the coloured
run under the colour-set arrays given, from the default image (relative counts + mega table) and from the "big_path" 2 image
(absolute counts), with the marks given and derived -- and stores every array in out.npz.

    python unitig_links_mega_worker.py in.npz out.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbwt_amd import capi  # noqa: E402


def store(out, tag, u):
    out[tag + "bases"], out[tag + "off"], out[tag + "first"] = u.copy()
    out[tag + "link_off"], out[tag + "link_to"] = u.links()
    out[tag + "col_unitig"], out[tag + "col_offset"] = u.column_map()


def main():
    inp = np.load(sys.argv[1], allow_pickle=False)
    n, k, nk, n_colors = (int(x) for x in inp["meta"])
    out = {"version": np.array(capi.lib().sbwtgpu_version().decode())}
    for name, big in (("rel", 1), ("big", 2)):
        capi.set_tuning("big_path", big)
        for marks in (1, 0):
            idx = capi.Index.create(inp["A"], inp["C"], inp["G"], inp["T"], inp["ssup"] if marks else None, n, k, nk, 0)
            with idx.unitig_graph_dev(links=True, column_map=True) as u:
                store(out, "%s%d/plain/" % (name, marks), u)
            with capi.ColorSets.from_arrays(idx, n_colors, inp["ids"], inp["table"]) as s, \
                    s.unitig_graph_dev(links=True, column_map=True) as u:
                store(out, "%s%d/colored/" % (name, marks), u)
            idx.close()
    capi.set_tuning("big_path", 1)
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
