"""Child of tests/test_gpu_colored_unitigs.py::test_mega_block_layout: started with SBWTGPU_LIB naming the test build whose mega
blocks hold 2^12 columns (sbwt_amd/build.py), it exports the coloured unitigs of the index and the colour-set arrays in in.npz
-- from the default image (relative counts + mega table) and from the "big_path" 2 image (absolute counts), with the marks
given and derived -- and stores them in out.npz.

    python colored_unitig_mega_worker.py in.npz out.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbwt_amd import capi  # noqa: E402


def main():
    inp = np.load(sys.argv[1], allow_pickle=False)
    n, k, nk, n_colors = (int(x) for x in inp["meta"])
    out = {"version": np.array(capi.lib().sbwtgpu_version().decode())}
    for name, big in (("rel", 1), ("big", 2)):
        capi.set_tuning("big_path", big)
        for marks in (1, 0):
            idx = capi.Index.create(inp["A"], inp["C"], inp["G"], inp["T"], inp["ssup"] if marks else None, n, k, nk, 0)
            with capi.ColorSets.from_arrays(idx, n_colors, inp["ids"], inp["table"]) as s, s.unitigs_dev() as u:
                b, o, f = u.copy()
                tag = "%s%d/" % (name, marks)
                out[tag + "bases"], out[tag + "off"], out[tag + "first"], out[tag + "set_id"] = b, o, f, u.set_ids()
                out[tag + "breaks"] = np.array(u.color_info()["n_color_breaks"], dtype=np.int64)
            idx.close()
    capi.set_tuning("big_path", 1)
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
