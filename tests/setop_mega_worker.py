"""Child of tests/test_gpu_setops.py::test_mega_block_layout: started with SBWTGPU_LIB naming the test build whose mega blocks
hold 2^12 columns (sbwt_amd/build.py), it runs the four set operations on the two indexes in in.npz -- from the default image
(relative counts + mega table) and from the "big_path" 2 image (absolute counts), with marks and without -- and stores the
results and a's keys in out.npz.

    python setop_mega_worker.py in.npz out.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbwt_amd import capi  # noqa: E402

OPS = ("union", "intersection", "difference", "symmetric-difference")


def main():
    inp = np.load(sys.argv[1], allow_pickle=False)
    k = int(inp["meta"][0])
    out = {"version": np.array(capi.lib().sbwtgpu_version().decode())}

    def create(name, marks):
        n, nk = (int(x) for x in inp[name + "/meta"])
        return capi.Index.create(inp[name + "/A"], inp[name + "/C"], inp[name + "/G"], inp[name + "/T"],
                                 inp[name + "/ssup"] if marks else None, n, k, nk, 0)
    for name, big in (("rel", 1), ("big", 2)):
        capi.set_tuning("big_path", big)
        for marks in (1, 0):
            image = "%s%d" % (name, marks)
            ia, ib = create("a", marks), create("b", 1 - marks)
            out[image + "/keys"] = ia.kmer_keys()
            for op in OPS:
                bits, info = ia.setop(ib, op)
                pre = "%s/%s/" % (image, op)
                for c in range(4):
                    out[pre + "ACGT"[c]] = bits.cols[c]
                out[pre + "ssup"] = bits.ssup
                out[pre + "meta"] = np.array([bits.n_nodes, bits.n_kmers, info["n_both"], info["n_either"]], dtype=np.int64)
            ia.close()
            ib.close()
    capi.set_tuning("big_path", 1)
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
