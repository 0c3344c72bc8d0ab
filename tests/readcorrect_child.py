"""Child process of tests/test_gpu_readcorrect.py: corrects the reads of <dir>/reads.txt over the set of <dir>/keys.npy and
<dir>/good.npy with whatever BBK_CORRECTOR_HOST says in its environment, and writes <dir>/out.txt: one "<flag> <read>" line
per read, then the five counters, then the `where` bytes.

    python tests/readcorrect_child.py <dir> <k>
"""
import sys

import numpy as np


def main():
    import torch

    import spades_for_blackbird_amd as B
    d, k = sys.argv[1], int(sys.argv[2])
    keys, good = np.load(d + "/keys.npy"), np.load(d + "/good.npy")
    reads = []
    with open(d + "/reads.txt") as f:
        for line in f.read().split("\n")[:-1]:
            w = line.split()
            reads.append((w[0], [ord(c) - 33 for c in w[1]]) if w else ("", []))
    ctx = B.Context(0)
    dev = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(dev, len(keys), k)
    c = s.corrector(good)
    out, res, where = c.correct(reads)
    st = c.stats
    with open(d + "/out.txt", "w") as f:
        for r, o in zip(res.tolist(), out):
            f.write("%d %s\n" % (r, o))
        f.write(" ".join(str(st[x]) for x in B.Corrector.STATS) + "\n")
        f.write(" ".join(str(x) for x in where.tolist()) + "\n")
    c.free()
    s.free()
    ctx.close()


if __name__ == "__main__":
    main()
