"""bbk_corrector_correct_prepared against bbk_corrector_correct on the golden pair with seeded errors -- as a module for
tests/test_gpu_hreads.py, and as its child process, which runs the comparison with whatever BBK_CORRECTOR_HOST says in its
environment and prints the number of searches that went through the host rule.

    python tests/hreads_child.py <golden dir>
"""
import sys

import numpy as np


def arrays(records):
    """(bases np.uint8, quals np.uint8, offsets np.uint64[n + 1]) of [(seq, qual)]"""
    off = np.zeros(len(records) + 1, dtype=np.uint64)
    if records:
        off[1:] = np.cumsum([len(s) for s, _ in records], dtype=np.uint64)
    bases = np.frombuffer("".join(s for s, _ in records).encode("latin-1"), dtype=np.uint8)
    quals = np.array([x for _, q in records for x in q], dtype=np.uint8)
    return bases, quals, off


def golden_inputs(golden_dir, k=21):
    """(k, keys, good, the trimmed reads bbk_corrector_correct takes, the same reads as parsed)"""
    from tests import readcorrect_cases as Cs
    index, keys, good, trimmed = Cs.golden_case(golden_dir, k)
    raw = Cs.seeded_errors(Cs.golden_reads(golden_dir), 0.02, 2024)  # the reads golden_case trims
    return k, keys, good, trimmed, raw


def device_set(ctx, keys, k):
    import torch
    d = torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(d, len(keys), k)
    s._keep = d
    return s


def compare_corrections(ctx, inputs):
    """both doors over the same reads: bases, offsets, flags, where and the five counters are equal; returns the
    counters and the values `where` takes"""
    k, keys, good, trimmed, raw = inputs
    s = device_set(ctx, keys, k)
    c1, c2 = s.corrector(good), s.corrector(good)
    bases, quals, off = arrays(trimmed)
    out1, res1, where1 = c1.correct_arrays(bases, quals, off)
    hr = ctx.hammer_reads(*arrays(raw), k)
    out2, off2, res2, where2 = c2.correct_prepared(hr)
    assert np.array_equal(off, off2) and np.array_equal(out1, out2)
    assert np.array_equal(res1, res2) and np.array_equal(where1, where2) and c1.stats == c2.stats
    assert not np.array_equal(out1, bases)
    st, wh = c1.stats, sorted(set(where1.tolist()))
    for x in (hr, c1, c2, s):
        x.free()
    return st, wh


def main():
    import spades_for_blackbird_amd as B
    ctx = B.Context(0)
    st, wh = compare_corrections(ctx, golden_inputs(sys.argv[1]))
    ctx.close()
    assert wh == [0, 2], wh
    print("host searches %d" % st["host_searches"])


if __name__ == "__main__":
    main()
