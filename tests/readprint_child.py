"""The device FASTQ printer run over a batch of records -- as a module for tests/test_gpu_readprint.py, and as its child
process, which runs the overflow batch with whatever BBK_CORRECTOR_HOST says in its environment and pickles what came out.

    python tests/readprint_child.py <output file>
"""
import pickle
import sys

import numpy as np

from tests.hreads_child import arrays, device_set


def run_batch(ctx, k, keys, good, left, right=None, tags=True, qvoffset=33, trim_quality=4, prepared=False):
    """records (name, seq, qual) through hammer_reads, correct_resident and print -> dict: the streams as bytes, their
    sizes, per side what Corrected.export(outcome=True) gives as lists, and the corrector's counters.  prepared: also
    check Corrected.export() against correct_prepared on the same batch with a corrector of its own."""
    s = device_set(ctx, keys, k)
    c = s.corrector(good)
    sides, held = [], []
    for recs in (left, right):
        if recs is None:
            continue
        hr = ctx.hammer_reads(*arrays([(seq, qual) for _, seq, qual in recs]), k, trim_quality=trim_quality)
        cr = c.correct_resident(hr)
        assert len(cr) == len(recs)
        ex = cr.export(outcome=True)
        if prepared:
            c2 = s.corrector(good)
            want = c2.correct_prepared(hr)
            assert all(np.array_equal(a, b) for a, b in zip(ex[:4], want)), "export() differs from correct_prepared"
            c2.free()
        sides.append([x.tolist() for x in ex])
        held.append((hr, cr))
    names = [[n for n, _, _ in recs] for recs in (left, right) if recs is not None]
    text = held[0][1].print(names[0], qvoffset=qvoffset, tags=tags, mate=held[1][1] if right is not None else None,
                            mate_names=names[1] if right is not None else None)
    sizes = text.sizes
    out = dict(streams=[text.stream(i) for i in range(len(sizes))], sizes=sizes, sides=sides, stats=c.stats)
    text.free()
    for hr, cr in held:
        cr.free()
        hr.free()
    c.free()
    s.free()
    return out


def overflow_batch(k=21):
    """the batch of test_overflow_goes_to_the_host_rule (tests/test_gpu_readcorrect.py) as named records"""
    from tests import readcorrect_cases as Cs
    from tests import readcorrect_restated as R
    big, qual, good_kmers = R.branching_read(k, 150, step=2)
    small, qual_s, good_s = R.branching_read(k, 60, step=4, seed=6)
    unit = [c for c in Cs.unit_cases(k) if c.what in ("both sides", "N corrected", "every start good")]
    index, keys, good = R.make_index(good_kmers | good_s | set().union(*[c.good for c in unit]))
    reads = [(big, qual), (small, qual_s)] + [(c.seq, c.qual) for c in unit] + [(big, qual)]
    return index, keys, good, [("read %d" % i, s, q) for i, (s, q) in enumerate(reads)]


def main():
    import spades_for_blackbird_amd as B
    k = 21
    _, keys, good, records = overflow_batch(k)
    ctx = B.Context(0)
    got = run_batch(ctx, k, keys, good, records, tags=True, prepared=True)
    ctx.close()
    with open(sys.argv[1], "wb") as f:
        pickle.dump(got, f)


if __name__ == "__main__":
    main()
