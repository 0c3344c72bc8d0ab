"""The crafted reads of the singleton-filter tests (tests/test_gpu_hammer_filtered.py, tests/test_gpu_hammer_driver.py): a
400-base genome at about 6x, a handful of substituted bases so that singleton k-mers exist, and two reads that consist of
singletons only.  Pure Python."""
from tests import kmerdata_restated as KR
from tests import readcorrect_restated as R

K = 21
READ_LEN = 60


def genome_reads(seed, n_reads=40, quality=35, substitutions=(3, 11, 19, 27, 35), glen=400, shift=0, name="r%d"):
    """(genome, [(name, seq, qual)]): read i is READ_LEN bases of the genome from an evenly spaced start (moved on by
    `shift`, around the end), every second one reverse complemented; the reads named in `substitutions` carry one wrong
    base of quality 8 in their middle"""
    g = R.genome(glen, seed, K)
    out = []
    for i in range(n_reads):
        st = (i * (glen - READ_LEN) // (n_reads - 1) + shift) % (glen - READ_LEN + 1)
        s, q = list(g[st:st + READ_LEN]), [quality] * READ_LEN
        if i in substitutions:
            p = READ_LEN // 2 + (i % 5)
            s[p] = R.NUCL[(R.NUCL.index(s[p]) + 1 + i % 3) % 4]
            q[p] = 8
        s = "".join(s)
        if i % 2:
            s, q = KR.revcomp(s), q[::-1]
        out.append((name % i, s, q))
    return g, out


def crafted_pair(seed=9, quality=35, left_subst=(3, 11, 19), right_subst=(5, 27), lonely=True):
    """(left, right) records of one paired library over the same genome; with `lonely` the left mate of pair 7 is a read
    of another genome at quality 12"""
    _, left = genome_reads(seed, quality=quality, substitutions=left_subst, name="p%d/1")
    _, right = genome_reads(seed, quality=quality, substitutions=right_subst, shift=150, name="p%d/2")
    if lonely:
        left[7] = (left[7][0], R.genome(150, seed + 1, K)[:READ_LEN], [12] * READ_LEN)
    return left, right


def filtered_case(seed=5):
    """(genome, records): the genome reads plus two reads of another genome, whose k-mers occur once each"""
    g, recs = genome_reads(seed)
    other = R.genome(150, seed + 1, K)
    mine = set(R.kmers_of(g, K)) | {KR.revcomp(x) for x in R.kmers_of(g, K)}
    assert not mine & set(R.kmers_of(other, K))
    recs.insert(7, ("lonely0", other[:READ_LEN], [40] * READ_LEN))
    recs.append(("lonely1", KR.revcomp(other[70:70 + READ_LEN]), [40] * READ_LEN))
    return g, recs


def counted(records, k=K):
    """{k-mer: multiplicity} over both strands of the valid k-mers, as pass 1 counts them"""
    data = KR.fill_kmer_data([(s, q) for _, s, q in records], k)
    return {km: st.count for km, st in data.items()}


def filtered_set(records, k=K, min_count=2):
    """(k-mers in the order of the set, their keys): the k-mers counted at least min_count times"""
    kept = sorted((km for km, c in counted(records, k).items() if c >= min_count), key=KR.kmer_key)
    return kept, [KR.kmer_key(x) for x in kept]


def fastq_text(records, offset=33):
    return "".join("@%s\n%s\n+\n%s\n" % (n, s, "".join(chr(x + offset) for x in q)) for n, s, q in records)
