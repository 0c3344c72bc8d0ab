"""Shared test helpers (pure Python, no reference code)."""
import gzip

import numpy as np

_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def rc(s):
    return s[::-1].translate(_COMP)


def read_fastq_gz(path):
    out = []
    with gzip.open(path, "rt") as f:
        while True:
            h = f.readline()
            if not h:
                break
            out.append(f.readline().strip())
            f.readline()
            f.readline()
    return out


def gpu_gfa(ctx, reads, k, tmp_path, name="g.gfa"):
    """(GFA text, Unitigs) of the engine for a list of reads"""
    r = ctx.reads_from_ascii(reads)
    x = ctx.extindex(r, k)
    u = ctx.unitigs(x)
    p = str(tmp_path / name)
    u.write_gfa(p)
    with open(p) as f:
        return f.read(), u


def gfa_bytes(u, path):
    u.write_gfa(str(path))
    with open(str(path), "rb") as f:
        return f.read()


def expected_gfa(u, k):
    """the GFA text of a result without coverage, from its exported sequences and links"""
    lines = ["S\t%d\t%s\tDP:f:0\tKC:i:0\n" % (3 + 2 * i, s) for i, s in enumerate(u.sequences())]
    lines += ["L\t%d\t%s\t%d\t%s\t%dM\n" % (3 + 2 * a, "+" if oa else "-", 3 + 2 * b, "+" if ob else "-", k)
              for a, oa, b, ob in u.links().tolist()]
    return "".join(lines).encode()


def synth_reads(n_reads, read_len=150, genome_len=None, sub_rate=0.005, seed=42, n_rate=0.0):
    """Synthetic reads in the shape of SURVEY 8(d): uniform genome, uniform starts,
    random strand, substitutions; optional N injection for the LongestValid rule."""
    rng = np.random.default_rng(seed)
    if genome_len is None:
        genome_len = max(read_len + 1, n_reads * read_len // 50)
    g = rng.integers(0, 4, size=genome_len, dtype=np.uint8)
    starts = rng.integers(0, genome_len - read_len + 1, size=n_reads)
    idx = starts[:, None] + np.arange(read_len)[None, :]
    r = g[idx]
    sub = rng.random(r.shape) < sub_rate
    r = np.where(sub, (r + rng.integers(1, 4, size=r.shape, dtype=np.uint8)) & 3, r).astype(np.uint8)
    flip = rng.random(n_reads) < 0.5
    r[flip] = (3 - r[flip])[:, ::-1]
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    asc = lut[r]
    if n_rate > 0:
        asc = np.where(rng.random(asc.shape) < n_rate, np.uint8(ord("N")), asc)
    return [bytes(row).decode() for row in asc]


def polya_reads(seed=5, n_tx=8, read_len=150, n_reads=1500, n_tail=400, sub_rate=0.01):
    """RNA-seq-shaped reads: random transcripts of 300-3000 bp with poly-A tails of 10-60 bp, reads on random strands
    with 1 % substitutions (errors inside the tails make low-complexity tips), a share of them ending inside the tail;
    plus a few poly-C reads (complex flanks: the C run becomes a junction) and a few (AT)n reads (never clipped)."""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    txs = [np.concatenate([rng.integers(0, 4, size=int(rng.integers(300, 3001)), dtype=np.uint8),
                           np.zeros(int(rng.integers(10, 61)), dtype=np.uint8)]) for _ in range(n_tx)]
    reads = []

    def emit(t, start):
        r = t[start:start + read_len].copy()
        err = rng.random(len(r)) < sub_rate
        r[err] = (r[err] + rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)) & 3
        if rng.random() < 0.5:
            r = (3 - r)[::-1]
        reads.append(bytes(lut[r]).decode())
    for _ in range(n_reads):
        t = txs[int(rng.integers(0, n_tx))]
        emit(t, int(rng.integers(0, len(t) - read_len + 1)))
    for _ in range(n_tail):
        t = txs[int(rng.integers(0, n_tx))]
        emit(t, len(t) - int(rng.integers(0, 10)) - read_len)
    for _ in range(4):
        flank = [bytes(lut[rng.integers(0, 4, size=10, dtype=np.uint8)]).decode() for _ in range(2)]
        reads.append(flank[0] + "C" * 130 + flank[1])
        reads.append("AT" * 75)
    return reads


def check_profile_join(ctx, tmp_path, k, sets, exported, min_samples, min_mult=5, ci=2, cs=255):
    """profile == restatement: arrays, files, and the files loaded again"""
    from tests import kmerprofile_restated as R
    n_samples, nw = len(sets), R.words(k)
    p = ctx.kmerprofile(k, sets, min_samples, min_mult=min_mult, ci=ci, cs=cs)
    rk, rr = R.join([R.filter_sample(keys, cnt, ci, cs) for keys, cnt in exported], min_samples, min_mult)
    exp_keys = np.array(rk, dtype=np.uint64).reshape(len(rk), nw)
    exp_rows = np.array(rr, dtype=np.uint16).reshape(len(rr), n_samples)
    assert len(p) == len(rk) and p.samples == n_samples and p.k == k
    assert p.keys().tobytes() == exp_keys.tobytes()
    assert p.rows().tobytes() == exp_rows.tobytes()
    prefix = str(tmp_path / ("prof_%d_%d_%d_%d" % (min_samples, min_mult, ci, cs)))
    p.write(prefix)
    assert open(prefix + ".kmers", "rb").read() == R.kmers_bytes(rk)
    assert open(prefix + ".bpr", "rb").read() == R.bpr_bytes(rr)
    q = ctx.kmerprofile_load(prefix, k, n_samples)
    assert len(q) == len(rk) and q.keys().tobytes() == exp_keys.tobytes() and q.rows().tobytes() == exp_rows.tobytes()
    return p, rk, rr
