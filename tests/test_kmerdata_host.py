"""CPU: the host side of spades-kmerdata (host/hammer_reads.hpp, through bbk-hammer-reads-dump) against the restatement's
valid k-mer starts, coalesced: on the crafted reads that take every corner of the trimming rule and of the generator,
and on a real FASTQ file.  The header is also run under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone
host program."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import kmerdata_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [10, 11, 21, 22, 32]


@pytest.fixture(scope="module")
def dump_exe():
    from spades_for_blackbird_amd import build_host
    return [e for e in build_host.build() if e.endswith("bbk-hammer-reads-dump")][0]


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [tuple(int(x) for x in line.split()) for line in r.stdout.split("\n")[:-1]]


def _expected(reads, k, trim_quality=4):
    out = []
    for i, (seq, qual) in enumerate(reads):
        out += [(i, s, n) for s, n in R.coalesce(R.valid_starts(seq, qual, k, trim_quality), k)]
    return out


def _write_fastq(path, reads, offset=33):
    with open(path, "w") as f:
        for i, (seq, qual) in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, seq, "".join(chr(q + offset) for q in qual)))


def _crafted(k):
    return [(s, q) for _, s, q in R.crafted_reads(k, np.random.default_rng(100 + k))]


@pytest.mark.parametrize("k", KS)
def test_crafted_reads(dump_exe, tmp_path, k):
    reads = _crafted(k)
    exp = _expected(reads, k)
    assert len(exp) >= 9
    p = str(tmp_path / "c.fq")
    _write_fastq(p, reads)
    assert _run(dump_exe, ["-k", str(k), p]) == exp
    # another offset and another trimming threshold
    _write_fastq(p, reads, offset=64)
    assert _run(dump_exe, ["-k", str(k), "--qvoffset", "64", p]) == exp
    assert _run(dump_exe, ["-k", str(k), "--qvoffset", "64", "--trim-quality", "2", p]) == _expected(reads, k, 2)


def _read_fastq_gz(path):
    with gzip.open(path, "rt") as f:
        lines = f.read().split("\n")
    return [(lines[i + 1], [ord(c) - 33 for c in lines[i + 3]]) for i in range(0, len(lines) - 3, 4)]


def test_real_fastq(dump_exe, golden_dir):
    path = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    reads = _read_fastq_gz(path)
    # 2054 reads of up to 100 bases (958 of them whole), no N, qualities 2..41
    assert len(reads) == 2054 and all(len(s) <= 100 and "N" not in s for s, _ in reads)
    assert min(min(q) for _, q in reads) == 2 and max(max(q) for _, q in reads) == 41
    exp = _expected(reads, 21)
    assert sum(1 for _, s, n in exp if n < 100) > 500  # many q = 2 tails
    assert _run(dump_exe, [path]) == exp  # k = 21 is the default
    assert _run(dump_exe, ["-k", "32", path]) == _expected(reads, 32)


def test_header_under_sanitizers(tmp_path):
    from spades_for_blackbird_amd import build_host
    exe = build_host.build_sanitized(program="bbk-hammer-reads-dump")
    for k in KS:
        reads = _crafted(k) + [("", []), ("A", [40]), ("N", [40])]
        p = str(tmp_path / ("s%d.fq" % k))
        _write_fastq(p, reads)
        # an empty record is no record for the reader: compare over what it yields
        kept = [r for r in reads if r[0]]
        assert _run(exe, ["-k", str(k), p]) == _expected(kept, k)
        assert _run(exe, ["-k", str(k), "--trim-quality", "0", p]) == _expected(kept, k, 0)
