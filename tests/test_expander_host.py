"""CPU: the host side of the expansion (host/hammer_reads.hpp: expander_candidate, through bbk-hammer-reads-dump
--expander) against the restated candidate rule (tests/expander_restated.py), on the crafted reads and on a real FASTQ
file; the same program under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone host program; and the default
mode, which shares the trimming and the generator with the new one, against the output of the commit before it."""
import gzip
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import expander_restated as E
from tests import kmerdata_restated as KR

KS = [10, 11, 21, 22, 32]

# md5 of what `bbk-hammer-reads-dump <args> ecoli_1K_1.fq.gz [ecoli_1K_2.fq.gz]` printed before --expander existed
PARENT_MD5 = [
    (["-k", "21"], (1, 2), "5ecba7209de964d7b5994cd2e5982f21"),
    (["-k", "32"], (1, 2), "d9420fbb473ca1da323389b19d945f82"),
    (["--trim-quality", "7", "-k", "21"], (1,), "43c96c8df3d6958a65b9670398eecab0"),
]


@pytest.fixture(scope="module")
def dump_exe():
    from spades_for_blackbird_amd import build_host
    return [e for e in build_host.build() if e.endswith("bbk-hammer-reads-dump")][0]


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [tuple(int(x) for x in line.split()) for line in r.stdout.split("\n")[:-1]]


def _write_fastq(path, reads, offset=33):
    with open(path, "w") as f:
        for i, (seq, qual) in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, seq, "".join(chr(q + offset) for q in qual)))


def _crafted(k):
    return [(s, q) for _, s, q in KR.crafted_reads(k, np.random.default_rng(100 + k))]


@pytest.mark.parametrize("k", KS)
def test_crafted_reads(dump_exe, tmp_path, k):
    reads = _crafted(k)
    exp = E.candidates(reads, k)
    assert len(exp) == 4
    p = str(tmp_path / "c.fq")
    _write_fastq(p, reads)
    assert _run(dump_exe, ["-k", str(k), "--expander", p]) == exp
    assert _run(dump_exe, ["--expander", "-k", str(k), p]) == exp  # the flag takes no value, wherever it stands
    # another offset and another trimming threshold
    _write_fastq(p, reads, offset=64)
    assert _run(dump_exe, ["-k", str(k), "--qvoffset", "64", "--expander", p]) == exp
    exp2 = E.candidates(reads, k, 2)
    assert exp2 != exp
    assert _run(dump_exe, ["-k", str(k), "--qvoffset", "64", "--trim-quality", "2", "--expander", p]) == exp2


def test_real_fastq(dump_exe, golden_dir):
    path = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    with gzip.open(path, "rt") as f:
        lines = f.read().split("\n")
    reads = [(lines[i + 1], [ord(c) - 33 for c in lines[i + 3]]) for i in range(0, len(lines) - 3, 4)]
    exp = E.candidates(reads, 21)
    assert len(exp) == 2054 and sum(1 for _, _, n in exp if n < 100) > 500
    assert _run(dump_exe, ["--expander", path]) == exp  # k = 21 is the default
    exp32 = E.candidates(reads, 32)
    assert 0 < len(exp32) < 2054  # some reads keep fewer than 32 bases
    assert _run(dump_exe, ["-k", "32", "--expander", path]) == exp32


def test_default_mode_prints_what_it_printed(dump_exe, golden_dir):
    for args, files, md5 in PARENT_MD5:
        r = subprocess.run([dump_exe] + args + [os.path.join(golden_dir, "ecoli_1K_%d.fq.gz" % f) for f in files],
                           capture_output=True)
        assert r.returncode == 0, r.stderr
        assert hashlib.md5(r.stdout).hexdigest() == md5, args


def test_header_under_sanitizers(tmp_path):
    from spades_for_blackbird_amd import build_host
    exe = build_host.build_sanitized(program="bbk-hammer-reads-dump")
    for k in KS:
        reads = _crafted(k) + [("", []), ("A", [40]), ("N", [40])]
        p = str(tmp_path / ("s%d.fq" % k))
        _write_fastq(p, reads)
        kept = [r for r in reads if r[0]]  # an empty record is no record for the reader
        assert _run(exe, ["-k", str(k), "--expander", p]) == E.candidates(kept, k)
        assert _run(exe, ["-k", str(k), "--trim-quality", "0", "--expander", p]) == E.candidates(kept, k, 0)
