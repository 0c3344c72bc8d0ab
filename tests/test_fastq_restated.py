"""CPU: the restatement of the host FASTQ reader (tests/fastq_restated.py) against the real one (bbk-fastx-dump --records over
host/fastx.hpp), and the strict four-line index against the restatement: before its verdict the index yields exactly the
reader's records, and from text_end of the verdict's record the reader yields the rest.  No GPU."""
import gzip
import os
import random
import subprocess

import pytest

from spades_for_blackbird_amd import build_host
from tests import fastq_restated as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecoli_1K_1.fq.gz")


@pytest.fixture(scope="module")
def dump():
    return [e for e in build_host.build() if e.endswith("bbk-fastx-dump")][0]


def dumped(exe, path):
    """the records bbk-fastx-dump --records prints for the file"""
    r = subprocess.run([exe, "--records", str(path)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out, fields, p = r.stdout, [], 0
    while p < len(out):
        sp = out.index(b" ", p)
        n = int(out[p:sp])
        fields.append(out[sp + 1:sp + 1 + n])
        assert out[sp + 1 + n:sp + 2 + n] == b"\n"
        p = sp + 2 + n
    assert len(fields) % 3 == 0
    return [tuple(fields[i:i + 3]) for i in range(0, len(fields), 3)]


def edge_texts():
    """[(label, text)]: what the state machine does at the ends of a stream and around records that are not four lines"""
    rng = random.Random(11)
    good = F.crafted_text()
    out = [("empty", b""), ("crafted", good), ("crafted, no last line feed", good[:-1]),
           ("only line feeds", b"\n\n\n"), ("junk before the first header", b"junk\nmore\n" + good),
           ("header is the last byte", good + b"@"), ("header line without a line feed", good + b"@tail"),
           ("header only", good + b"@tail\n"), ("no plus line at the end", good + b"@t\nACGT\n"),
           ("plus line at EOF", good + b"@t\nACGT\n+"), ("plus line, then EOF", good + b"@t\nACGT\n+\n"),
           ("truncated quality at EOF", good + b"@t\nACGT\n+\nII"), ("quality without a line feed", good + b"@t\nACGT\n+\nIIII"),
           ("quality over two lines", b"@t\nACGT\n+\nII\nII\n" + good), ("quality over two lines, too long", b"@t\nACGT\n+\nII\nIII\n" + good),
           ("crlf empty record", F.fq("e", "", eol=b"\r\n") + good), ("cr only line ends", good.replace(b"\n", b"\r")),
           ("fasta then fastq", b">f one\nACGT\nacgt\n" + good), ("fasta at the end", good + b">f\nAC\n"),
           ("fasta header at the end", good + b">f\n")]
    for kind in F.FORM_DAMAGE + F.QUALITY_DAMAGE:
        out.append((kind, good + F.damaged(kind, rng) + good))
    out.append(("several", good + b"".join(F.damaged(k, rng) + good for k in F.FUZZ_DAMAGE)))
    return out


def texts():
    return edge_texts() + [("fuzz %d" % s, F.fuzz_text(s)) for s in (1, 2, 3)] + [("golden", gzip.open(GOLDEN).read())]


def test_the_restatement_is_the_host_reader(dump, tmp_path):
    for i, (label, text) in enumerate(texts()):
        p = tmp_path / ("t%d.fq" % i)
        p.write_bytes(text)
        assert F.records(text) == dumped(dump, p), label
    assert dumped(dump, GOLDEN) == F.records(gzip.open(GOLDEN).read())  # through zlib as well


@pytest.mark.parametrize("final", [True, False])
def test_the_strict_index_against_the_restatement(final):
    for label, text in texts():
        want = F.records(text)
        ix = F.StrictIndex(text, final=final)
        assert ix.recs(0, ix.usable) == want[:ix.usable], label
        if ix.verdict is None:
            if final:
                assert ix.usable == len(want), label
            continue
        r, kind, byte = ix.verdict
        rest = F.records(text, ix.text_end(r))
        if kind == F.QUALITY:  # the reader takes the record; its caller refuses it for this byte
            assert byte == next(c for c in rest[0][2] if not 33 <= c <= 33 + F.MAX_QUAL), label
        if final or kind == F.QUALITY:  # (not final: the chunk's end may have cut the verdict's record)
            assert want[:r] + rest == want, label


def test_the_walk_over_chunks():
    for label, text in texts():
        want = F.records(text)
        for chunk in (7, 1000, 4096, 100000):
            if chunk == 7 and len(text) > 20000:
                continue
            got, bad = F.walk(text, lambda d, f: F.StrictIndex(d, f), chunk)
            assert got == want, (label, chunk)
            assert [b for _, b in bad] == [next(c for c in want[i][2] if not 33 <= c <= 126) for i, _ in bad], (label, chunk)


def test_the_golden_file_is_strict():
    text = gzip.open(GOLDEN).read()
    ix = F.StrictIndex(text)
    assert ix.verdict is None and ix.n == 2054 and ix.recs(0, ix.n) == F.records(text)


def test_the_block_rule():
    text = F.crafted_text()
    ix, recs = F.StrictIndex(text), F.records(text)
    for first in (0, 3, len(recs) - 1, len(recs)):
        for max_bases in (0, 1, 64, 65, 700, 10 ** 9):
            n, bases = 0, 0  # ReadSource::parse: take a record, then close the block when the bases have reached -b
            for _, seq, _ in recs[first:]:
                n, bases = n + 1, bases + len(seq)
                if bases >= max_bases:
                    break
            assert ix.records_within(first, max_bases) == n, (first, max_bases)
