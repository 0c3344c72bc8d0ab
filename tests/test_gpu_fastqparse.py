"""GPU: FASTQ text parsed on the device (bbk_fastq_input_*, bbk_hreads_from_fastq_input, bbk_corrected_print_resident,
csrc/fastqparse.hip).  Every comparison is an equality with the restatement of the host reader and of the strict index
(tests/fastq_restated.py), or with the batch bbk_hreads_from_host makes of the restatement's records."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import fastq_restated as F
from tests import readcorrect_restated as R
from tests.hreads_child import device_set

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # BBK_ERR_ARG of include/bbk.h


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def split(blob, off):
    blob = blob.tobytes()
    return [blob[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def fields_of(hr, qvoffset=33):
    """the records of a batch as the reader gives them: (name, seq, qual) bytes"""
    b, q, off, names, noff = hr.records()
    assert int(off[0]) == 0 and int(noff[0]) == 0 and int(off[-1]) == len(b) == len(q) and int(noff[-1]) == len(names)
    return list(zip(split(names, noff), split(b, off), split((q + np.uint8(qvoffset)).astype(np.uint8), off)))


def host_batch(ctx, recs, k, qvoffset=33, tq=4):
    """Context.hammer_reads on the reader's records"""
    bases = np.frombuffer(b"".join(s for _, s, _ in recs), dtype=np.uint8)
    quals = np.frombuffer(b"".join(q for _, _, q in recs), dtype=np.uint8) - np.uint8(qvoffset)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    if recs:
        off[1:] = np.cumsum([len(s) for _, s, _ in recs], dtype=np.uint64)
    return ctx.hammer_reads(bases, quals, off, k, trim_quality=tq)


def tables(hr):
    return [hr.trims(), hr.candidates()] + [x for t in ("kmer", "corrector") for x in hr.stretches(t)]


def check_range(ctx, inp, first, n, k, want, qvoffset=33):
    """records [first, first + n) of the index as a batch: the records are the reader's, and trims, flags and both stretch
    tables are those of the batch made from host arrays"""
    hr = inp.hammer_reads(first, n, k)
    assert len(hr) == n and fields_of(hr, qvoffset) == want
    ref = host_batch(ctx, want, k, qvoffset)
    for a, b in zip(tables(hr), tables(ref)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    hr.free()
    ref.free()


def check_index(ctx, text, final=True, qvoffset=33, k=21, batch=True):
    """the index of one chunk against the restated strict index, and its usable records against the reader's"""
    ix = F.StrictIndex(text, final=final, qvoffset=qvoffset)
    inp = ctx.fastq_input(text, final=final, qvoffset=qvoffset)
    assert inp.records == ix.n and inp.verdict() == ix.verdict
    for n in sorted({0, min(1, ix.n), ix.usable, ix.n}):
        assert inp.text_end(n) == ix.text_end(n), n
    if batch:
        want = F.records(text)[:ix.usable]
        assert want == ix.recs(0, ix.usable)
        check_range(ctx, inp, 0, ix.usable, k, want, qvoffset)
    return inp, ix


class DeviceIndex:
    """the index of a chunk in the shape tests/fastq_restated.walk reads"""

    def __init__(self, ctx, data, final, k=21):
        self.inp, self.k = ctx.fastq_input(data, final=final), k
        self.n, self.verdict = self.inp.records, self.inp.verdict()
        self.usable = self.n if self.verdict is None else self.verdict[0]

    def text_end(self, n):
        return self.inp.text_end(n)

    def recs(self, first, n):
        hr = self.inp.hammer_reads(first, n, self.k)
        out = fields_of(hr)
        hr.free()
        return out


# ---- crafted records -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 21])
@pytest.mark.parametrize("last_line_feed", [True, False])
def test_crafted_records(ctx, k, last_line_feed):
    text = F.crafted_text()
    inp, ix = check_index(ctx, text if last_line_feed else text[:-1], k=k)
    assert ix.verdict is None and ix.n == len(F.crafted_records())
    got = dict(zip((label for label, _ in F.crafted_records()), DeviceIndex(ctx, text, True, k).recs(0, ix.n)))
    assert got["lower"][1].isupper() and got["nN."][1] == b"ACGTNNN..ACGT" * 5
    assert got["no name"][0] == b"" and got["blank name"][0] == b"read 1 with  blanks\tand a tab"
    assert got["lone cr fields"][:2] == (b"\r", b"\r") and got["x cr"][:2] == (b"x", b"A") and got["two cr"][:2] == (b"two\r", b"AC\r")
    assert got["crlf"][0] == b"crlf rec" and len(got["crlf"][1]) == 64
    assert [len(got["len%d" % n][1]) for n in F.SEQ_LENGTHS] == list(F.SEQ_LENGTHS)
    inp.free()


def test_qualities_at_the_ends_of_both_offsets(ctx):
    for qv in (33, 64):
        text = F.crafted_text(qv)
        inp, ix = check_index(ctx, text, qvoffset=qv)
        assert ix.verdict is None
        _, q, _, _, _ = inp.hammer_reads(0, ix.n, 21).records()
        assert int(q.min()) == 0 and int(q.max()) == 93


def test_a_chunk_that_is_not_final_cut_after_every_line(ctx):
    text = F.crafted_text()
    last = F.crafted_records()[-1][1]
    n = len(F.crafted_records())
    body = len(text) - len(last)
    cuts = [body + i + 1 for i, c in enumerate(last) if c == 0x0A]  # behind every line of the last record
    assert len(cuts) == 4
    for j, cut in enumerate(cuts):
        inp, ix = check_index(ctx, text[:cut], final=False)
        assert inp.records == (n if j == 3 else n - 1) and inp.verdict() is None
        assert inp.text_end(inp.records) == (len(text) if j == 3 else body)
        # one byte further, inside a line: the line does not count
        inp2, _ = check_index(ctx, text[:cut - 2], final=False, batch=False)
        assert inp2.records == n - 1 and inp2.text_end(n - 1) == body
    for empty in (b"", b"@only a header"):
        inp, ix = check_index(ctx, empty, final=False)
        assert inp.records == 0 and inp.verdict() is None and inp.text_end(0) == 0


# ---- every line start across the tile boundaries of the index kernels -----------------------------------------------
def test_boundary_sweep(ctx):
    rest = F.crafted_text()
    want_rest = F.records(rest)
    for pad in list(range(131)) + [1023, 1024, 1025, 4095, 4096, 4097]:
        name = b"p" * pad
        text = F.fq(name, "ACGTACGTAC") + rest
        inp = ctx.fastq_input(text)
        assert inp.records == len(want_rest) + 1 and inp.verdict() is None, pad
        hr = inp.hammer_reads(0, inp.records, 21)
        assert fields_of(hr) == [(name, b"ACGTACGTAC", b"I" * 10)] + want_rest, pad
        hr.free()
        inp.free()


def test_a_line_feed_on_either_side_of_a_tile_edge(ctx):
    for tile in (1024, 4096):
        for at in (tile - 1, tile):  # the header's line feed is the last byte of a tile / the first byte of the next
            text = F.fq(b"n" * (at - 1), "ACGT") + F.crafted_text()
            assert text[at] == 0x0A
            check_index(ctx, text)


# ---- verdicts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", F.FORM_DAMAGE)
def test_form_verdicts(ctx, kind):
    good, rng = F.crafted_text(), random.Random(3)
    n = len(F.crafted_records())
    text = good + F.damaged(kind, rng) + good
    inp, ix = check_index(ctx, text)
    assert inp.verdict() == (n, F.FORM, -1)
    # the reader takes over between records: it yields everything behind the usable ones
    assert F.records(text)[:n] + F.records(text, inp.text_end(n)) == F.records(text)
    with pytest.raises(B.BBKError) as e:
        inp.hammer_reads(0, n + 1, 21)
    assert "error %d" % ERR_ARG in str(e.value)


@pytest.mark.parametrize("qv", [33, 64])
def test_quality_verdicts(ctx, qv):
    good, rng = F.crafted_text(qv), random.Random(4)
    n = len(F.crafted_records(qv))
    for kind, byte in (("quality below", qv - 1), ("quality above", qv + 94)):
        inp, ix = check_index(ctx, good + F.damaged(kind, rng, qv) + good, qvoffset=qv)
        assert inp.verdict() == (n, F.QUALITY, byte)
    # the same bytes are fine under the other offset's range when they fall inside it
    inp, ix = check_index(ctx, F.fq("q", "ACGT", qual=bytes([qv - 1, qv, qv + 93, qv + 94])), qvoffset=qv)
    assert inp.verdict() == (0, F.QUALITY, qv - 1)


def test_leftover_lines_and_the_smallest_verdict(ctx):
    good, rng = F.crafted_text(), random.Random(6)
    n = len(F.crafted_records())
    for extra in (b"@left over", b"@left over\nACGT\n", b"@left over\nACGT\n+\n", b"\n"):
        inp, ix = check_index(ctx, good + extra)
        assert inp.verdict() == (n, F.FORM, -1) and inp.records == n
        inp, ix = check_index(ctx, good + extra, final=False)
        assert inp.verdict() is None and inp.records == n
    # several in one text: the smallest record wins, whatever its kind
    for order in (("quality above", "fasta", "blank line"), ("two-line sequence", "quality below", "missing plus")):
        text = good + b"".join(F.damaged(kind, rng) + good for kind in order)
        inp, ix = check_index(ctx, text)
        assert inp.verdict()[:2] == (n, F.QUALITY if order[0].startswith("quality") else F.FORM)
    many = b"".join(F.damaged(rng.choice(F.FORM_DAMAGE + F.QUALITY_DAMAGE), rng) for _ in range(300))
    check_index(ctx, good * 3 + many, batch=False)


# ---- fuzz ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuzz():
    return {seed: (text, F.records(text)) for seed in (1, 2, 3) for text in (F.fuzz_text(seed),)}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("chunk", [1000, 4096, 100000])
def test_fuzz_in_chunks(ctx, fuzz, seed, chunk):
    text, want = fuzz[seed]
    got, bad = F.walk(text, lambda d, f: DeviceIndex(ctx, d, f), chunk)
    assert len(got) == len(want) == 2000 and got == want
    assert bad and [b for _, b in bad] == [next(c for c in want[i][2] if not 33 <= c <= 126) for i, _ in bad]


# ---- sub-ranges and the block rule -----------------------------------------------------------------------------------
def test_sub_ranges_and_the_block_rule(ctx):
    rng = random.Random(8)
    good = F.crafted_text()
    text = good + good + F.damaged("fasta", rng) + good
    inp, ix = check_index(ctx, text)
    want = F.records(text)
    u = ix.usable
    assert u == 2 * len(F.crafted_records())
    for first, n in ((0, 0), (u, 0), (0, 1), (1, 1), (5, 17), (u - 1, 1), (9, u - 9)):
        check_range(ctx, inp, first, n, 21, want[first:first + n])
    for first in (0, 1, 8, u - 1, u, u + 1):
        for max_bases in (0, 1, 64, 65, 1000, 1001, 2500, 10 ** 12, 2 ** 64 - 1):
            assert inp.records_within(first, max_bases) == ix.records_within(first, max_bases), (first, max_bases)
    for first, n in ((0, u + 1), (u, 1), (u + 1, 0)):
        with pytest.raises(B.BBKError) as e:
            inp.hammer_reads(first, n, 21)
        assert "error %d" % ERR_ARG in str(e.value)
    for k in (0, 33):
        with pytest.raises(B.BBKError) as e:
            inp.hammer_reads(0, 1, k)
        assert "error %d" % ERR_ARG in str(e.value)
    with pytest.raises(B.BBKError):
        ctx.fastq_input(good, qvoffset=163)
    with pytest.raises(ValueError):
        inp.text_end(inp.records + 1)


def test_the_same_bytes_on_every_run(ctx):
    text, _ = F.fuzz_text(2, n=400, damage=0), None
    runs = []
    for _ in range(2):
        inp = ctx.fastq_input(text)
        hr = inp.hammer_reads(0, inp.records, 21)
        runs.append([x.tobytes() for x in hr.records()] + [x.tobytes() for x in tables(hr)])
        hr.free()
        inp.free()
    assert runs[0] == runs[1]


# ---- the printer with resident names ---------------------------------------------------------------------------------
def pair_texts(k=21):
    """(keys, good, left text, right text): pairs with every combination of good and bad mates, the mates of different
    lengths, names of 0 to 70 bytes, trims on both sides"""
    g, other = R.genome(300, 91, k), R.genome(200, 92, k)
    _, keys, good = R.make_index(R.kmers_of(g, k))
    sides = ([], [])
    flags = [(1, 1), (0, 1), (1, 0), (0, 0), (1, 0), (0, 1), (0, 0), (1, 1), (0, 1), (1, 1), (0, 0), (1, 0)]
    for i, pair in enumerate(flags):
        for side, ok in enumerate(pair):
            n = 60 + 7 * i + 3 * side
            seq = (g if ok else other)[i:i + n]
            if ok and i % 3 == 0:  # a substitution of low quality behind a clean island: corrected
                p = 40
                seq = seq[:p] + R.NUCL[(R.NUCL.index(seq[p]) + 1) % 4] + seq[p + 1:]
            qual = bytes([33 + 30] * n)
            if ok and i % 3 == 0:
                qual = qual[:40] + bytes([33 + 10]) + qual[41:]
            if i % 4 == 1:  # bad ends: trimmed on both sides
                seq, qual = "N" * i + seq + "N", bytes([35] * i) + qual + bytes([35])
            sides[side].append(F.fq("x" * (6 * i) + ("/%d" % (side + 1) if i else ""), seq, qual=qual))
    return keys, good, b"".join(sides[0]), b"".join(sides[1])


@pytest.mark.parametrize("tags", [False, True])
def test_print_resident_equals_print_with_exported_names(ctx, tags):
    k = 21
    keys, good, lt, rt = pair_texts(k)
    s = device_set(ctx, keys, k)
    c = s.corrector(good)
    batches = []
    for text in (lt, rt):
        inp = ctx.fastq_input(text)
        assert inp.verdict() is None and inp.records == 12
        hr = inp.hammer_reads(0, 12, k)
        inp.free()  # the batch does not borrow the index
        batches.append((hr, c.correct_resident(hr)))
    names = [split(*hr.records()[3:]) for hr, _ in batches]
    assert names[0][0] == b"" and names[1][11] == b"x" * 66 + b"/2"
    (hl, cl), (hrr, crr) = batches
    for mate, mate_names in ((None, None), (crr, names[1])):
        res, ref = cl.print_resident(mate=mate, tags=tags), cl.print(names[0], tags=tags, mate=mate, mate_names=mate_names)
        assert res.sizes == ref.sizes and len(res.sizes) == (5 if mate is not None else 2)
        assert all(res.stream(i) == ref.stream(i) for i in range(len(res.sizes)))
        assert sum(1 for x in res.sizes if x) >= 2
        if tags:
            flat = b"".join(res.stream(i) for i in range(len(res.sizes)))
            assert b" BH:ok" in flat and b"ltrim=" in flat
    # a batch made from host arrays holds no names
    plain = host_batch(ctx, F.records(lt), k)
    cp = c.correct_resident(plain)
    assert len(plain.records()[3]) == 0 and not plain.records()[4].any()
    for left, mate in ((cp, None), (cl, cp), (cp, crr)):
        with pytest.raises(B.BBKError) as e:
            left.print_resident(mate=mate)
        assert "error %d" % ERR_ARG in str(e.value) and "no names" in str(e.value)


# ---- spades-kmerdata --device-parse on the golden pair ---------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTPUTS = ("0.cor.fastq", "1.cor.fastq", "0.unpaired.fastq", "0.bad.fastq", "1.bad.fastq", "kmers", "kmstat")


def run_tool(out, files, extra=()):
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    args = ["-o", str(out), "-k", "21", "-b", "30000", "--correct", "--paired", "--correct-stats"] + list(extra) + list(files)
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)


def outputs(prefix):
    return [open("%s.%s" % (prefix, name), "rb").read() for name in OUTPUTS]


@pytest.fixture(scope="module")
def golden_pair():
    return [os.path.join(GOLDEN, "ecoli_1K_%d.fq.gz" % i) for i in (1, 2)]


@pytest.fixture(scope="module")
def host_parsed(golden_pair, tmp_path_factory):
    """what the tool writes without the option, every pass parsing the input"""
    prefix = tmp_path_factory.mktemp("fastqparse_cli") / "host"
    r = run_tool(prefix, golden_pair)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (r.stdout + r.stderr).count("Prepared batch") >= 3
    out = outputs(prefix)
    assert out[0] and out[1] and out[5] and out[6], [len(x) for x in out]  # (the pair is clean: nothing unpaired or bad)
    return out


@pytest.mark.parametrize("extra", [("--resident-bytes", "300000"), ("--resident-bytes", "100000000"),
                                   ("--device-parse",), ("--device-parse", "--resident-bytes", "300000", "--parse-chunk", "100000"),
                                   ("--device-parse", "--resident-bytes", "100000000"), ("--device-parse", "--parse-chunk", "5000")],
                         ids=" ".join)
def test_cli_writes_the_same_files(golden_pair, host_parsed, tmp_path, extra):
    r = run_tool(tmp_path / "out", golden_pair, extra)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "the serial reader goes on" not in r.stdout + r.stderr  # the golden pair is in the four-line form throughout
    for name, got, want in zip(OUTPUTS, outputs(tmp_path / "out"), host_parsed):
        assert got == want, name


def test_cli_falls_back_at_a_two_line_record(golden_pair, tmp_path):
    text = gzip.open(golden_pair[0]).read()
    recs = F.records(text)
    m = len(recs) // 2
    name, seq, qual = recs[m]
    cut = F.StrictIndex(text)
    a, b = cut.text_end(m), cut.text_end(m + 1)
    h = len(seq) // 2
    two = b"@" + name + b"\n" + seq[:h] + b"\n" + seq[h:] + b"\n+\n" + qual + b"\n"
    left = tmp_path / "left.fq"
    left.write_bytes(text[:a] + two + text[b:])
    assert F.records(left.read_bytes()) == recs and F.StrictIndex(left.read_bytes()).verdict == (m, F.FORM, -1)
    files = [str(left), golden_pair[1]]
    runs = {}
    for label, extra in (("host", ()), ("device", ("--device-parse",)), ("chunks", ("--device-parse", "--parse-chunk", "70000",
                                                                                     "--resident-bytes", "300000"))):
        r = run_tool(tmp_path / label, files, extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("the serial reader goes on" in r.stdout + r.stderr) == (label != "host")
        runs[label] = outputs(tmp_path / label)
    assert runs["device"] == runs["host"] and runs["chunks"] == runs["host"]


def test_cli_refuses_a_bad_quality_the_same_way(golden_pair, tmp_path):
    text = bytearray(gzip.open(golden_pair[1]).read())
    cut = F.StrictIndex(bytes(text))
    m = 1500
    text[cut.text_end(m + 1) - 10] = 0x20  # a blank in the quality line of record m of the right file
    right = tmp_path / "right.fq"
    right.write_bytes(bytes(text))
    seen = []
    for extra in ((), ("--device-parse",)):
        r = run_tool(tmp_path / "out", [golden_pair[0], str(right)], extra)
        line = [x for x in r.stderr.split("\n") if "quality character" in x]
        assert r.returncode != 0 and len(line) == 1 and "record %d " % m in line[0], r.stderr
        seen.append((r.returncode, line[0]))
    assert seen[0] == seen[1]
