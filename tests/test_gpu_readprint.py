"""GPU: the device FASTQ printer (bbk_corrector_correct_resident, bbk_corrected_*, bbk_fastq_text_*, csrc/readprint.hip) and
spades-kmerdata --correct --paired / --correct-stats / --output-dir against the restatement (tests/readprint_restated.py).
Every comparison is byte equality of each stream.  Sets are injected with kmerset_from_device, bits with
KMerSet.corrector(good)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import readcorrect_cases as Cs
from tests import readcorrect_restated as R
from tests import readprint_restated as P
from tests.hreads_child import arrays, device_set
from tests.readprint_child import overflow_batch, run_batch

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # BBK_ERR_ARG of include/bbk.h
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 21


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


# ---- cases ---------------------------------------------------------------------------------------------------------------
def shape_cases(k=K):
    """(index, keys, good, records): a genome of 400 bases whose k-mers are the good set, and records cut from it at the
    sizes where the kernels change their path"""
    g = R.genome(400, 77, k)
    index, keys, good = R.make_index(R.kmers_of(g, k))
    other = R.genome(120, 78, k)  # shares no k-mer with g (checked below)
    assert not set(R.kmers_of(other, k)) & set(index)
    recs = []

    def add(name, seq, qual=None, left=0, right=0):
        """left / right: that many N of quality 2 around the read: trimmed away when the rule says so"""
        qual = [30] * len(seq) if qual is None else qual
        recs.append((name, "N" * left + seq + "N" * right, [2] * left + list(qual) + [2] * right))

    add("n0", "")                                   # a record of 0 bases
    add("gone", "ACGTNACGTN" * 3, [2] * 30)         # trimmed to nothing
    for n in (1, k - 1, k, 63, 64, 65, 129, 300):   # trimmed lengths: fewer than k, exactly k, the wavefront's edges
        add("len%d" % n, g[7:7 + n])
    for n in (0, 1, 63, 64, 65, 200):               # names at the wavefront's edges of the copy loop
        add("x" * n, g[n:n + 70])
    for n in (9, 10, 99, 100):                      # the digit width changes: left trim only, right trim only
        add("lt%d" % n, g[n:n + 66], left=n)
        add("rt%d" % n, g[n:n + 66], right=n)
    add("both", g[30:130], left=9, right=100)       # both trims: the tail is more than twice the left trim
    add("kept", g[30:130], left=10, right=9)        # a bad tail that the left trim keeps (read.hpp:101-114)
    add("nosolid", other[:80])                      # k bases and more, no good k-mer: no tag
    # the last base wrong at quality 30: searched, kept as it is -- failed
    add("failed", g[100:180] + R.NUCL[(R.NUCL.index(g[180]) + 1) % 4])
    for n in (9, 10):                               # n substitutions of quality 10, 20 bases apart, behind a clean island
        s, q = list(g[20:320]), [30] * 300
        for j in range(n):
            p = 60 + 20 * j
            s[p] = R.NUCL[(R.NUCL.index(s[p]) + 2) % 4]
            q[p] = 10
        add("changed%d" % n, "".join(s), q)
    return index, keys, good, recs


def pair_cases(k=K):
    """(index, keys, good, left, right): every (left, right) flag combination three times, in mixed order"""
    g = R.genome(300, 91, k)
    other = R.genome(200, 92, k)
    index, keys, good = R.make_index(R.kmers_of(g, k))
    left, right = [], []
    for i, (lgood, rgood) in enumerate([(1, 1), (0, 1), (1, 0), (0, 0), (1, 0), (0, 1), (0, 0), (1, 1), (0, 1), (1, 1), (0, 0), (1, 0)]):
        for side, ok, recs in (("1", lgood, left), ("2", rgood, right)):
            n = 60 + 7 * i + (3 if side == "2" else 0)  # the mates differ in length
            seq = (g if ok else other)[i:i + n]
            recs.append(("pair%d/%s" % (i, side), seq, [30] * n))
    return index, keys, good, left, right


def expected(index, good, left, right=None, tags=True, qvoffset=33, k=K):
    """(streams as bytes, the restatement's rows per side, its corrector)"""
    rc = R.ReadCorrector(index, good, k)
    rows = [P.corrected_records(rc, recs, 4, tags, qvoffset) for recs in (left, right) if recs is not None]
    streams = P.route_single(rows[0]) if right is None else P.route_paired(rows[0], rows[1])
    return [s.encode("latin-1") for s in streams], rows, rc


def check(ctx, index, keys, good, left, right=None, tags=True, qvoffset=33, k=K):
    want, rows, rc = expected(index, good, left, right, tags, qvoffset, k)
    got = run_batch(ctx, k, keys, good, left, right, tags=tags, qvoffset=qvoffset)
    for i, (g, w) in enumerate(zip(got["streams"], want)):
        assert g == w, (i, len(g), len(w), next((j, g[j:j + 40], w[j:j + 40]) for j in range(max(len(g), len(w))) if g[j:j + 1] != w[j:j + 1]))
    assert len(got["streams"]) == len(want) and got["sizes"] == [len(w) for w in want]
    for side, r in zip(got["sides"], rows):
        assert side[2] == [int(x[0]) for x in r]                       # the flags
        assert side[4] == [x[3] for x in r] and side[5] == [x[2] for x in r]  # changed, tag kind
    assert [got["stats"][x] for x in B.Corrector.STATS[:4]] == rc.stats()
    return got, rows, rc


@pytest.fixture(scope="module")
def shapes():
    return shape_cases()


# ---- tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tags,qvoffset", [(True, 33), (False, 33), (True, 64)])
def test_shapes(ctx, shapes, tags, qvoffset):
    index, keys, good, recs = shapes
    got, rows, rc = check(ctx, index, keys, good, recs, tags=tags, qvoffset=qvoffset)
    kinds = [x[2] for x in rows[0]]
    assert set(kinds) == {P.NONE, P.OK, P.FAILED, P.CHANGED}
    assert {x[3] for x in rows[0] if x[2] == P.CHANGED} == {9, 10}
    by = {r[0]: x for r, x in zip(recs, rows[0])}
    assert by["kept"][1].count("ltrim=10") == 1 and "rtrim" not in by["kept"][1]
    assert " ltrim=9 rtrim=100\n" in by["both"][1]
    assert got["sizes"][0] > 0 and got["sizes"][1] > 0
    if not tags:  # what the host path printed before: Read::print of the corrected trimmed read, the name untouched
        flat = "".join(x[1] for x in rows[0])
        assert "BH:" not in flat
        rc2 = R.ReadCorrector(index, good, K)
        for (name, seq, qual), x in zip(recs, rows[0]):
            s, q, lt, rt, initial = R.trim_read(seq, list(qual), 4)
            out, _ = rc2.correct_batch([(s, q)])
            assert x[1] == R.read_print(name, out[0], q, lt, rt, initial, qvoffset), name


def test_empty_batch(ctx, shapes):
    index, keys, good, _ = shapes
    got, _, _ = check(ctx, index, keys, good, [])
    assert got["streams"] == [b"", b""]
    got, _, _ = check(ctx, index, keys, good, [], [])
    assert got["streams"] == [b""] * 5


def test_pairs(ctx):
    index, keys, good, left, right = pair_cases()
    got, rows, _ = check(ctx, index, keys, good, left, right)
    flags = {(l[0], r[0]) for l, r in zip(*rows)}
    assert flags == {(True, True), (True, False), (False, True), (False, False)}
    assert all(s.count(b"\n") >= 8 for s in got["streams"])  # two records or more in every stream
    assert sum(got["sizes"]) == sum(len(x[1]) for side in rows for x in side)
    # the unpaired stream keeps the order (pair, left before right)
    names = [line[1:].split(b" ")[0] for line in got["streams"][2].split(b"\n")[0::4] if line]
    order = [(int(n[4:].split(b"/")[0]), n[-1:]) for n in names]
    assert order == sorted(order) and {o[1] for o in order} == {b"1", b"2"}


def test_pairs_without_a_good_mate(ctx):
    """no pair and no single good mate: the cor and unpaired streams are empty"""
    index, keys, good, left, right = pair_cases()
    bad_l = [r for r, ok in zip(left, [x[0] for x in expected(index, good, left)[1][0]]) if not ok]
    bad_r = [r for r, ok in zip(right, [x[0] for x in expected(index, good, right)[1][0]]) if not ok]
    n = min(len(bad_l), len(bad_r))
    assert n >= 2
    got, _, _ = check(ctx, index, keys, good, bad_l[:n], bad_r[:n])
    assert got["sizes"][:3] == [0, 0, 0] and got["sizes"][3] > 0 and got["sizes"][4] > 0


def test_host_rule(ctx, tmp_path):
    """the overflow batch: on the device path two searches go through the host rule; in a child process under
    BBK_CORRECTOR_HOST=1 all of them do -- the resident result and the text are the same"""
    index, keys, good, records = overflow_batch(K)
    want, rows, rc = expected(index, good, records)
    got = run_batch(ctx, K, keys, good, records, tags=True, prepared=True)
    assert got["streams"] == want
    s = device_set(ctx, keys, K)
    c = s.corrector(good)
    limits = c.limits()
    c.free()
    s.free()
    beyond = {r for r, _, inf in rc.searches if inf.max_heap > limits[0] or inf.pops > limits[1]}
    searched = {r for r, _, _ in rc.searches}
    assert got["sides"][0][3] == [2 if r in beyond else 1 if r in searched else 0 for r in range(len(records))]
    assert beyond and searched - beyond
    out = str(tmp_path / "host.pkl")
    env = dict(os.environ, BBK_CORRECTOR_HOST="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "readprint_child.py"), out], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out, "rb") as f:
        host = pickle.load(f)
    assert host["streams"] == got["streams"] and host["sizes"] == got["sizes"]
    for i in (0, 1, 2, 4, 5):  # bases, offsets, flags, changed, tags
        assert host["sides"][0][i] == got["sides"][0][i], i
    assert host["sides"][0][3] == [2 if r in searched else 0 for r in range(len(records))]
    assert {x: host["stats"][x] for x in B.Corrector.STATS[:4]} == {x: got["stats"][x] for x in B.Corrector.STATS[:4]}


def test_batching(ctx, shapes, tmp_path):
    """one batch, and the same records in three batches appended to the same files: the same bytes"""
    index, keys, good, recs = shapes
    want, _, _ = expected(index, good, recs)
    s = device_set(ctx, keys, K)
    c = s.corrector(good)
    for tag, parts in (("one", [recs]), ("three", [recs[:1], recs[1:17], recs[17:]])):
        for j, part in enumerate(parts):
            hr = ctx.hammer_reads(*arrays([(seq, qual) for _, seq, qual in part]), K)
            cr = c.correct_resident(hr)
            text = cr.print([n for n, _, _ in part], tags=True)
            for i in (0, 1):
                text.write(i, str(tmp_path / ("%s.%d.fastq" % (tag, i))), append=j > 0)
            for x in (text, cr, hr):
                x.free()
    for i in (0, 1):
        one = open(str(tmp_path / ("one.%d.fastq" % i)), "rb").read()
        assert one == want[i] and one == open(str(tmp_path / ("three.%d.fastq" % i)), "rb").read()
    # append=False replaces what the file holds
    hr = ctx.hammer_reads(*arrays([(seq, qual) for _, seq, qual in recs[:3]]), K)
    cr = c.correct_resident(hr)
    text = cr.print([n for n, _, _ in recs[:3]], tags=True)
    p = str(tmp_path / "one.0.fastq")
    text.write(0, p)
    assert open(p, "rb").read() == text.stream(0) and len(text.stream(0)) < len(want[0])
    for x in (text, cr, hr, c, s):
        x.free()


def test_refusals(ctx, shapes):
    import ctypes as C
    index, keys, good, recs = shapes
    L = B.load_library()
    s = device_set(ctx, keys, K)
    c = s.corrector(good)
    part = recs[2:6]
    hr = ctx.hammer_reads(*arrays([(seq, qual) for _, seq, qual in part]), K)
    hr3 = ctx.hammer_reads(*arrays([(seq, qual) for _, seq, qual in part[:3]]), K)
    cr, cr3 = c.correct_resident(hr), c.correct_resident(hr3)
    names = [n for n, _, _ in part]

    def refused(fn, match):
        with pytest.raises(B.BBKError, match=match) as err:
            fn()
        assert "bbk error %d:" % ERR_ARG in str(err.value)

    h = C.c_void_p()
    off = np.arange(5, dtype=np.uint64)
    blob = np.frombuffer(b"abcd", dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    # NULL arguments
    assert L.bbk_corrector_correct_resident(None, hr._h, C.byref(h)) == ERR_ARG
    assert L.bbk_corrector_correct_resident(c._h, None, C.byref(h)) == ERR_ARG
    assert L.bbk_corrector_correct_resident(c._h, hr._h, None) == ERR_ARG
    assert L.bbk_corrected_export(None, cr._h, None, None, None, None, None, None) == ERR_ARG
    assert L.bbk_corrected_export(ctx._h, None, None, None, None, None, None, None) == ERR_ARG
    assert L.bbk_corrected_print(None, None, vp(blob), vp(off), None, None, 33, 0, C.byref(h)) == ERR_ARG
    assert L.bbk_corrected_print(cr._h, None, vp(blob), None, None, None, 33, 0, C.byref(h)) == ERR_ARG
    assert L.bbk_corrected_print(cr._h, None, None, vp(off), None, None, 33, 0, C.byref(h)) == ERR_ARG  # names of 4 bytes
    assert L.bbk_corrected_print(cr._h, cr._h, vp(blob), vp(off), vp(blob), None, 33, 0, C.byref(h)) == ERR_ARG
    assert L.bbk_corrected_print(cr._h, None, vp(blob), vp(off), None, None, 33, 0, None) == ERR_ARG
    assert b"NULL argument" in L.bbk_last_error() and not h.value
    assert L.bbk_corrected_size(None) == 0 and L.bbk_fastq_text_streams(None) == 0 and L.bbk_fastq_text_size(None, 0) == 0
    # every pointer of export may be NULL
    assert L.bbk_corrected_export(ctx._h, cr._h, None, None, None, None, None, None) == 0
    # left and right of different sizes, of different contexts
    refused(lambda: cr.print(names, mate=cr3, mate_names=names[:3]), "4 left and 3 right")
    other = B.Context(0)
    s2 = device_set(other, keys, K)
    c2 = s2.corrector(good)
    hr2 = other.hammer_reads(*arrays([(seq, qual) for _, seq, qual in part]), K)
    cr2 = c2.correct_resident(hr2)
    refused(lambda: cr.print(names, mate=cr2, mate_names=names), "different contexts")
    refused(lambda: c.correct_resident(hr2), "another context")
    for x in (cr2, hr2, c2, s2):
        x.free()
    other.close()
    # names: descending offsets, a line feed inside a name
    bad = np.array([0, 3, 2, 4, 4], dtype=np.uint64)
    assert L.bbk_corrected_print(cr._h, None, vp(blob), vp(bad), None, None, 33, 0, C.byref(h)) == ERR_ARG
    assert b"descend" in L.bbk_last_error()
    assert L.bbk_corrected_print(cr._h, cr._h, vp(blob), vp(off), vp(blob), vp(bad), 33, 0, C.byref(h)) == ERR_ARG
    assert b"right name 1 descend" in L.bbk_last_error()
    refused(lambda: cr.print(["a", "b\nc", "d", "e"]), "line feed")
    with pytest.raises(ValueError):
        cr.print(names[:3])
    # the quality offset
    refused(lambda: cr.print(names, qvoffset=-1), "qvoffset -1")
    refused(lambda: cr.print(names, qvoffset=163), "qvoffset 163")
    text = cr.print(names, qvoffset=162)
    assert text.sizes[0] + text.sizes[1] > 0
    # a stream index out of range
    buf = np.zeros(1 << 16, dtype=np.uint8)
    for i in (-1, 2, 5):
        assert L.bbk_fastq_text_export(ctx._h, text._h, i, vp(buf)) == ERR_ARG and b"streams 0..1" in L.bbk_last_error()
        assert L.bbk_fastq_text_write(ctx._h, text._h, i, b"/nonexistent/x", 0) == ERR_ARG
        assert L.bbk_fastq_text_size(text._h, i) == 0
    assert L.bbk_fastq_text_export(None, text._h, 0, vp(buf)) == ERR_ARG
    assert L.bbk_fastq_text_write(ctx._h, text._h, 0, None, 0) == ERR_ARG
    # a batch made for another k
    hr20 = ctx.hammer_reads(*arrays([(seq, qual) for _, seq, qual in part]), 20)
    refused(lambda: c.correct_resident(hr20), "prepared for k = 20")
    for x in (text, hr20, cr, cr3, hr, hr3, c, s):
        x.free()


# ---- spades-kmerdata ---------------------------------------------------------------------------------------------------------
def _parse(path):
    with open(path) as f:
        lines = f.read().split("\n")
    return [(lines[j][1:], lines[j + 1], [ord(c) - 33 for c in lines[j + 3]]) for j in range(0, len(lines) - 3, 4)]


@pytest.fixture(scope="module")
def cli_input(tmp_path_factory, golden_dir):
    """the golden pair with seeded errors and low-quality ends, as test_cli of tests/test_gpu_readcorrect.py makes them"""
    d = tmp_path_factory.mktemp("readprint_cli")
    files = []
    for i in (1, 2):
        reads = Cs.seeded_errors(Cs.golden_reads(golden_dir, (i,)), 0.01, 40 + i)
        p = str(d / ("in%d.fq" % i))
        with open(p, "w") as f:
            for j, (seq, qual) in enumerate(reads):
                if j % 5 == 0:
                    qual = [2] * 3 + qual[3:-2] + [3, 1]
                elif j % 5 == 1:
                    qual = qual[:-4] + [2] * 4
                f.write("@r%d/%d extra words\n%s\n+\n%s\n" % (j, i, seq, "".join(chr(q + 33) for q in qual)))
        files.append(p)
    return str(d), files


def _run(args, timeout=120):
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout)


FIVE = ("0.cor", "1.cor", "0.unpaired", "0.bad", "1.bad")  # in the order of the streams


def test_cli_paired(cli_input, tmp_path):
    """--correct --paired --correct-stats: the five files are the restatement run over the tool's own k-mers and good
    bits; once more in several blocks that stay resident"""
    d, files = cli_input
    prefix, again = str(tmp_path / "out"), str(tmp_path / "again")
    r = _run(["-o", prefix, "-k", str(K), "-b", "100000", "--correct", "--paired", "--correct-stats"] + files)
    assert r.returncode == 0, r.stdout + r.stderr
    log = r.stdout + r.stderr
    assert "Correcting pair of reads: %s and %s" % tuple(files) in log
    keys = np.fromfile(prefix + ".kmers", dtype=np.uint64)
    n = len(keys)
    rec = np.fromfile(prefix + ".kmstat", dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    good = (rec["c"][:n] & 1).astype(int).tolist()
    index = {"".join(R.NUCL[(int(x) >> (2 * i)) & 3] for i in range(K)): j for j, x in enumerate(keys)}
    want, rows, rc = expected(index, good, _parse(files[0]), _parse(files[1]))
    for name, w in zip(FIVE, want):
        got = open("%s.%s.fastq" % (prefix, name), "rb").read()
        assert got == w, name
        assert got, "%s is empty: choose another seed or rate" % name
    flat = b"".join(want)
    for tag in (b" BH:ok\n", b" BH:failed\n", b" BH:changed:"):
        assert tag in flat, "no %r: choose another seed or rate" % tag
    st = rc.stats()
    assert "Correction done. Changed %d bases in %d reads." % (st[1], st[0]) in log
    assert "Failed to correct %d bases out of %d." % (st[2], st[3]) in log
    r = _run(["-o", again, "-k", str(K), "-b", "30000", "--resident-bytes", "100000000", "--correct", "--paired", "--correct-stats"] + files)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (r.stdout + r.stderr).count("Prepared batch") >= 3
    for name in FIVE + ("kmers", "kmstat"):
        ext = name if name.startswith("km") else name + ".fastq"
        assert open("%s.%s" % (again, ext), "rb").read() == open("%s.%s" % (prefix, ext), "rb").read(), name


def test_cli_output_dir(cli_input, tmp_path):
    """--output-dir: the reference's file names, and a corrected.yaml that the tool's own dataset reader takes back"""
    d, files = cli_input
    prefix, out = str(tmp_path / "out"), str(tmp_path / "corrected")
    r = _run(["-o", prefix, "-k", str(K), "--correct", "--paired", "--output-dir", out] + files)
    assert r.returncode == 0, r.stdout + r.stderr
    names = ["in1.00.0_0.cor.fastq", "in2.00.0_0.cor.fastq", "in_unpaired.00.0_0.cor.fastq", "in1.00.bad.fastq", "in2.00.bad.fastq"]
    assert sorted(os.listdir(out)) == sorted(names + ["corrected.yaml"])
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".fastq")]
    assert all(os.path.getsize(os.path.join(out, f)) > 0 for f in names)
    # the tool reads the description back: left, right, then single reads, each "Processing <file>"
    r = _run(["-o", str(tmp_path / "back"), "-k", str(K), "-d", os.path.join(out, "corrected.yaml")])
    assert r.returncode == 0, r.stdout + r.stderr
    seen = [line.split("Processing ")[1] for line in r.stdout.split("\n") if "Processing " in line]
    assert seen == [os.path.join(os.path.realpath(out), f) for f in names[:3]]
    text = open(os.path.join(out, "corrected.yaml")).read()
    assert text.index("left reads") < text.index("right reads") < text.index("single reads")


def test_cli_unequal_pair(cli_input, tmp_path):
    d, files = cli_input
    short = str(tmp_path / "short.fq")
    with open(files[1]) as f, open(short, "w") as g:
        g.write("".join(f.readlines()[:-4]))
    r = _run(["-o", str(tmp_path / "out"), "-k", str(K), "--correct", "--paired", files[0], short])
    assert r.returncode != 0
    assert "Pair of read files %s and %s contain unequal amount of reads" % (files[0], short) in r.stderr
    r = _run(["-o", str(tmp_path / "out"), "-k", str(K), "--correct", "--paired", files[0]])
    assert r.returncode != 0 and "a pair is a left and a right file" in r.stderr
