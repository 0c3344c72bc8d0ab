"""GPU: the BayesHammer engine against tests/golden/hammer_ref/, the recorded outputs of the reference's own code
(oracle/record_hammer_ref.py; one thread, K = 21, tau = 1, one iteration, no singleton filter).  Nothing here reads the
reference tree or oracle/_ref/: the fixtures and tests/hammer_ref_case.py are all there is.

Every stage is compared with the reference directly; the stages that take the output of another one are fed the
reference's recorded output of it (statistics and clusters through bbk_kmerstats_load / bbk_hamclusters_load, good bits
through expander(good) / corrector(good)), so each stands alone.  The whole tool is compared file by file.
"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import expander_restated as E
from tests import hammer_ref_case as C
from tests import kmerdata_restated as KR
from tests import readprint_restated as P
from tests.hreads_child import arrays, device_set
from tests.test_hammer_reference_fixtures import K, OFFSET, TRIM, ascending, fx, good_of, records, reads_in_order

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _prepared(ctx, case):
    """the prepared batch of all reads of a case, the left file first"""
    return ctx.hammer_reads(*arrays(reads_in_order(case)), K, trim_quality=TRIM)


# ---- prepared reads: trims and both stretch tables against stage 0 ----------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_prepared_reads(ctx, case):
    rows = fx(case, "stage0")["reads"]
    hr = _prepared(ctx, case)
    assert len(hr) == len(rows)
    trims = [tuple(int(x) for x in t) for t in hr.trims()]
    tables = {}
    for table in ("kmer", "corrector"):
        off, st = hr.stretches(table)
        tables[table] = [[tuple(int(x) for x in st[j]) for j in range(int(off[i]), int(off[i + 1]))] for i in range(len(hr))]
    hr.free()
    for i, row in enumerate(rows):
        assert trims[i] == ((row["ltrim"], row["size"]) if row["size"] else (0, 0)), row["name"]
        want = KR.coalesce(row["starts_q2"], K) if row["size"] >= K else []
        # the k-mer table lies in the record as parsed, the corrector's in the trimmed read; the parsed reads are upper
        # case, where the two predicates agree
        assert tables["kmer"][i] == [(s + row["ltrim"], n) for s, n in want], row["name"]
        assert tables["corrector"][i] == want, row["name"]


# ---- statistics against stage 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_statistics(ctx, case):
    reads = reads_in_order(case)
    assert all(len(s) <= 1024 for s, _ in reads) and KR.min_window_complement(reads, K, TRIM) >= 2 ** -10  # the bound's condition
    s1 = fx(case, "stage1")
    asc, _, order = ascending(case)
    hr = _prepared(ctx, case)
    rd, qu = hr.stretch_view()
    s = ctx.count(rd, K, B.BOTH_STRANDS)
    assert [int(x) for x in s.export()[:, 0]] == [KR.kmer_key(x) for x in asc]  # the set: the reference counted the same k-mers
    ks = s.kmer_stats()
    ks.push(rd, qu)
    ks.finish()
    cnt, tq, qw = ks.export()
    data = KR.fill_kmer_data(reads, K, trim_quality=TRIM)  # for the float32 factors of the bound only
    worst = Fraction(0)
    for i, j in enumerate(order):
        km = asc[i]
        assert int(cnt[i]) == s1["count"][j], km
        assert ["%016x" % int(w) for w in qw[i]] == s1["qual_words"][j], km
        ref = Fraction(float(np.array([int(s1["total_qual_bits"][j], 16)], dtype=np.uint32).view(np.float32)[0]))
        exact, bound = KR.total_qual_bound(data[km].factors)
        assert abs(ref - exact) <= bound and abs(Fraction(float(tq[i])) - exact) <= bound, km
        worst = max(worst, abs(Fraction(float(tq[i])) - ref) / bound)
    print("%s: worst |device - reference| total_qual = %.4f of the bound" % (case, float(worst)))
    assert worst <= 2  # both lie within one bound of the exact product
    for h in (ks, s, hr):
        h.free()


# ---- clusters against stage 2 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_clusters(ctx, case):
    asc, pos, _ = ascending(case)
    s = device_set(ctx, [KR.kmer_key(x) for x in asc], K)
    h = s.hamming_clusters()
    members, sizes = h.members(), h.sizes()
    got, o = set(), 0
    for n in (int(x) for x in sizes):
        got.add(frozenset(asc[int(m)] for m in members[o:o + n]))
        o += n
    assert got == {frozenset(c) for c in fx(case, "stage2")["clusters"]}
    h.free()
    s.free()


# ---- subclusters against stage 3, from the reference's recorded statistics and clusters ---------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_subclusters(ctx, case, tmp_path):
    asc, pos, order = ascending(case)
    s1, s3 = fx(case, "stage1"), fx(case, "stage3")
    n = len(asc)
    prefix = str(tmp_path / case)
    rec = np.zeros(n, dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    rec["c"] = np.array([s1["count"][j] for j in order], dtype=np.uint32) << 1
    rec["tq"] = np.array([int(s1["total_qual_bits"][j], 16) for j in order], dtype=np.uint32).view(np.float32)
    rec["w"] = np.array([[int(w, 16) for w in s1["qual_words"][j]] for j in order], dtype=np.uint64)
    rec.tofile(prefix + ".kmstat")
    clusters = fx(case, "stage2")["clusters"]
    np.array([pos[x] for c in clusters for x in c], dtype=np.uint64).tofile(prefix + ".hamming")
    np.array([len(c) for c in clusters], dtype=np.uint64).tofile(prefix + ".hamming.idx")
    s = device_set(ctx, [KR.kmer_key(x) for x in asc], K)
    ks, hc = ctx.kmerstats_load(s, prefix + ".kmstat"), ctx.hamclusters_load(n, prefix + ".hamming")
    sc = hc.subcluster(ks)
    got = sc.export()
    assert [int(x) for x in got["good"][:n]] == good_of(case, s3["good"])
    # new centres: the reference numbers them in the order of its cluster file, which follows its hash; compared as a set
    assert len(got["new_keys"]) == len(s3["new_centres"]) == len(set(s3["new_centres"]))
    assert dict(zip((int(x) for x in got["new_keys"]), (int(x) for x in got["good"][n:]))) == \
        dict(zip((KR.kmer_key(x) for x in s3["new_centres"]), (int(b) for b in s3["good"][n:])))
    assert case != "crafted" or len(s3["new_centres"]) == 2
    for h in (sc, hc, ks, s):
        h.free()


# ---- the Expander against the final bits of stage 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_expander(ctx, case):
    asc, pos, _ = ascending(case)
    rounds = fx(case, "stage4")["rounds"]
    assert fx(case, "stage4")["extra_pass_added"] == 0  # the reference reached the closure: snapshot rounds end in the same set
    s = device_set(ctx, [KR.kmer_key(x) for x in asc], K)
    e = s.expander(good_of(case, fx(case, "stage3")["good"]))
    hr = _prepared(ctx, case)
    rd = hr.candidate_view()
    assert len(rd) == len(E.candidates(reads_in_order(case), K, TRIM))
    counts = e.run(rd, max_rounds=1000, min_changed=1)
    assert e.export().tolist() == good_of(case, rounds[-1]["good"])
    assert sum(counts) == sum(r["added"] for r in rounds) and counts[-1] == 0
    for h in (e, hr, s):
        h.free()


# ---- the corrector and the printed text against stage 5 -----------------------------------------------------------------------
def _names(case):
    base = [n[:-len(".fastq")] for n in C.case_texts(case)[2]]
    common = os.path.commonprefix(base)
    return ["%s.00.0_0.cor.fastq" % base[0], "%s.00.0_0.cor.fastq" % base[1], "%s_unpaired.00.0_0.cor.fastq" % common,
            "%s.00.bad.fastq" % base[0], "%s.00.bad.fastq" % base[1]]


@pytest.mark.parametrize("case", C.CASES)
def test_corrector_and_printed_text(ctx, case):
    asc, pos, _ = ascending(case)
    s5 = fx(case, "stage5")
    s = device_set(ctx, [KR.kmer_key(x) for x in asc], K)
    c = s.corrector(good_of(case, fx(case, "stage4")["rounds"][-1]["good"]))
    held = []
    for recs in records(case):
        hr = ctx.hammer_reads(*arrays([(seq, qual) for _, seq, qual in recs]), K, trim_quality=TRIM)
        held.append((hr, c.correct_resident(hr)))
    names = [[n for n, _, _ in recs] for recs in records(case)]
    text = held[0][1].print(names[0], qvoffset=OFFSET, tags=True, mate=held[1][1], mate_names=names[1])
    streams = [text.stream(i) for i in range(len(P.PAIRED_STREAMS))]
    for name, got in zip(_names(case), streams):
        assert bytes(got) == s5["files"][name].encode("latin-1"), name
    st = c.stats
    changed_reads, changed, uncorrected, total = (st[x] for x in ("changed_reads", "changed_nucleotides", "uncorrected_nucleotides",
                                                                  "total_nucleotides"))
    assert changed_reads == s5["changed_reads"]
    assert "Changed %d bases in %d reads." % (changed, changed_reads) in s5["log"][0]
    assert "Failed to correct %d bases out of %d." % (uncorrected, total) in s5["log"][1]
    text.free()
    for hr, cr in held:
        cr.free()
        hr.free()
    c.free()
    s.free()


# ---- the whole tool: spades-hammer <config.info>, the drop-in claim of README row f16 ------------------------------------------
def _config(path, **subst):
    out = []
    for line in open(os.path.join(ROOT, "tests", "golden", "hammer_config.info")).read().split("\n"):
        key = line.split()[0] if line.split() else ""
        out.append("%s %s" % (key, subst.pop(key)) if key in subst else line)
    out += ["%s %s" % kv for kv in sorted(subst.items())]  # this project's own keys are not in the file
    with open(path, "w") as f:
        f.write("\n".join(out))
    return path


def _hammer(tmp, case, name, **subst):
    d = os.path.join(str(tmp), name)
    os.makedirs(os.path.join(d, "in"))
    left, right, names = C.case_texts(case)
    paths = [os.path.join(d, "in", n) for n in names]
    for p, text in zip(paths, (left, right)):
        with open(p, "w", encoding="latin-1") as f:
            f.write(text)
    y = os.path.join(d, "dataset.yaml")
    with open(y, "w") as f:
        f.write('- orientation: "fr"\n  type: "paired-end"\n  left reads:\n    - "%s"\n  right reads:\n    - "%s"\n' % tuple(paths))
    out = os.path.join(d, "corrected")
    cfg = _config(os.path.join(d, "config.info"), dataset=y, output_dir=out, input_working_dir=os.path.join(out, "tmp"), **subst)
    exe = [e for e in build_host.build() if e.endswith("/spades-hammer")][0]
    r = subprocess.run([exe, os.path.abspath(cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out, r.stdout + r.stderr


def _yaml_files(path):
    """the quoted file names of a dataset description, in the order they are written"""
    with open(path) as f:
        return [line.split('"')[1] for line in f if line.strip().startswith("-") and '"' in line and "/" in line]


def _check_tool_output(out, case):
    s5 = fx(case, "stage5")
    assert sorted(f for f in os.listdir(out) if f.endswith(".fastq")) == sorted(s5["files"])
    for name, text in s5["files"].items():
        with open(os.path.join(out, name), "rb") as f:
            assert f.read() == text.encode("latin-1"), name
    listed = _yaml_files(os.path.join(out, "corrected.yaml"))
    assert [os.path.basename(f) for f in listed] == [f for _, f in s5["dataset"]]
    assert all(os.path.realpath(os.path.dirname(f)) == os.path.realpath(out) for f in listed)


@pytest.mark.parametrize("case", C.CASES)
def test_whole_tool(tmp_path, case):
    out, log = _hammer(tmp_path, case, "plain")
    _check_tool_output(out, case)
    s5 = fx(case, "stage5")
    for line in s5["log"]:
        assert line.split(": ", 1)[1] in log, line


def test_whole_tool_with_device_parse(tmp_path):
    out, _ = _hammer(tmp_path, "crafted", "device_parse", bbk_device_parse="1")
    _check_tool_output(out, "crafted")
