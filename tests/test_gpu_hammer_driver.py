"""GPU: spades-hammer <config.info> as the pipeline's error-correction stage runs it.  The oracle of
every case is spades-kmerdata -- whose own outputs tests/test_gpu_readprint.py pins to the restatements -- or the Python
restatements themselves, never spades-hammer: a drop-in run, two iterations, the early exit, the determined PHRED offset,
the singleton filter and bbk_device_parse."""
import os
import subprocess

import numpy as np
import pytest

from spades_for_blackbird_amd import build_host
from tests import hammer_filtered_case as Fc
from tests import kmerdata_restated as KR
from tests import readcorrect_restated as R
from tests import readprint_restated as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = Fc.K


def _exe(name):
    return [e for e in build_host.build() if e.endswith("/" + name)][0]


def _config(path, **subst):
    """the shipped config.info with values substituted in place, as the stage script does (prepare_config_bh)"""
    out = []
    for line in open(os.path.join(ROOT, "tests", "golden", "hammer_config.info")).read().split("\n"):
        key = line.split()[0] if line.split() else ""
        out.append("%s %s" % (key, subst.pop(key)) if key in subst else line)
    out += ["%s %s" % kv for kv in sorted(subst.items()) if kv[0].startswith("bbk_")]  # this project's keys are not in the file
    assert all(k.startswith("bbk_") for k in subst), subst
    with open(path, "w") as f:
        f.write("\n".join(out))
    return path


def _hammer(tmp, name, dataset, **subst):
    """runs spades-hammer on a config in tmp/name: (output directory, working directory, log)"""
    d = os.path.join(str(tmp), name)
    os.makedirs(d)
    out, wd = os.path.join(d, "corrected"), os.path.join(d, "corrected", "tmp")
    cfg = _config(os.path.join(d, "config.info"), dataset=dataset, output_dir=out, input_working_dir=wd, **subst)
    r = subprocess.run([_exe("spades-hammer"), os.path.abspath(cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out, wd, r.stdout + r.stderr


def _kmerdata(args):
    r = subprocess.run([_exe("spades-kmerdata")] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def _paired_yaml(path, left, right, single=()):
    with open(path, "w") as f:
        f.write('- orientation: "fr"\n  type: "paired-end"\n  left reads:\n    - "%s"\n  right reads:\n    - "%s"\n' % (left, right))
        if single:
            f.write("  single reads:\n" + "".join('    - "%s"\n' % s for s in single))
    return path


def _fastqs(d):
    return sorted(f for f in os.listdir(d) if f.endswith(".fastq"))


def _read(d, f):
    with open(os.path.join(d, f), "rb") as fh:
        return fh.read()


def _yaml_files(path, tmp):
    """the read files of a dataset description as the tools' own reader (load_dataset_libs) lists them"""
    log = _kmerdata(["-o", os.path.join(str(tmp), "yaml_probe_%d" % len(os.listdir(str(tmp)))), "-k", str(K), "-d", path])
    return [line.split("Processing ")[1] for line in log.split("\n") if "Processing " in line]


def _write_pair(d, left, right, offset=33):
    os.makedirs(d, exist_ok=True)
    paths = [os.path.join(d, "reads_1.fq"), os.path.join(d, "reads_2.fq")]
    for p, recs in zip(paths, (left, right)):
        with open(p, "w", encoding="latin-1") as f:
            f.write(Fc.fastq_text(recs, offset))
    return paths


PAIR_NAMES = ["%s.%s.0_0.cor.fastq", "%s.%s.0_0.cor.fastq", "%s_unpaired.%s.0_0.cor.fastq", "%s.%s.bad.fastq", "%s.%s.bad.fastq"]


def _pair_names(left_base, right_base, common, ii):
    return [n % (b, ii) for n, b in zip(PAIR_NAMES, (left_base, right_base, common, left_base, right_base))]


# ---- (a) the drop-in run and (f) bbk_device_parse -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_run(tmp_path_factory, golden_dir):
    tmp = tmp_path_factory.mktemp("hammer_golden")
    files = [os.path.join(golden_dir, "ecoli_1K_%d.fq.gz" % i) for i in (1, 2)]
    y = _paired_yaml(os.path.join(str(tmp), "dataset.yaml"), *files)
    out, wd, log = _hammer(tmp, "hammer", y)
    return tmp, files, y, out, wd, log


def test_drop_in_run(golden_run):
    tmp, files, y, out, wd, log = golden_run
    ref = os.path.join(str(tmp), "kmerdata_out")
    _kmerdata(["-o", os.path.join(str(tmp), "kd"), "-k", str(K), "--correct", "--paired", "--correct-stats", "--output-dir", ref, "-d", y])
    names = _pair_names("ecoli_1K_1.fq", "ecoli_1K_2.fq", "ecoli_1K_", "00")
    assert _fastqs(out) == sorted(names) == _fastqs(ref)
    for f in names:
        assert _read(out, f) == _read(ref, f), f
    assert _read(out, names[0]) and _read(out, names[1])
    assert os.path.isdir(wd) and os.listdir(wd) == []  # general_debug 0: no intermediate file
    assert _yaml_files(os.path.join(out, "corrected.yaml"), tmp) == [os.path.join(os.path.realpath(out), f) for f in names[:3]]
    for line in ("=== ITERATION 0 begins ===", "Trying to determine PHRED offset", "Determined value is 33", "Solid k-mers iteration 0 produced",
                 "Correction done. Changed ", "Saving corrected dataset description to %s" % os.path.join(os.path.realpath(out), "corrected.yaml"),
                 "All done. Exiting."):
        assert line in log, line
    assert "ITERATION 1" not in log  # general_max_iterations 1


def test_device_parse_gives_the_same_bytes(golden_run):
    tmp, files, y, out, wd, log = golden_run
    out2, _, log2 = _hammer(tmp, "device_parse", y, bbk_device_parse="1")
    assert _fastqs(out2) == _fastqs(out)
    for f in _fastqs(out):
        assert _read(out2, f) == _read(out, f), f


# ---- (b) iterations ------------------------------------------------------------------------------------------------------
def test_two_iterations(tmp_path):
    left, right = Fc.crafted_pair()
    files = _write_pair(str(tmp_path / "in"), left, right)
    y = _paired_yaml(str(tmp_path / "dataset.yaml"), *files)
    out, _, log = _hammer(tmp_path, "two", y, general_max_iterations="2", input_qvoffset="33")
    assert "=== ITERATION 1 begins ===" in log and "ITERATION 2" not in log
    # iteration 0 is spades-kmerdata over the input
    ref0 = str(tmp_path / "ref0")
    log0 = _kmerdata(["-o", str(tmp_path / "kd0"), "-k", str(K), "--correct", "--paired", "--correct-stats", "--output-dir", ref0, "-d", y])
    assert "Correction done. Changed 0 bases" not in log0  # iteration 0 changes reads: the loop goes on
    names0 = _pair_names("reads_1", "reads_2", "reads_", "00")
    assert _fastqs(ref0) == sorted(names0)
    for f in names0:
        assert _read(out, f) == _read(ref0, f), f  # also: iteration 1 left the .00. files as they were
    # iteration 1 is spades-kmerdata over the .00. files: the pair, and the unpaired reads as single reads
    y1 = _paired_yaml(str(tmp_path / "dataset1.yaml"), *[os.path.join(ref0, f) for f in names0[:2]], single=[os.path.join(ref0, names0[2])])
    ref1 = str(tmp_path / "ref1")
    _kmerdata(["-o", str(tmp_path / "kd1"), "-k", str(K), "--correct", "--paired", "--correct-stats", "--output-dir", ref1, "-d", y1])
    names1 = sorted(f for f in _fastqs(out) if f not in names0)
    assert len(names1) == 7 and all(".01." in f for f in names1)

    def as_iteration_0(f):  # the iteration number is the field in front of the suffix CorrectAllReads appends
        head, tail = f.rsplit(".01.", 1)
        return head + ".00." + tail

    assert sorted(as_iteration_0(f) for f in names1) == _fastqs(ref1)
    for f in names1:
        assert _read(out, f) == _read(ref1, as_iteration_0(f)), f
    expect = ["reads_1.00.0_0.cor.01.0_0.cor.fastq", "reads_2.00.0_0.cor.01.0_0.cor.fastq", "reads__unpaired.00.0_0.cor.01.0_1.cor.fastq"]
    listed = _yaml_files(os.path.join(out, "corrected.yaml"), tmp_path)
    assert all(".01." in f for f in listed) and len(listed) == 4
    assert [os.path.basename(f) for f in listed[:2]] == expect[:2] and os.path.basename(listed[3]) == expect[2]


# ---- (c) the early exit ---------------------------------------------------------------------------------------------------
def test_early_exit(tmp_path):
    left, right = Fc.crafted_pair(quality=40, left_subst=(), right_subst=(), lonely=False)
    files = _write_pair(str(tmp_path / "in"), left, right)
    y = _paired_yaml(str(tmp_path / "dataset.yaml"), *files)
    out, _, log = _hammer(tmp_path, "early", y, general_max_iterations="3", input_qvoffset="33")
    assert "Correction done. Changed 0 bases in 0 reads." in log
    assert "Too few reads have changed in this iteration. Exiting." in log
    assert "=== ITERATION 0 begins ===" in log and "ITERATION 1" not in log
    names0 = _pair_names("reads_1", "reads_2", "reads_", "00")
    assert _fastqs(out) == sorted(names0)
    assert _yaml_files(os.path.join(out, "corrected.yaml"), tmp_path) == [os.path.join(os.path.realpath(out), f) for f in names0[:3]]


# ---- (d) the determined offset --------------------------------------------------------------------------------------------
def test_offset_64_is_determined(tmp_path):
    left, right = Fc.crafted_pair()
    runs = {}
    for offset in (33, 64):
        files = _write_pair(str(tmp_path / ("in%d" % offset)), left, right, offset)
        y = _paired_yaml(str(tmp_path / ("dataset%d.yaml" % offset)), *files)
        out, _, log = _hammer(tmp_path, "offset%d" % offset, y)  # input_qvoffset is empty in the shipped file
        assert "Determined value is %d" % offset in log
        runs[offset] = out
    names = _fastqs(runs[33])
    assert names == _fastqs(runs[64]) and len(names) == 5
    some = 0
    for f in names:
        a, b = _read(runs[33], f).split(b"\n"), _read(runs[64], f).split(b"\n")
        assert len(a) == len(b), f
        for i, (la, lb) in enumerate(zip(a, b)):
            assert lb == (bytes(c + 31 for c in la) if i % 4 == 3 else la), (f, i)
        some += len(a) > 1
    assert some >= 3


# ---- (e) the singleton filter ---------------------------------------------------------------------------------------------
def _parse(path):
    with open(path) as f:
        lines = f.read().split("\n")
    return [(lines[j][1:], lines[j + 1], [ord(c) - 33 for c in lines[j + 3]]) for j in range(0, len(lines) - 3, 4)]


def test_singleton_filter(tmp_path):
    _, recs = Fc.filtered_case()
    kmers, keys = Fc.filtered_set(recs)
    d = tmp_path / "in"
    d.mkdir()
    fq = str(d / "reads.fq")
    with open(fq, "w") as f:
        f.write(Fc.fastq_text(recs))
    y = str(tmp_path / "dataset.yaml")
    with open(y, "w") as f:
        f.write('- type: "single"\n  single reads:\n    - "%s"\n' % fq)
    out, wd, log = _hammer(tmp_path, "filtered", y, count_filter_singletons="1", general_debug="1", input_qvoffset="33")
    counts = Fc.counted(recs)
    assert "Singleton filter: %d k-mers of multiplicity 1 dropped." % sum(1 for c in counts.values() if c == 1) in log
    # the set: the Python-counted both-strand k-mers of multiplicity 2 and more
    got_keys = np.fromfile(os.path.join(wd, "00.kmers"), dtype=np.uint64)
    assert got_keys.tolist() == keys
    n = len(keys)
    rec = np.fromfile(os.path.join(wd, "00.kmstat"), dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    stats = KR.fill_kmer_data([(s, q) for _, s, q in recs], K, kmer_set=set(kmers))
    assert (rec["c"][:n] >> 1).tolist() == [stats[km].count for km in kmers]
    assert sorted(f for f in os.listdir(wd)) == sorted("00." + x for x in ("kmers", "kmstat", "hamming", "hamming.idx", "subclusters",
                                                                           "subclusters.idx", "newkmers"))
    # the corrected reads: the restated correction over the tool's own set and good bits
    good = (rec["c"][:n] & 1).astype(int).tolist()
    index = {km: i for i, km in enumerate(kmers)}
    rc = R.ReadCorrector(index, good, K)
    rows = P.corrected_records(rc, _parse(fq), 4, True, 33)
    want = [x.encode("latin-1") for x in P.route_single(rows)]
    names = ["reads.00.0_0.cor.fastq", "reads.00.bad.fastq"]
    assert _fastqs(out) == sorted(names)
    assert [_read(out, f) for f in names] == want
    assert want[0] and want[1]
    # the unfiltered run of the same input gives other bytes: the filter reached the correction
    plain, wd0, _ = _hammer(tmp_path, "plain", y, count_filter_singletons="0", general_debug="1", input_qvoffset="33")
    assert len(np.fromfile(os.path.join(wd0, "00.kmers"), dtype=np.uint64)) == len(counts) > n
    assert [_read(plain, f) for f in names] != want
