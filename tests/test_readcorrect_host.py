"""CPU: the host rule of the read corrector (csrc/readcorrect_host.hpp, the path of the searches that outgrow the device's
capacities) against the restatement (tests/readcorrect_restated.py): every corrected base, every result flag, the four
counters, and per search its pops, its largest heap and whether it failed.  The header runs in a stand-alone program
(tests/readcorrect_check.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  It walks the reads through
generator_stretches, the generator half of host/hammer_reads.hpp, which is thereby held against ValidKMerGenerator on reads
that are trimmed already."""
import os
import subprocess

import pytest

from tests import kmerdata_restated as KR
from tests import readcorrect_cases as Cs
from tests import readcorrect_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rc") / "readcorrect_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "readcorrect_check.cpp")])
    return exe


def _run(exe, path, k, keys, good, reads):
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (k, len(keys), len(reads)))
        for x, g in zip(keys, good):
            f.write("%d %d\n" % (x, g))
        for seq, qual in reads:
            f.write("%d %s %s\n" % (len(seq), seq, "".join(chr(q + 33) for q in qual)) if seq else "0\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, res, searches, stats = [], [], [], None
    for line in r.stdout.split("\n")[:-1]:
        w = line.split()
        if w[0] == "read":
            res.append(int(w[1]))
            out.append("" if w[2] == "-" else w[2])
        elif w[0] == "search":
            searches.append(tuple(int(x) for x in w[1:]))
        else:
            stats = [int(x) for x in w[1:]]
    return out, res, searches, stats


def _expected(k, index, good, reads):
    rc = R.ReadCorrector(index, good, k)
    out, res = rc.correct_batch(reads)
    searches = [(r, d, inf.pops, inf.max_heap, int(inf.failed)) for r, d, inf in rc.searches]
    return out, res, searches, rc.stats()


@pytest.mark.parametrize("k", [11, 21, 32])
def test_unit_cases(check_exe, tmp_path, k):
    cases = Cs.unit_cases(k) + [Cs.size_thr_case(k)]
    index, keys, good, reads = Cs.build(cases)
    reads += [("", []), (reads[0][0][:k - 1], reads[0][1][:k - 1])]  # CorrectReadsBatch: shorter than k
    exp = _expected(k, index, good, reads)
    assert exp[3][0] > 5 and exp[3][2] > 0
    assert _run(check_exe, str(tmp_path / "c"), k, keys, good, reads) == exp


@pytest.mark.parametrize("k", [11, 21, 32])
def test_island_cases(check_exe, tmp_path, k):
    cases = Cs.island_cases(k)
    index, keys, good, reads = Cs.build_islands(k, cases)
    rc = R.ReadCorrector(index, good, k)
    for (what, read, good_starts, _), (seq, qual) in zip(cases, reads):
        lleft, lright, solid = rc.island(seq, qual)
        runs = KR.coalesce(sorted(good_starts), 1)  # (first start, starts) of every run
        if runs:
            first, n = max(runs, key=lambda r: (r[1], -r[0]))
            assert (lleft, lright, solid) == (first, first + n - 1 + k - 1, n + k - 1), what
        else:
            assert solid == 0, what
    assert _run(check_exe, str(tmp_path / "c"), k, keys, good, reads) == _expected(k, index, good, reads)


def test_branching_reads(check_exe, tmp_path):
    k = 21
    for length, step in ((60, 4), (150, 2)):
        read, qual, good_kmers = R.branching_read(k, length, step=step)
        index, keys, good = R.make_index(good_kmers)
        exp = _expected(k, index, good, [(read, qual)])
        assert _run(check_exe, str(tmp_path / "c"), k, keys, good, [(read, qual)]) == exp


def test_golden_reads_with_seeded_errors(check_exe, tmp_path, golden_dir):
    k = 21
    for rate, files in ((0.02, (1, 2)), (0.05, (1,))):
        index, keys, good, reads = Cs.golden_case(golden_dir, k, rate=rate, files=files)
        exp = _expected(k, index, good, reads)
        assert exp[3][0] > 500 and exp[3][2] > 0  # many changed reads, some failed searches
        got = _run(check_exe, str(tmp_path / "c"), k, keys, good, reads)
        assert got[3] == exp[3] and got[1] == exp[1] and got[2] == exp[2]
        assert got[0] == exp[0]


def test_generator_stretches_of_trimmed_reads(check_exe, tmp_path):
    """host/hammer_reads.hpp: generator_stretches on a read that is trimmed already.  The read keeps a bad tail because it
    was trimmed on the left (trimming it again would cut the tail off); the generator's end_ stops before the q < 2 bases,
    so with every k-mer of the read good the island still ends before them and the right search runs"""
    k = 11
    seq = R.genome(k + 12, 5, k)
    qual = [2] * 3 + [30] * (k + 4) + [3] * 3 + [1] * 2
    s, q, lt, rt, n = R.trim_read(seq, qual, 4)
    assert lt == 3 and len(s) == k + 9  # the tail stayed
    assert len(R.trim_read(s, q, 4)[0]) < len(s)  # trimming again is not the same
    index, keys, good = R.make_index(R.kmers_of(s, k))
    rc = R.ReadCorrector(index, good, k)
    assert rc.island(s, q) == (0, len(s) - 3, len(s) - 2)
    exp = _expected(k, index, good, [(s, q)])
    assert len(exp[2]) == 2 and exp[1] == [1]
    assert _run(check_exe, str(tmp_path / "c"), k, keys, good, [(s, q)]) == exp
