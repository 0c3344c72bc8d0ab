"""CPU (needs g++ only): the graph of the mapping stage on the host.

tests/gfa_graph_check.cpp is a stand-alone program over csrc/gfa_graph.h, the host-only header with the GFA1 reader, the
segment / link / loop passes of the edge index (csrc/edgeprof.hip) and the block-parallel text writer.  Built with
AddressSanitizer + UBSan (host code only, nothing is loaded into python); one run checks the cases written out in the
program, and its dump mode is compared with the restated graph (tests/gmapper_restated.py) on two GFA texts."""
import os
import random
import subprocess

import pytest

from tests import gmapper_restated as G
from tests.helpers import rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gfa_graph") / "gfa_graph_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fopenmp", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", path, os.path.join(ROOT, "tests", "gfa_graph_check.cpp")])
    return path


def test_gfa_graph_on_the_host(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0 and "GFA-GRAPH-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _adversarial(rng, k=21):
    """the graph of test_gpu_gmapper.test_a_ranges_k127_and_adversarial_graphs: a homopolymer loop A^22 between G A^21 and
    A^21 C, a palindromic segment, a circular segment; here with KC tags, one of them negative"""
    x, y = _rand(rng, 30), _rand(rng, 50)
    segs = ["A" * 22, "G" + "A" * 21, "A" * 21 + "C", x + rc(x), y + y[:k]]
    kc = ["\tKC:i:%d" % v if v is not None else "" for v in (22, None, -3, 4000000000, 7)]
    return ("".join("S\t%d\t%s%s\n" % (3 + 2 * i, q, t) for i, (q, t) in enumerate(zip(segs, kc))) +
            "L\t3\t+\t3\t+\t21M\nL\t5\t+\t3\t+\t21M\nL\t3\t+\t7\t+\t21M\nL\t11\t+\t11\t+\t21M\n")


def _chain(rng, k=21):
    """four segments of a random genome that overlap by k, linked in a chain, under names that are no numbers"""
    genome = _rand(rng, 400)
    cuts = [0, 90, 200, 310, 400]
    segs = [genome[max(0, a - k):b] for a, b in zip(cuts, cuts[1:])]
    return ("".join("S\tutg%d\t%s\n" % (i, q.lower() if i == 2 else q) for i, q in enumerate(segs)) +
            "".join("L\tutg%d\t+\tutg%d\t+\t%dM\n" % (i, i + 1, k) for i in range(3)) + "L\tutg3\t-\tutg2\t-\t21M\n")


@pytest.mark.parametrize("make", [_adversarial, _chain])
def test_dump_equals_the_restated_graph(exe, tmp_path, make):
    k = 21
    text = make(random.Random(127))
    path = tmp_path / "g.gfa"
    path.write_text(text)
    r = subprocess.run([exe, "dump", str(path), str(k)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    rows = [line.split(" ") for line in r.stdout.splitlines()]
    assert rows and all(f[0] in ("S", "L") for f in rows), r.stdout[:500]
    g = G.Graph.from_gfa(text, k)
    n = len(g.names)
    assert n >= 4
    assert [f[1:] for f in rows if f[0] == "S"] == [
        [g.names[i], g.seq[2 * i], str(g.kc[i]), str(int(g.conj[2 * i] == 2 * i)), str(int(g.index_loop1(2 * i)))]
        for i in range(n)]
    assert [(int(f[1]), f[2], int(f[3]), f[4]) for f in rows if f[0] == "L"] == g.links
    if make is _adversarial:  # the flags this graph is there for
        assert g.index_loop1(0) and g.conj[6] == 6 and g.kc[2] == 2 ** 32 - 3 and g.kc[3] == 4000000000
