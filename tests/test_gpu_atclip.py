"""GPU: the early poly-A/T clipper (csrc/atclip.hip: bbk_extindex_remove_at_edges / _remove_at_tips) against the
sequential restatement of EarlyLowComplexityClipperProcessor (tests/atclip_restated.py): same counts, byte-equal masks;
its composition with the early tip clipper and the unitig stage against the oracle; the gbuilder options."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from oracle import oracle as O
from spades_for_blackbird_amd.tools import gfa_canon
from tests import atclip_restated as R
from tests.helpers import polya_reads, synth_reads

pytestmark = pytest.mark.gpu


READS = polya_reads()
AT_READ = "AT" * 75


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def greads(ctx):
    return ctx.reads_from_ascii(READS)


def _order(keys):
    return np.lexsort([keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)])


_BASE = {}


def base_index(k):
    """(restated Index in the oracle's order, permutation to the ascending order of the device table, sorted keys)"""
    if k not in _BASE:
        ox = O.ExtIndex(READS, k, 1)
        order = _order(ox.kmers)
        _BASE[k] = (R.Index.from_oracle(ox), order, ox.kmers[order])
    return _BASE[k]


def restated(k, steps):
    base, order, _ = base_index(k)
    ix = R.Index(base.kmers, base.masks, k)
    out = []
    for st in steps:
        out.append(R.remove_at_edges(ix, st[1]) if st[0] == "edges" else R.remove_at_tips(ix, *st[1:]))
    return out, ix.mask_array()[order]


def on_gpu(x, steps):
    return [x.remove_at_edges(st[1]) if st[0] == "edges" else x.remove_at_tips(*st[1:]) for st in steps]


def check(x, k, steps):
    exp, exp_masks = restated(k, steps)
    got = on_gpu(x, steps)
    assert got == exp, steps
    gk, gm = x.export()
    assert np.array_equal(gk, base_index(k)[2])
    assert np.array_equal(gm, exp_masks), steps
    return got


@pytest.mark.parametrize("ratio", [0.8, 0.6])
@pytest.mark.parametrize("k", [21, 25, 33, 55, 77, 101])
def test_parity_with_restatement(ctx, greads, k, ratio):
    edge = ("edges", ratio)
    plans = [[edge]] + [[("tips", ratio, mn, mx)] for mn, mx in ((10, 200), (5, 3), (k, 1000))] + \
        [[edge, ("tips", ratio, 10, 200)]]
    results = []
    for steps in plans:
        results.append(check(ctx.extindex(greads, k), k, steps))
    assert results[0][0][0] > 0, "no low-complexity edge in the data"
    assert results[1][0][0] > 0, "no low-complexity tip in the data"


def _kmer_masks(x, k, seq):
    keys, masks = x.export()
    pos = {s: i for i, s in enumerate(R.kmer_strings(keys, k))}
    return [int(masks[pos[min(s, R.rc(s))]]) for s in (seq[i:i + k] for i in range(len(seq) - k + 1))]


def test_at_repeats_are_kept(ctx, greads):
    k = 21
    x = ctx.extindex(greads, k)
    before = _kmer_masks(x, k, AT_READ)
    assert x.remove_at_edges(0.6)[0] > 0 and x.remove_at_tips(0.6, 10, 200)[0] > 0
    assert _kmer_masks(x, k, AT_READ) == before


def test_input_routes_and_table_widths(ctx, greads, monkeypatch):
    """The same masks from the streaming builder, from the count + index pass, and with 64-bit prefix-table entries."""
    steps = [("edges", 0.8), ("tips", 0.8, 10, 200)]
    for k in (21, 33):
        b = ctx.extbuilder(k)
        for lo in range(0, len(READS), 700):
            b.push(ctx.reads_from_ascii(READS[lo:lo + 700]))
        check(b.finish(), k, steps)
        _, x = ctx.count_extindex(greads, k)
        check(x, k, steps)
    monkeypatch.setenv("BBK_WIDE_INDEX", "1")
    for k in (21, 55):
        check(ctx.extindex(greads, k), k, steps)


def oracle_route(k, bound, reads=READS):
    """The restated A/T passes written into the oracle's own masks, then its early tip clipper: (tip-clip result, the
    oracle index ready for its unitig stage)"""
    ox = O.ExtIndex(reads, k, 1)
    ix = R.Index.from_oracle(ox)
    R.remove_at_edges(ix, 0.8)
    R.remove_at_tips(ix, 0.8, 10, 200)
    np.ctypeslib.as_array(ox._st.masks, shape=(ox._st.n_k,))[:] = ix.mask_array()
    return ox.clip_tips(bound), ox


@pytest.mark.parametrize("k,bound", [(21, 129), (33, 40), (55, 95), (77, 20)])
def test_composition_with_tip_clipper(ctx, greads, k, bound):
    exp_clip, ox = oracle_route(k, bound)
    x = ctx.extindex(greads, k)
    x.remove_at_edges()
    x.remove_at_tips()
    assert x.clip_tips(bound) == exp_clip
    got = sorted(min(s, R.rc(s)) for s in ctx.unitigs(x).sequences())
    exp = sorted(min(s, R.rc(s)) for s in ox.unitigs().seqs)
    assert got == exp


def _consistent(keys, masks, k):
    ix = R.Index(R.kmer_strings(keys, k), masks, k)
    for s in ix.oriented():
        m = ix.get(s)
        for c in range(4):
            if m >> c & 1:
                assert ix.get(s[1:] + R.ACGT[c]) >> (4 + R.IDX[s[0]]) & 1, (s, c)


def test_properties(ctx, greads):
    k = 21
    x = ctx.extindex(greads, k)
    _, m0 = x.export()
    assert x.remove_at_edges()[0] > 0
    assert x.remove_at_edges() == (0, 0)  # (a) only junctions lose bits, and the collected ones have none left
    _, m1 = x.export()
    assert x.remove_at_tips()[0] > 0
    keys, m2 = x.export()
    for a, b in ((m0, m1), (m1, m2)):
        assert not np.any(b & ~a)  # (b) no mask gains a bit
    _consistent(keys, m2, k)  # (c) every outgoing bit has its incoming bit
    # (d) uniform data: without errors nothing is of low complexity and there are no short tips; with errors no
    # junction is of low complexity (short error tips may be, so the tip pass is left to the parity test)
    for sub_rate in (0.0, 0.01):
        reads = synth_reads(1500, read_len=150, genome_len=15000, sub_rate=sub_rate, seed=13)
        x = ctx.extindex(ctx.reads_from_ascii(reads), k)
        _, before = x.export()
        assert x.remove_at_edges() == (0, 0)
        if sub_rate == 0.0:
            assert x.remove_at_tips() == (0, 0)
        assert np.array_equal(x.export()[1], before)


def test_argument_errors(ctx, greads):
    x = ctx.extindex(greads, 21)
    for ratio in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(B.BBKError):
            x.remove_at_edges(ratio)
        with pytest.raises(B.BBKError):
            x.remove_at_tips(ratio)
    with pytest.raises(B.BBKError):
        x.remove_at_tips(0.8, 10, 0)
    with pytest.raises(B.BBKError):
        x.remove_at_tips(0.8, 22, 200)
    x.remove_at_tips(0.8, 21, 200)  # min_len = k is allowed
    a = C.c_uint64()
    L = ctx._L
    assert L.bbk_extindex_remove_at_edges(None, x._h, 0.8, C.byref(a), C.byref(a)) == -1
    assert L.bbk_extindex_remove_at_edges(ctx._h, None, 0.8, C.byref(a), C.byref(a)) == -1
    assert L.bbk_extindex_remove_at_edges(ctx._h, x._h, 0.8, None, C.byref(a)) == -1
    assert L.bbk_extindex_remove_at_tips(ctx._h, x._h, 0.8, 10, 200, C.byref(a), None) == -1
    even = ctx.extindex(greads, 20)
    with pytest.raises(B.BBKError):
        even.remove_at_edges()
    with pytest.raises(B.BBKError):
        even.remove_at_tips()


@pytest.fixture(scope="module")
def gbuilder():
    from spades_for_blackbird_amd import build, build_host
    build.build()
    return next(p for p in build_host.build() if os.path.basename(p) == "spades-gbuilder")


def test_gbuilder_early_clipping(gbuilder, tmp_path):
    # without the (AT)n reads: they form self-conjugate perfect loops, whose KC the oracle counts on both strands and
    # the engine on one (with or without clipping); everything else of the graph is compared, KC included
    reads = [r for r in READS if r != AT_READ]
    k, bound = 21, 129
    fa = tmp_path / "r.fa"
    with open(fa, "w") as f:
        for i, s in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, s))
    _, ox = oracle_route(k, bound, reads)
    exp = gfa_canon.canon_md5(ox.unitigs().gfa(with_cov=True)[0], k, with_kc=True)
    plain = O.ExtIndex(reads, k, 1).unitigs().gfa(with_cov=True)[0]
    assert gfa_canon.canon_md5(plain, k, with_kc=True) != exp  # the options change the graph
    for name, extra in (("one", []), ("copy2", ["--devices", "0,0", "--exchange", "copy"])):
        out = tmp_path / (name + ".gfa")
        r = subprocess.run([gbuilder, str(fa), str(out), "-k", str(k), "--gfa", "-c", "--early-at-clip",
                            "--early-tip-clip", str(bound), "-b", "200000"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
        assert gfa_canon.canon_md5(open(out).read(), k, with_kc=True) == exp, name
        for line in ("-mers were removed by early poly A/T remover", "-mers were removed by early poly A/T tip clipper",
                     "-mers were removed by early tip clipper"):
            assert line in r.stdout, (name, line)
    r = subprocess.run([gbuilder, str(fa), str(tmp_path / "x.gfa"), "--early-tip-clip"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--early-at-clip" in r.stdout  # a missing bound prints the usage
