"""Times the paired-info stage (EdgeIndex.pairinfo) on pairs of 150-base mates cut from a random genome, over the gbuilder
graph of error-free reads of that genome at k = 21: the wall time of the estimate pass (push_estimate + estimate) and of
the fill pass (fill_begin + push_fill + fill_finish), and within each the kernel-family times from bbk_ctx_profile_get
(device events) of map_paths, of the join kernels and of the sort-reduce.  One warm-up, then the median of --repeats.
Alongside: the single-thread wall time of the restatement's join (tests/pairinfo_restated.py) over the exported paths of
the same pairs -- the host alternative a user of bbk_paths_export has today -- and a check that it gives the same
histogram and the same points.  Prints one JSON line.

    python tools/pairinfo_perf.py [--pairs 200000] [--genome 1000000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import spades_for_blackbird_amd as B  # noqa: E402
from tests import gmapper_restated as G  # noqa: E402
from tests import pairinfo_cases as Cs  # noqa: E402
from tests import pairinfo_restated as P  # noqa: E402

MAP = ("gmap_count", "gmap_write")
JOIN = ("pairinfo_join",)
SORT_REDUCE = ("hist", "scan", "scatter", "unique", "reduce")


def cut_pairs(genome, n, read_len, seed):
    """fr pairs of fragments ~ N(400, 30), either strand; the mates as two lists of str"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(genome.encode(), dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    F = np.maximum(read_len, np.rint(rng.normal(400, 30, n)).astype(np.int64))
    a = (rng.random(n) * (len(g) - F)).astype(np.int64)
    idx = np.arange(read_len)
    head = g[a[:, None] + idx]                                   # the fragment's first read_len bases
    tail_rc = comp[g[(a + F)[:, None] - 1 - idx]]                # the reverse complement of its last read_len bases
    flip = rng.random(n) < 0.5                                   # the fragment comes from the other strand
    first = np.where(flip[:, None], tail_rc, head)
    second = np.where(flip[:, None], head, tail_rc)
    return [bytes(r).decode() for r in first], [bytes(r).decode() for r in second]


def host_join(g, k, paths1, paths2, len2, insert_size):
    """the restatement's listeners over exported paths, one thread: (histogram, points)"""
    isc, counts, index = P.InsertSizeCounter(g, 0), P.PairCounts(g), P.PairedIndex(g)
    flip = lambda p, npos: [(g.conj[e], [npos - r[1], npos - r[0], g.length(e) - r[3], g.length(e) - r[2]])  # noqa: E731
                            for e, r in reversed(p)]
    pairs = [(p1, flip(p2, n2 - k), n2) for p1, p2, n2 in zip(paths1, paths2, len2)]  # fr: the second mate is turned
    for p1, p2, n2 in pairs:
        isc.process(p1, p2, n2, 0)
        counts.process(p1, p2)
    for p1, p2, n2 in pairs:
        P.fill_pair(index, counts, p1, p2, n2, 0, insert_size, 0, 0)
    return sorted(isc.hist.items()), index.points()


def exported(ix, reads):
    off, rec = ix.map_paths(reads)
    e, a, b, c, d = (rec[f].tolist() for f in ("edge", "init_start", "init_end", "map_start", "map_end"))
    off = off.tolist()
    return [[(e[j], [a[j], b[j], c[j], d[j]]) for j in range(off[i], off[i + 1])] for i in range(len(off) - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--genome", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gfa", default=None, help="where the graph is written (default: a temporary directory)")
    a = ap.parse_args()
    k, seed = 21, 7
    ctx = B.Context(0)
    cover = ctx.reads_synth(30 * a.genome // a.read_len, read_len=a.read_len, genome_len=a.genome, sub_rate=0.0,
                            seed_genome=seed, seed_reads=seed + 1)
    tmp = None
    if a.gfa is None:
        tmp = tempfile.TemporaryDirectory()
        a.gfa = os.path.join(tmp.name, "pairinfo_perf.gfa")
    ctx.unitigs(ctx.extindex(cover, k)).write_gfa(a.gfa)
    ix = ctx.edgeindex_from_gfa(a.gfa, k)
    first_s, second_s = cut_pairs(Cs.synth_genome(seed, a.genome), a.pairs, a.read_len, seed)
    first, second = ctx.reads_from_ascii(first_s), ctx.reads_from_ascii(second_s)
    state = {}

    def estimate_pass():
        pi = ix.pairinfo(0)
        pi.push_estimate(first, second, B.ORIENT_FR)
        state["pi"], state["st"] = pi, pi.estimate()

    def fill_pass():
        pi = state["pi"]
        pi.fill_begin(int(state["st"]["mean"]), 0, 0)
        pi.push_fill(first, second, B.ORIENT_FR)
        pi.fill_finish()

    def timed(fn):
        fn()  # warm-up: code objects, arena growth
        ctx.profile(True)
        walls, fam = [], {f: [] for f in MAP + JOIN + SORT_REDUCE}
        for _ in range(a.repeats):
            ctx.profile_reset()
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            for f in fam:
                fam[f].append(ctx.profile_get(f)["ms"])
        ctx.profile(False)
        med = {f: float(np.median(v)) for f, v in fam.items()}
        kernels = {"map_paths": sum(med[f] for f in MAP), "join": sum(med[f] for f in JOIN),
                   "sort_reduce": sum(med[f] for f in SORT_REDUCE)}
        total = sum(kernels.values())
        return {"wall_ms_min": min(walls), "wall_ms_median": float(np.median(walls)), "kernel_ms_median": kernels,
                "kernel_share": {f: (v / total if total else 0.0) for f, v in kernels.items()}}

    est_t = timed(estimate_pass)
    fill_t = timed(fill_pass)
    pi, st = state["pi"], state["st"]
    his, cnt = pi.hist()
    e1, e2, gap, w = pi.points()

    # the host alternative: export the paths, join them in Python (one thread)
    g = G.Graph.from_gfa(open(a.gfa).read(), k)
    t0 = time.perf_counter()
    p1, p2 = exported(ix, first), exported(ix, second)
    t_export = time.perf_counter() - t0
    t0 = time.perf_counter()
    h_hist, h_points = host_join(g, k, p1, p2, [len(s) for s in second_s], int(st["mean"]))
    t_join = time.perf_counter() - t0
    same = (h_hist == list(zip(his.tolist(), cnt.tolist())) and
            h_points == list(zip(e1.tolist(), e2.tolist(), gap.tolist(), w.tolist())))
    out = {"k": k, "pairs": a.pairs, "read_len": a.read_len, "genome": a.genome, "segments": ix.segments,
           "mapped": st["mapped"], "negative": st["negative"], "edge_pairs": st["edge_pairs"], "mean": st["mean"],
           "hist_keys": len(his), "points": len(e1), "estimate_pass": est_t, "fill_pass": fill_t,
           "host_join_single_thread": {"paths_export_and_unpack_s": t_export, "join_s": t_join, "same_result": bool(same)}}
    print(json.dumps(out))
    if tmp is not None:
        tmp.cleanup()
    if not same:
        sys.exit("the host join and the engine disagree")


if __name__ == "__main__":
    main()
