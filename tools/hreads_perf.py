"""Times the prepared read batch (HammerReads, csrc/hreads.hip) on the input of tools/readcorrect_perf.py: a random genome,
200 000 reads of 150 bases with 1 % substitutions (a tenth of them an N, quality 10 at an error and 35 elsewhere), k = 21,
the both-strand k-mers of the genome as the good set.  Three measurements, each one warm-up and then the median of
--repeats, and the whole thing --runs times in one process:
  kernels   k_hr_prepare (both passes), and the kernels behind the two views and the corrector's trimmed reads, from
            bbk_ctx_profile_get (device events)
  library   the wall time of bbk_corrector_correct on the host-trimmed reads (the existing door: it cuts the stretches on
            the host and uploads them; the trim itself is outside the timed call) against bbk_hreads_from_host +
            bbk_corrector_correct_prepared on the records as parsed, alternating call by call; the outputs must be equal
  tool      spades-kmerdata --correct end to end with --resident-bytes 0 and with everything resident; the output files
            must be the same bytes
Prints one JSON line per run and, with --out-dir, writes hreads_perf_<reads>_k21_run<i>.json there.

    python tools/hreads_perf.py [--reads 200000] [--repeats 5] [--runs 2] [--out-dir profiles/hreads] [--no-cli]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import spades_for_blackbird_amd as B  # noqa: E402

KERNELS = ("k_hr_prepare", "k_hr_ranges", "k_hr_pack", "k_hr_copy", "k_rc_island", "k_rc_search")


def med(x):
    return float(np.median(x))


def make_input(a):
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, a.genome)]
    starts = rng.integers(0, a.genome - a.read_len + 1, a.reads)
    bases = genome[(starts[:, None] + np.arange(a.read_len)[None, :])].reshape(-1).copy()
    err = rng.random(len(bases)) < a.sub_rate
    code = np.searchsorted(acgt, bases)
    bases[err] = acgt[(code[err] + rng.integers(1, 4, int(err.sum()))) % 4]
    bases[err & (rng.random(len(bases)) < 0.1)] = ord("N")
    qual = np.where(err, 10, 35).astype(np.uint8)
    off = (np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(a.read_len)).astype(np.uint64)
    return genome, bases, qual, off


def library(ctx, cor, a, bases, qual, off, k):
    """the two doors, alternating; returns the figures"""
    hr = ctx.hammer_reads(bases, qual, off, k)
    trims = hr.trims().astype(np.int64)
    hr.free()
    pos = np.arange(len(bases), dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), a.read_len)
    keep = (pos >= np.repeat(trims[:, 0], a.read_len)) & (pos < np.repeat(trims[:, 0] + trims[:, 1], a.read_len))
    tb, tq = bases[keep].copy(), qual[keep].copy()
    toff = np.zeros(a.reads + 1, dtype=np.uint64)
    toff[1:] = np.cumsum(trims[:, 1]).astype(np.uint64)

    def old():
        return cor.correct_arrays(tb, tq, toff)

    def new():
        h = ctx.hammer_reads(bases, qual, off, k)
        t1 = time.perf_counter()
        r = cor.correct_prepared(h)
        t2 = time.perf_counter()
        h.free()
        return r, t1, t2

    o, (n, _, _) = old(), new()  # warm-up: code objects, arena growth
    assert np.array_equal(o[0], n[0]) and np.array_equal(toff, n[1]) and np.array_equal(o[1], n[2]) and np.array_equal(o[2], n[3])
    w_old, w_new, w_prep, w_corr = [], [], [], []
    ker = {x: [] for x in KERNELS}
    for _ in range(a.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        old()
        w_old.append((time.perf_counter() - t0) * 1e3)
        ctx.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        _, t1, t2 = new()
        w_new.append((time.perf_counter() - t0) * 1e3)
        w_prep.append((t1 - t0) * 1e3)
        w_corr.append((t2 - t1) * 1e3)
        for x in KERNELS:
            ker[x].append(ctx.profile_get(x)["ms"])
    # the views, by themselves
    v_wall, v_ker = {"stretch": [], "candidate": []}, {"stretch": [], "candidate": []}
    for i in range(a.repeats + 1):
        h = ctx.hammer_reads(bases, qual, off, k)
        for name, fn in (("stretch", h.stretch_view), ("candidate", h.candidate_view)):
            ctx.synchronize()
            ctx.profile_reset()
            t0 = time.perf_counter()
            fn()
            if i:
                v_wall[name].append((time.perf_counter() - t0) * 1e3)
                v_ker[name].append(sum(ctx.profile_get(x)["ms"] for x in ("k_hr_ranges", "k_hr_pack", "k_hr_copy")))
        sizes = {"kmer_stretches": len(h.stretch_view()[0]), "candidates": len(h.candidate_view()),
                 "trimmed_reads": int((trims[:, 1] != a.read_len).sum())}
        h.free()
    return {"existing_wall_ms_median": med(w_old), "existing_wall_ms_min": min(w_old),
            "prepared_wall_ms_median": med(w_new), "prepared_wall_ms_min": min(w_new),
            "prepared_from_host_wall_ms_median": med(w_prep), "prepared_correct_wall_ms_median": med(w_corr),
            "existing_over_prepared_wall": med(w_old) / med(w_new),
            "kernels_ms_median_in_prepared_call": {x: med(v) for x, v in ker.items()},
            "views": {n: {"wall_ms_median": med(v_wall[n]), "kernels_ms_median": med(v_ker[n])} for n in v_wall}, **sizes}


def cli(a, bases, qual, k, tmp):
    from spades_for_blackbird_amd import build_host
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    path = os.path.join(tmp, "reads.fq")
    seqs = bases.reshape(a.reads, a.read_len)
    qs = (qual + 33).astype(np.uint8).reshape(a.reads, a.read_len)
    with open(path, "wb") as f:
        for i in range(a.reads):
            f.write(b"@r%d\n" % i + seqs[i].tobytes() + b"\n+\n" + qs[i].tobytes() + b"\n")
    exts = (".kmers", ".kmstat", ".hamming", ".hamming.idx", ".subclusters", ".subclusters.idx", ".newkmers", ".0.cor.fastq",
            ".0.bad.fastq")
    wall = {"0": [], "all": []}
    outs = {}
    for i in range(a.repeats + 1):
        for name, budget in (("0", "0"), ("all", str(4 * len(bases)))):
            prefix = os.path.join(tmp, "out_" + name)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-o", prefix, "--correct", "-k", str(k), "-b", str(a.cli_block), "--resident-bytes", budget,
                                path], capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stdout + r.stderr
            print("spades-kmerdata --correct --resident-bytes %s: %.2f s" % (budget, dt), file=sys.stderr, flush=True)
            if i:
                wall[name].append(dt)
            else:
                outs[name] = [open(prefix + e, "rb").read() for e in exts]
    assert outs["0"] == outs["all"]
    return {"block_bytes": a.cli_block, "resident_0_wall_s_median": med(wall["0"]), "resident_0_wall_s_min": min(wall["0"]),
            "resident_all_wall_s_median": med(wall["all"]), "resident_all_wall_s_min": min(wall["all"]),
            "resident_0_over_all": med(wall["0"]) / med(wall["all"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=int, default=1_000_000)
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--cli-block", type=int, default=8_000_000)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    k = 21
    genome, bases, qual, off = make_input(a)
    for run in range(1, a.runs + 1):
        ctx = B.Context(0)
        g = ctx.reads_from_ascii([genome.tobytes().decode()])
        kset = ctx.count(g, k, B.BOTH_STRANDS)
        cor = kset.corrector(np.ones(len(kset), dtype=np.uint8))
        ctx.profile(True)
        res = {"k": k, "reads": a.reads, "read_len": a.read_len, "genome": a.genome, "sub_rate": a.sub_rate, "repeats": a.repeats,
               "run": run, "library": library(ctx, cor, a, bases, qual, off, k)}
        print("run %d: library %s" % (run, json.dumps(res["library"])), file=sys.stderr, flush=True)
        ctx.profile(False)
        for x in (cor, kset, g):
            x.free()
        ctx.close()
        if not a.no_cli:
            with tempfile.TemporaryDirectory() as tmp:
                res["cli"] = cli(a, bases, qual, k, tmp)
        print(json.dumps(res), flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, "hreads_perf_%dk_k%d_run%d.json" % (a.reads // 1000, k, run)), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
