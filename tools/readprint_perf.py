"""Times the correction pass of spades-kmerdata --correct -- correct, print, write -- for two builds of the tool on the same
input, and the three kernels of csrc/readprint.hip.  Input: that of tools/hreads_perf.py written as one FASTQ file: a random
genome, 200 000 reads of 150 bases with 1 % substitutions (a tenth of them an N, quality 10 at an error and 35 elsewhere),
k = 21.
  tool      `--parent-exe` (a spades-kmerdata built from the parent commit, next to its own libbbk.so) and this tree's
            spades-kmerdata, alternating run by run, one warm-up each and then --repeats runs, every run under its own
            time limit.  The correction pass is read from the tool's own log: from "Starting read correction." to
            "Correction done." (millisecond stamps); the wall time of the whole run is recorded next to it.  The .cor.fastq
            and .bad.fastq of the two builds must be the same bytes.
  kernels   k_rp_outcome, k_rp_size, k_rp_write from bbk_ctx_profile_get (device events) around correct_resident + print
            of the whole input as one batch, with and without tags; one warm-up, then the median of --repeats
Prints one JSON line and, with --out-dir, writes readprint_perf_<reads>k_k21.json there.

    python tools/readprint_perf.py --parent-exe <path> [--reads 200000] [--repeats 5] [--out-dir profiles/readprint]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import spades_for_blackbird_amd as B  # noqa: E402
from tools.hreads_perf import make_input, med  # noqa: E402

KERNELS = ("k_rp_outcome", "k_rp_size", "k_rp_write")
STAMP = re.compile(r"^\s*(\d+):(\d\d):(\d\d)\.(\d\d\d)\s+INFO\s+(.*)$")


def stamp_of(log, words):
    for line in log.split("\n"):
        m = STAMP.match(line)
        if m and m.group(5).startswith(words):
            return int(m.group(1)) * 3600 + int(m.group(2)) * 60 + int(m.group(3)) + int(m.group(4)) / 1000.0
    raise RuntimeError("no log line %r" % words)


def write_fastq(path, a, bases, qual):
    seqs = bases.reshape(a.reads, a.read_len)
    qs = (qual + 33).astype(np.uint8).reshape(a.reads, a.read_len)
    with open(path, "wb") as f:
        for i in range(a.reads):
            f.write(b"@r%d\n" % i + seqs[i].tobytes() + b"\n+\n" + qs[i].tobytes() + b"\n")


def tool(a, exes, path, tmp, k):
    """exes: {"parent": exe, "new": exe}; alternating, the warm-up run first"""
    args = ["--correct", "-k", str(k), "-b", str(a.cli_block), "--resident-bytes", str(4 * a.reads * a.read_len), path]
    res = {n: {"correction_pass_s": [], "wall_s": []} for n in exes}
    outs = {}
    for i in range(a.repeats + 1):
        for name, exe in exes.items():
            prefix = os.path.join(tmp, "out_" + name)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-o", prefix] + args, capture_output=True, text=True, timeout=a.step_timeout)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stdout + r.stderr
            log = r.stdout
            dc = stamp_of(log, "Correction done.") - stamp_of(log, "Starting read correction.")
            print("%s: correction pass %.3f s, run %.2f s" % (name, dc, dt), file=sys.stderr, flush=True)
            if i:
                res[name]["correction_pass_s"].append(round(dc, 3))
                res[name]["wall_s"].append(round(dt, 3))
            else:
                outs[name] = [open(prefix + e, "rb").read() for e in (".0.cor.fastq", ".0.bad.fastq", ".kmstat")]
    if len(exes) == 2:
        assert outs["parent"] == outs["new"], "the two builds wrote different files"
        res["same_bytes"] = True
        res["output_bytes"] = [len(x) for x in outs["new"][:2]]
        res["median_ratio_new_over_parent"] = med(res["new"]["correction_pass_s"]) / med(res["parent"]["correction_pass_s"])
        res["new_median_over_parent_slowest"] = med(res["new"]["correction_pass_s"]) / max(res["parent"]["correction_pass_s"])
    for n in exes:
        res[n]["correction_pass_s_median"] = med(res[n]["correction_pass_s"])
        res[n]["wall_s_median"] = med(res[n]["wall_s"])
    return res


def kernels(a, genome, bases, qual, off, k):
    ctx = B.Context(0)
    g = ctx.reads_from_ascii([genome.tobytes().decode()])
    kset = ctx.count(g, k, B.BOTH_STRANDS)
    cor = kset.corrector(np.ones(len(kset), dtype=np.uint8))
    names = ["r%d" % i for i in range(a.reads)]
    ctx.profile(True)
    out = {}
    for tags in (False, True):
        ker = {x: [] for x in KERNELS}
        wall_print, size = [], 0
        for i in range(a.repeats + 1):
            hr = ctx.hammer_reads(bases, qual, off, k)
            ctx.synchronize()
            ctx.profile_reset()
            cr = cor.correct_resident(hr)
            t0 = time.perf_counter()
            text = cr.print(names, tags=tags)
            t1 = time.perf_counter()
            if i:
                wall_print.append((t1 - t0) * 1e3)
                for x in KERNELS:
                    ker[x].append(ctx.profile_get(x)["ms"])
            size = sum(text.sizes)
            for x in (text, cr, hr):
                x.free()
        out["tags" if tags else "plain"] = {"kernels_ms_median": {x: med(v) for x, v in ker.items()},
                                            "print_call_wall_ms_median": med(wall_print), "text_bytes": size}
    ctx.profile(False)
    for x in (cor, kset, g):
        x.free()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=int, default=1_000_000)
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cli-block", type=int, default=8_000_000)
    ap.add_argument("--step-timeout", type=float, default=300)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    k = 21
    from spades_for_blackbird_amd import build_host
    exes = {}
    if a.parent_exe:
        exes["parent"] = a.parent_exe
    exes["new"] = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    genome, bases, qual, off = make_input(a)
    res = {"k": k, "reads": a.reads, "read_len": a.read_len, "genome": a.genome, "sub_rate": a.sub_rate, "repeats": a.repeats,
           "block_bytes": a.cli_block}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fq")
        write_fastq(path, a, bases, qual)
        res["tool"] = tool(a, exes, path, tmp, k)
    res["kernels"] = kernels(a, genome, bases, qual, off, k)
    print(json.dumps(res), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "readprint_perf_%dk_k%d.json" % (a.reads // 1000, k)), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
