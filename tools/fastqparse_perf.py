"""Times FASTQ parsing on the device against the serial host reader, on the input of tools/hreads_perf.py written as one
FASTQ file: a random genome, 200 000 reads of 150 bases with 1 % substitutions, k = 21.
  block     (a) the host way of getting one block ready: the serial parse loop of spades-kmerdata (bbk-fastx-dump
            --time-records: next_record, the record appended to the block, the quality offset subtracted) plus
            bbk_hreads_from_host on the arrays it leaves -- against bbk_fastq_input_from_host (upload + index) plus
            bbk_hreads_from_fastq_input (gather + prepare) on the text of the same file; the k_fq_* kernels and
            k_hr_prepare from bbk_ctx_profile_get (device events).  One warm-up, then the median of --repeats.
  tool      (b) the wall time of spades-kmerdata --correct with --resident-bytes 0 and with everything resident, with and
            without --device-parse: the four alternate run by run, one warm-up each and then --repeats runs, every run
            under its own time limit; the output files of the four must be the same bytes.
Prints one JSON line and, with --out-dir, writes fastqparse_perf_<reads>k_k21.json there.

    python tools/fastqparse_perf.py [--reads 200000] [--repeats 5] [--out-dir profiles/fastqparse]
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
from tools.hreads_perf import make_input, med  # noqa: E402
from tools.readprint_perf import write_fastq  # noqa: E402

KERNELS = ("k_fq_count", "k_fq_lines", "k_fq_records", "k_fq_gather", "k_hr_prepare")


def block(a, dump, path, bases, qual, off, k):
    host_parse = []
    for i in range(a.repeats + 1):
        r = subprocess.run([dump, "--time-records", path], capture_output=True, text=True, timeout=a.step_timeout)
        assert r.returncode == 0, r.stderr
        n, nb, dt = r.stdout.split()
        assert int(n) == a.reads and int(nb) == len(bases)
        if i:
            host_parse.append(float(dt) * 1e3)
    text = np.fromfile(path, dtype=np.uint8)
    ctx = B.Context(0)
    ctx.profile(True)
    from_host, index, gather = [], [], []
    ker = {x: [] for x in KERNELS}
    for i in range(a.repeats + 1):
        t0 = time.perf_counter()
        h = ctx.hammer_reads(bases, qual, off, k)
        t1 = time.perf_counter()
        ctx.synchronize()
        ctx.profile_reset()
        t2 = time.perf_counter()
        inp = ctx.fastq_input(text)
        t3 = time.perf_counter()
        d = inp.hammer_reads(0, inp.records, k)
        t4 = time.perf_counter()
        if i == 0:
            assert inp.verdict() is None and inp.records == a.reads
            got = d.records()
            assert np.array_equal(got[0], bases) and np.array_equal(got[1], qual) and np.array_equal(got[2], off)
            assert np.array_equal(d.trims(), h.trims())
        else:
            from_host.append((t1 - t0) * 1e3)
            index.append((t3 - t2) * 1e3)
            gather.append((t4 - t3) * 1e3)
            for x in KERNELS:
                ker[x].append(ctx.profile_get(x)["ms"])
        for x in (d, inp, h):
            x.free()
    ctx.profile(False)
    ctx.close()
    res = {"text_bytes": int(len(text)),
           "host": {"parse_loop_ms_median": med(host_parse), "hreads_from_host_ms_median": med(from_host)},
           "device": {"index_ms_median": med(index), "gather_prepare_ms_median": med(gather),
                      "kernels_ms_median": {x: med(v) for x, v in ker.items()}}}
    res["host"]["total_ms"] = res["host"]["parse_loop_ms_median"] + res["host"]["hreads_from_host_ms_median"]
    res["device"]["total_ms"] = res["device"]["index_ms_median"] + res["device"]["gather_prepare_ms_median"]
    return res


def tool(a, exe, path, tmp, k):
    everything = str(4 * a.reads * a.read_len)
    runs = {"resident_0": ["--resident-bytes", "0"], "resident_0_device_parse": ["--resident-bytes", "0", "--device-parse"],
            "resident_all": ["--resident-bytes", everything],
            "resident_all_device_parse": ["--resident-bytes", everything, "--device-parse"]}
    res = {n: {"wall_s": []} for n in runs}
    outs = {}
    for i in range(a.repeats + 1):
        for name, extra in runs.items():
            prefix = os.path.join(tmp, "out_" + name)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-o", prefix, "--correct", "-k", str(k), "-b", str(a.cli_block)] + extra + [path],
                               capture_output=True, text=True, timeout=a.step_timeout)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stdout + r.stderr
            print("%s: run %.2f s" % (name, dt), file=sys.stderr, flush=True)
            if i:
                res[name]["wall_s"].append(round(dt, 3))
            else:
                outs[name] = [open(prefix + e, "rb").read() for e in (".0.cor.fastq", ".0.bad.fastq", ".kmers", ".kmstat")]
    assert all(o == outs["resident_0"] for o in outs.values()), "the runs wrote different files"
    res["same_bytes"] = True
    res["output_bytes"] = [len(x) for x in outs["resident_0"]]
    for n in runs:
        res[n]["wall_s_median"] = med(res[n]["wall_s"])
    return res


def main():
    ap = argparse.ArgumentParser()
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
    exes = {os.path.basename(e): e for e in build_host.build()}
    _, bases, qual, off = make_input(a)
    res = {"k": k, "reads": a.reads, "read_len": a.read_len, "genome": a.genome, "sub_rate": a.sub_rate, "repeats": a.repeats,
           "block_bytes": a.cli_block}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fq")
        write_fastq(path, a, bases, qual)
        res["block"] = block(a, exes["bbk-fastx-dump"], path, bases, qual, off, k)
        res["tool"] = tool(a, exes["spades-kmerdata"], path, tmp, k)
    print(json.dumps(res), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "fastqparse_perf_%dk_k%d.json" % (a.reads // 1000, k)), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
