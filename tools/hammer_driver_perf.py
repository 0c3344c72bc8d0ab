"""Times spades-hammer and the minimum-count filter on the input of tools/fastqparse_perf.py: a random genome, 200 000 reads
of 150 bases with 1 % substitutions written as one FASTQ file, k = 21.
  pass1     the count of the reads' k-mer stretches through the binding -- Counter(BOTH_STRANDS).finish() against
            Counter(BOTH_STRANDS | WITH_COUNTS).finish() (the payload the filter needs, carried to the end) against
            Counter(BOTH_STRANDS | WITH_COUNTS).finish(min_count=2) -- alternating, a host clock around calls that end in a
            wait; k_mc_count and k_mc_write from bbk_ctx_profile_get (device events); the size of the set before and after
            the filter.  One warm-up, then the median of --repeats.
  tool      the wall time of spades-hammer <config.info> against spades-kmerdata --correct --correct-stats --output-dir on
            the same single-read library, both once more with the singleton filter (count_filter_singletons 1 /
            --filter-singletons): the four alternate run by run, one warm-up each and then --repeats runs, every run under
            its own time limit; spades-hammer and spades-kmerdata must write the same bytes.
  registers VGPRs and SGPRs of the filter's kernels (k_select_count of select.h over kmerfilter.hip's predicates, and
            k_mc_write) from the code-object metadata of kmerfilter.o where the object is at hand
            (--registers-only prints them and stops: no GPU needed).
Prints one JSON line and, with --out-dir, writes hammer_driver_perf_<reads>k_k21.json there.

    python tools/hammer_driver_perf.py [--reads 200000] [--repeats 5] [--out-dir profiles/hammer_driver]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import spades_for_blackbird_amd as B  # noqa: E402
from spades_for_blackbird_amd import build  # noqa: E402
from tools.hreads_perf import make_input, med  # noqa: E402
from tools.readprint_perf import write_fastq  # noqa: E402

KERNELS = ("k_mc_count", "k_mc_write")  # the timing families of the filter's count and write


def registers():
    """{kernel: {"vgpr": n, "sgpr": n}} of kmerfilter.o's kernels, from the notes of its gfx950 code object"""
    objdump, readelf = build._llvm_tool("llvm-objdump"), build._llvm_tool("llvm-readelf")
    obj = os.path.join(build.CSRC, "kmerfilter.o")
    if not objdump or not readelf or not os.path.exists(obj):
        return None
    out = {}
    d = tempfile.mkdtemp(prefix="bbk_regs_")
    try:
        shutil.copy(obj, d)
        subprocess.run([objdump, "--offloading", os.path.basename(obj)], capture_output=True, text=True, cwd=d, check=True)
        for f in os.listdir(d):
            if build.ARCH not in f:
                continue
            notes = subprocess.run([readelf, "--notes", os.path.join(d, f)], capture_output=True, text=True, check=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S*k_(?:select|mc)_\S+)", block)
                v, s = re.search(r"\.vgpr_count:\s+(\d+)", block), re.search(r"\.sgpr_count:\s+(\d+)", block)
                if name and v and s:
                    out[name.group(1)] = {"vgpr": int(v.group(1)), "sgpr": int(s.group(1))}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def pass1(a, bases, qual, off, k):
    ctx = B.Context(0)
    hr = ctx.hammer_reads(bases, qual, off, k)
    rd, _ = hr.stretch_view()
    variants = {"plain": (B.BOTH_STRANDS, None), "with_counts": (B.BOTH_STRANDS | B.WITH_COUNTS, None),
                "filtered": (B.BOTH_STRANDS | B.WITH_COUNTS, 2)}
    ms = {n: [] for n in variants}
    ker = {x: [] for x in KERNELS}
    sizes = {}

    def count(flags, mc):
        c = ctx.counter(k, flags)
        c.push(rd)
        s = c.finish() if mc is None else c.finish(min_count=mc)
        ctx.synchronize()
        return s

    for i in range(a.repeats + 1):
        for name, (flags, mc) in variants.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            s = count(flags, mc)
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                ms[name].append(dt)
            else:
                sizes[name] = len(s)
                if mc is not None:
                    sizes["dropped"] = s.n_dropped
            s.free()
        ctx.profile(True)  # the kernels' device time in a run of its own: the events are not part of the timed ones
        ctx.profile_reset()
        count(*variants["filtered"]).free()
        if i:
            for x in KERNELS:
                ker[x].append(ctx.profile_get(x)["ms"])
        ctx.profile(False)
    assert sizes["plain"] == sizes["with_counts"] == sizes["filtered"] + sizes["dropped"]
    hr.free()
    ctx.close()
    return {"ms_median": {n: med(v) for n, v in ms.items()}, "ms": {n: [round(x, 3) for x in v] for n, v in ms.items()},
            "kernels_ms_median": {x: med(v) for x, v in ker.items()}, "set_size": sizes}


def config_text(dataset, out, **subst):
    subst = dict(subst, dataset=dataset, output_dir=out, input_working_dir=os.path.join(out, "tmp"), input_qvoffset="33")
    lines = []
    for line in open(os.path.join(ROOT, "tests", "golden", "hammer_config.info")).read().split("\n"):
        key = line.split()[0] if line.split() else ""
        lines.append("%s %s" % (key, subst[key]) if key in subst else line)
    lines += ["%s %s" % kv for kv in sorted(subst.items()) if kv[0].startswith("bbk_")]  # this project's keys are not in the file
    return "\n".join(lines)


def tool(a, exes, path, tmp, k):
    y = os.path.join(tmp, "dataset.yaml")
    with open(y, "w") as f:
        f.write('- type: "single"\n  single reads:\n    - "%s"\n' % path)
    runs = {}
    for name, filt in (("hammer", "0"), ("hammer_filtered", "1")):
        out = os.path.join(tmp, name)
        cfg = os.path.join(tmp, name + ".info")
        with open(cfg, "w") as f:
            f.write(config_text(y, out, count_filter_singletons=filt, bbk_bufsize=str(a.cli_block)))
        runs[name] = ([exes["spades-hammer"], cfg], out)
    for name, extra in (("kmerdata", []), ("kmerdata_filtered", ["--filter-singletons"])):
        out = os.path.join(tmp, name)
        runs[name] = ([exes["spades-kmerdata"], "-o", os.path.join(tmp, name + "_prefix"), "-k", str(k), "-b", str(a.cli_block),
                       "--correct", "--correct-stats", "--output-dir", out, "-d", y] + extra, out)
    res = {n: {"wall_s": []} for n in runs}
    outs = {}
    for i in range(a.repeats + 1):
        for name, (cmd, out) in runs.items():
            shutil.rmtree(out, ignore_errors=True)
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            print("%s: run %.2f s" % (name, dt), file=sys.stderr, flush=True)
            if i:
                res[name]["wall_s"].append(round(dt, 3))
            else:
                outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f.endswith(".fastq")}
    assert outs["hammer"] == outs["kmerdata"] and outs["hammer_filtered"] == outs["kmerdata_filtered"], "different files"
    res["same_bytes"] = True
    res["filter_changes_output"] = outs["hammer"] != outs["hammer_filtered"]
    res["output_bytes"] = {n: {f: len(b) for f, b in o.items()} for n, o in outs.items() if n.startswith("hammer")}
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
    ap.add_argument("--registers-only", action="store_true", help="print the kernels' registers from the built object and stop")
    a = ap.parse_args()
    k = 21
    if a.registers_only:
        print(json.dumps(registers()))
        return
    from spades_for_blackbird_amd import build_host
    exes = {os.path.basename(e): e for e in build_host.build()}
    _, bases, qual, off = make_input(a)
    res = {"k": k, "reads": a.reads, "read_len": a.read_len, "genome": a.genome, "sub_rate": a.sub_rate, "repeats": a.repeats,
           "block_bytes": a.cli_block, "registers": registers()}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fq")
        write_fastq(path, a, bases, qual)
        res["pass1"] = pass1(a, bases, qual, off, k)
        res["tool"] = tool(a, exes, path, tmp, k)
    print(json.dumps(res), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "hammer_driver_perf_%dk_k%d.json" % (a.reads // 1000, k)), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
