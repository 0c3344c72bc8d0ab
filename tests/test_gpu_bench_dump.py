"""GPU: `bench.py --steps K` times K steps, `--full` adds the side measurements, and `bench.py --dump-outputs DIR` writes
what the last timed step computed: what the engine returns for the same seeded reads, the k-mer set (and with
--ext-index the extension index) at the dumped record positions, within 64 MB for all ranks together."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import spades_for_blackbird_amd as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READS = 40000  # ~1.5 M distinct k-mers at k = 21: more than the dump keeps, so the sampled layout is exercised


def _u64(f):
    """float64 (n, 2 * words) of the dump -> u64 (n, words)"""
    assert f.dtype == np.float64 and np.array_equal(f, np.floor(f)) and f.min(initial=0) >= 0 and f.max(initial=0) < 2 ** 32
    return (f[:, 0::2].astype(np.uint64) << np.uint64(32)) | f[:, 1::2].astype(np.uint64)


LEAN = ["--no-cpu-baseline", "--no-gfa", "--no-e2e", "--no-k55", "--no-meta"]


def _bench(args, env=None, lean=True):
    """bench.py in a process of its own -> its JSON result line"""
    e = dict(os.environ, **(env or {}))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + (LEAN if lean else []),
                       capture_output=True, text=True, env=e, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_steps_sets_the_timed_steps():
    """--steps K runs K steps inside the timed region: every kernel of the step is launched K times as often there as
    with --steps 1, and ms_per_step is the timed region over K."""
    one, three = (_bench(["--gpus", "1", "--reads", str(READS), "--steps", str(k), "--warmup", "1"]) for k in (1, 3))
    l1 = {e["kernel"]: e["launches"] for e in one["roofline"]["kernels"]}
    l3 = {e["kernel"]: e["launches"] for e in three["roofline"]["kernels"]}
    assert l1 and l3 == {f: 3 * n for f, n in l1.items()}
    assert three["steps"] == 3 and three["ms_per_step"] == three["roofline"]["step"]["ms"] > 0


def test_bench_full_adds_the_side_measurements():
    """A plain run prints the headline and what the timed region measured; the side measurements that take runs of
    their own come with --full only, after the same timed steps."""
    side = {"e2e", "k55", "metagenome", "gfa_build", "cpu_baseline"}
    args = ["--gpus", "1", "--reads", str(READS), "--steps", "1", "--warmup", "1"]
    plain, full = _bench(args, lean=False), _bench(args + ["--full"], lean=False)
    assert not side & set(plain)
    assert side <= set(full)
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "distinct_kmers"):
        assert plain[key] == full[key], key
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["roofline"]["kernels"]
    assert "error" not in full["e2e"] and all("error" not in full["e2e"][t] for t in ("kmercount", "gbuilder"))
    assert full["k55"]["distinct_kmers"] > 0 and full["gfa_build"]["unitigs"] > 0
    assert set(full["metagenome"]["per_k"]) == {"21", "33", "55"} and full["cpu_baseline"]["value"] > 0


@pytest.mark.parametrize("ext_index", [False, True])
def test_bench_dump_outputs(tmp_path, ext_index):
    d = tmp_path / "out"
    line = _bench(["--gpus", "1", "--reads", str(READS), "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)] +
                  (["--ext-index"] if ext_index else []))
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    files = sorted(os.listdir(d))
    assert files == sorted(["kmers.npy", "kmers_index.npy", "kmers_size.npy"] +
                           (["extindex.npy", "extindex_index.npy", "extindex_masks.npy", "extindex_size.npy"] if ext_index
                            else []))
    assert line["dump_outputs"]["bytes"] == sum(os.path.getsize(d / f) for f in files) <= 64_000_000
    out = {f[:-4]: np.load(d / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())

    ctx = B.Context(0)
    reads = ctx.reads_synth(READS, read_len=150, genome_len=READS * 150 // 50, seed_genome=42, seed_reads=43)
    s = ctx.count(reads, 21, B.BOTH_STRANDS | B.REFERENCE_ORDER)
    n = len(s)
    assert out["kmers_size"][0] == n == line["distinct_kmers"]
    idx = out["kmers_index"].astype(np.int64)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(_u64(out["kmers"]), s.export(B.ORDER_REFERENCE_BUCKETS16)[idx])
    s.free()
    if ext_index:
        x = ctx.extindex(reads, 21)
        keys, masks = x.export()
        assert out["extindex_size"][0] == len(x)
        xi = out["extindex_index"].astype(np.int64)
        assert np.array_equal(_u64(out["extindex"]), keys[xi])
        assert np.array_equal(out["extindex_masks"], masks[xi].astype(np.float64))
        x.free()
    ctx.close()


def test_bench_dump_outputs_two_ranks(tmp_path):
    """`--gpus 2` (gloo, both ranks on the one GPU of the test box): every rank dumps its own shard, and the files of
    all ranks together stay within the 64 MB of the dump."""
    d = tmp_path / "out"
    line = _bench(["--gpus", "2", "--reads", "200000", "--steps", "1", "--warmup", "1", "--dump-outputs", str(d)],
                  env={"BBK_BENCH_BACKEND": "gloo"})
    files = sorted(os.listdir(d))
    assert files == sorted("kmers%s_rank%d.npy" % (p, r) for p in ("", "_index", "_size") for r in (0, 1))
    assert line["dump_outputs"]["ranks"] == 2
    assert line["dump_outputs"]["bytes"] == sum(os.path.getsize(d / f) for f in files) <= 64_000_000
    sizes = [int(np.load(d / ("kmers_size_rank%d.npy" % r))[0]) for r in (0, 1)]
    assert sum(sizes) == line["distinct_kmers"]
    for r in (0, 1):
        idx = np.load(d / ("kmers_index_rank%d.npy" % r)).astype(np.int64)
        assert len(_u64(np.load(d / ("kmers_rank%d.npy" % r)))) == len(idx) > 0 and idx[-1] < sizes[r]
