"""GPU: the N>1 sharded count end to end with two ranks sharing the one GPU of the test box (gloo for
the exchange, staged through the host).  The union of the two shards must be the single-rank result."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import spades_for_blackbird_amd as B
        from spades_for_blackbird_amd import distributed as D
        torch.cuda.set_device(0)
        ctx = B.Context(0, stream=torch.cuda.current_stream())
        reads = ctx.reads_synth(20000, read_len=150, genome_len=120000, seed_genome=42, seed_reads=43 + rank)
        # built in the final_kmers order (what bench.py --gpus N does); the ascending export sorts a copy
        shard = D.sharded_count(ctx, reads, 21, both_strands=True, reference_order=True)
        ptr, order = shard.device_keys()
        asc, ref = shard.export(B.ORDER_SORTED), shard.export(B.ORDER_REFERENCE_BUCKETS16)
        from oracle import oracle as O
        bk = np.array([O.bucket(asc[i], 16) for i in range(len(asc))])
        ref_ok = order == B.ORDER_REFERENCE_BUCKETS16 and np.array_equal(ref, asc[np.argsort(bk, kind="stable")])
        q.put((rank, asc, reads.to_list(), bool(ref_ok)))
        ctx.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu():
    from oracle import oracle as O
    world = 2
    c = mp.get_context("spawn")
    q = c.Queue()
    port = _free_port()
    procs = [c.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r, (k, rd, ok)) for r, k, rd, ok in (q.get(timeout=300) for _ in range(world)))
    assert all(v[2] for v in res.values()), "a shard is not in the final_kmers order"
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = res[0][0], res[1][0]
    sa, sb = set(int(x) for x in a[:, 0]), set(int(x) for x in b[:, 0])
    assert not (sa & sb)
    exp = O.kmercount(res[0][1] + res[1][1], 21, 16, 4)
    assert (sa | sb) == set(int(x) for x in exp[:, 0])
    assert len(sa) + len(sb) == len(exp)


def _gfa_worker(rank, world, port, q, tmpdir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import spades_for_blackbird_amd as B
        from spades_for_blackbird_amd import distributed as D
        torch.cuda.set_device(0)
        ctx = B.Context(0, stream=torch.cuda.current_stream())
        reads = ctx.reads_synth(6000, read_len=150, genome_len=20000, seed_genome=7, seed_reads=100 + rank)
        k = 21
        shard = D.sharded_extindex(ctx, reads, k)
        sk, sm = shard.export()
        # small messages: the gather runs in several point-to-point rounds
        full = D.gather_extindex(ctx, shard, k, dst=0, max_msg_bytes=4096)
        out = None
        if rank == 0:
            fk, fm = full.export()
            u = ctx.unitigs(full)
            path = os.path.join(tmpdir, "sharded.gfa")
            u.write_gfa(path)
            out = (fk, fm, open(path).read())
        q.put((rank, reads.to_list(), sk, sm, out))
        ctx.close()
    finally:
        dist.destroy_process_group()


def test_sharded_extindex_and_gfa_two_ranks(tmp_path):
    """(canonical k-mer, mask) records follow the k-mer's owner in the one exchange and are OR-merged
    there; the shards are gathered for the unitig stage.  Two ranks (sharing the one GPU of the test box, gloo staged
    through the host): every shard holds exactly the k-mers it owns with their COMPLETE masks, the gathered index is
    the single-rank index byte for byte, and the GFA equals the oracle's in canonical form."""
    from oracle import oracle as O
    from spades_for_blackbird_amd import distributed as D
    from spades_for_blackbird_amd.tools import gfa_canon
    world = 2
    c = mp.get_context("spawn")
    q = c.Queue()
    port = _free_port()
    procs = [c.Process(target=_gfa_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (rd, sk, sm, out) for r, rd, sk, sm, out in (q.get(timeout=300) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    reads = res[0][0] + res[1][0]
    ox = O.ExtIndex(reads, 21, 1)
    order = np.lexsort([ox.kmers[:, j] for j in range(ox.kmers.shape[1] - 1, -1, -1)])
    ek, em = ox.kmers[order], ox.masks[order]
    own = D.owner_of(ek, world)
    for r in range(world):
        sk, sm = res[r][1], res[r][2]
        assert np.array_equal(sk, ek[own == r]) and np.array_equal(sm, em[own == r]), "shard %d" % r
    fk, fm, txt = res[0][3]
    assert np.array_equal(fk, ek) and np.array_equal(fm, em)
    exp = ox.unitigs().gfa()[0]
    assert gfa_canon.canon_text(txt) == gfa_canon.canon_text(exp)


NCCL_SCRIPT = r"""
import os, sys, numpy as np, torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = %(port)r
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
dist.init_process_group("nccl", rank=0, world_size=1)
torch.cuda.set_device(0)
import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import distributed as D
from spades_for_blackbird_amd.tools import gfa_canon
# (1) a whole buffer through the collective, with the synchronisation sharded_count uses: every byte arrives as long
#     as the message stays within what distributed.py ever sends (MAX_MSG_BYTES), and up to 1 GiB
for nbytes in (D.MAX_MSG_BYTES, 1 << 30):
    n = nbytes // 8
    send = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
    recv = torch.zeros_like(send)
    dist.all_to_all_single(recv, send, [n], [n])
    torch.cuda.current_stream().synchronize()
    assert bool(torch.equal(recv, send)), nbytes
    del send, recv
# (2) the N>1 code path on RCCL with one rank == the unsharded result
ctx = B.Context(0, stream=torch.cuda.current_stream())
reads = ctx.reads_synth(300000, read_len=150, genome_len=900000, seed_genome=42, seed_reads=43)
a = D.sharded_count(ctx, reads, 21, both_strands=True, reference_order=True).export(B.ORDER_REFERENCE_BUCKETS16)
b = ctx.count(reads, 21, B.BOTH_STRANDS | B.REFERENCE_ORDER).export(B.ORDER_REFERENCE_BUCKETS16)
assert np.array_equal(a, b)
x1 = D.sharded_extindex(ctx, reads, 21)
xf = D.gather_extindex(ctx, x1, 21)
x0 = ctx.extindex(reads, 21)
k1, m1 = xf.export(); k0, m0 = x0.export()
assert np.array_equal(k1, k0) and np.array_equal(m1, m0)
dist.destroy_process_group()
print("NCCL-ONE-RANK-OK")
"""


def test_nccl_one_rank_path():
    """The RCCL-backed path with a single rank (all a one-GPU box can run): messages up to 1 GiB arrive complete (above
    that RCCL 2.26.6 drops the tail, which is why distributed.py caps messages at 256 MiB and keeps the own segment
    out of the collective), and the sharded count / extension index equal the unsharded ones."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", NCCL_SCRIPT % {"root": root, "port": str(_free_port())}],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "NCCL-ONE-RANK-OK" in r.stdout


def test_bench_two_ranks_rehearsal():
    """`python bench.py --gpus 2` exactly as the driver calls it (no launcher: bench.py starts its own ranks), with
    the collective backend switched to gloo so that both ranks can share the one GPU of the test box: the whole N>1 code
    path of the benchmark (owner exchange, merge, expansion, max-over-ranks timing; with --full the sharded GFA build)
    runs end to end and the aggregate equals the single-rank count of the union of the two ranks' reads."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BBK_BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--reads", "200000", "--steps", "1",
                        "--warmup", "1", "--full"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert line["gfa_build"]["ranks"] == 2 and line["gfa_build"]["unitigs"] > 0
    # the union of the two ranks' reads counted by one rank
    import spades_for_blackbird_amd as B
    ctx = B.Context(0)
    g = 2 * 200000 * 150 // 50
    a = ctx.reads_synth(200000, read_len=150, genome_len=g, seed_genome=42, seed_reads=43).to_list()
    b = ctx.reads_synth(200000, read_len=150, genome_len=g, seed_genome=42, seed_reads=44).to_list()
    both = ctx.count(ctx.reads_from_ascii(a + b), 21, B.BOTH_STRANDS)
    assert line["distinct_kmers"] == len(both)
    ctx.close()
