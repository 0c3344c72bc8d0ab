"""GPU: the chunk edges of the staged device -> host pump (context.hip: staged_d2h) through its two consumers, d2h_big
(memcpy into a host buffer) and d2f_big (parallel positional writes into a file), by way of the test-only entry
bbk_staged_copy.  The outputs of the rest of the suite are far below one 32 MiB chunk."""
import ctypes as C
import os

import numpy as np
import pytest

MiB = 1 << 20
# nothing; one word; the last size of d2h_big's direct path and the first of its pinned path; exactly one chunk; one chunk
# and a word; exactly two chunks; three chunks, the last one smaller than one page per writer
SIZES = [0, 8, 4 * MiB - 8, 4 * MiB, 32 * MiB, 32 * MiB + 8, 64 * MiB, 64 * MiB + 4096 + 8]


@pytest.mark.gpu
def test_staged_copy_chunk_edges(tmp_path):
    """every size in one context, in ascending order: the pinned buffers are allocated at 4 MiB and reused from there on"""
    import torch
    import spades_for_blackbird_amd as B
    L = B.load_library()
    L.bbk_staged_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    L.bbk_staged_copy.restype = C.c_int
    g = torch.Generator().manual_seed(20261019)
    src = torch.randint(0, 256, (max(SIZES),), dtype=torch.uint8, generator=g)
    exp = src.numpy()
    dev = src.cuda()
    torch.cuda.synchronize()
    ctx = B.Context(0)
    try:
        for n in SIZES:
            host = np.full(n + 8, 0xA5, dtype=np.uint8)  # 8 guard bytes behind the copy
            path = str(tmp_path / ("staged_%d.bin" % n))
            fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                rc = L.bbk_staged_copy(ctx._h, C.c_void_p(dev.data_ptr()), n, C.c_void_p(host.ctypes.data), fd)
            finally:
                os.close(fd)
            assert rc == 0, (n, L.bbk_last_error())
            assert np.array_equal(host[:n], exp[:n]), (n, np.flatnonzero(host[:n] != exp[:n])[:8])
            assert (host[n:] == 0xA5).all(), n
            assert os.path.getsize(path) == n, (n, os.path.getsize(path))
            got = np.fromfile(path, dtype=np.uint8)
            assert np.array_equal(got, exp[:n]), (n, np.flatnonzero(got != exp[:n])[:8])
            os.unlink(path)
    finally:
        ctx.close()
