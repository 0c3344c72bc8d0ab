"""GPU: the ordered selection of select.h through its test-only export bbk_select_u32 (per_item(vals[i] >= min), an emitter
that stores i and vals[i]) against numpy.flatnonzero: sizes around the lane width (4) and the tile (256), and one whose
tile totals need a second scan level (more than 4096 tiles); at each, the patterns a ballot-ranked selection can get
wrong.  Eight passing values lie behind n and must never be selected; the outputs behind `kept` keep their sentinel.
Bit-exact: integer work."""
import ctypes as C

import numpy as np
import pytest

import spades_for_blackbird_amd as B

pytestmark = pytest.mark.gpu

LANE, TILE = 4, 256  # select.h: kSelLane, kSelTile
SIZES = (0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 4096 * TILE + 3)
MIN = 1000
BEYOND = 8
SENTINEL_IDX, SENTINEL_VAL = 0x5A5A5A5A5A5A5A5A, 0xA5A5A5A5


def keep_mask(pattern, n):
    i = np.arange(n)
    if pattern == "none":
        return np.zeros(n, dtype=bool)
    if pattern == "all":
        return np.ones(n, dtype=bool)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == n - 1
    if pattern == "every_fifth":
        return i % 5 == 0
    if pattern == "half":
        return np.random.default_rng(n).random(n) < 0.5
    if pattern == "last_slot_of_tile":  # one item per tile, in the last lane's last slot
        return i % TILE == TILE - 1
    raise ValueError(pattern)


PATTERNS = ("none", "all", "first", "last", "every_fifth", "half", "last_slot_of_tile")


@pytest.fixture(scope="module")
def gpu():
    L = B.load_library()
    L.bbk_select_u32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.bbk_select_u32.restype = C.c_int
    ctx = B.Context(0)
    yield L, ctx
    ctx.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_select_against_flatnonzero(gpu, n, pattern):
    import torch
    L, ctx = gpu
    keep = keep_mask(pattern, n)
    rng = np.random.default_rng(7 * n + len(pattern))
    vals = np.where(keep, rng.integers(MIN, 1 << 32, size=n), rng.integers(0, MIN, size=n)).astype(np.uint32)
    vals = np.concatenate([vals, np.full(BEYOND, 0xFFFFFFFF, dtype=np.uint32)])  # passing values nobody may select
    exp_idx = np.flatnonzero(vals[:n] >= MIN).astype(np.uint64)
    assert np.array_equal(exp_idx, np.flatnonzero(keep))
    exp_val = vals[exp_idx.astype(np.int64)]
    d_vals = torch.from_numpy(vals.view(np.int32)).cuda()
    d_idx = torch.from_numpy(np.full(n + BEYOND, SENTINEL_IDX, dtype=np.uint64).view(np.int64)).cuda()
    d_val = torch.from_numpy(np.full(n + BEYOND, SENTINEL_VAL, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    kept = C.c_uint64(~0 & 0xFFFFFFFFFFFFFFFF)
    rc = L.bbk_select_u32(ctx._h, C.c_void_p(d_vals.data_ptr()), n, MIN, C.c_void_p(d_idx.data_ptr()),
                          C.c_void_p(d_val.data_ptr()), C.byref(kept))
    assert rc == 0, L.bbk_last_error()
    k = len(exp_idx)
    assert kept.value == k, (n, pattern, kept.value, k)
    got_idx = d_idx.cpu().numpy().view(np.uint64)
    got_val = d_val.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_idx[:k], exp_idx), (n, pattern, np.flatnonzero(got_idx[:k] != exp_idx)[:8])
    assert np.array_equal(got_val[:k], exp_val), (n, pattern, np.flatnonzero(got_val[:k] != exp_val)[:8])
    assert np.all(got_idx[k:] == SENTINEL_IDX) and np.all(got_val[k:] == SENTINEL_VAL), (n, pattern)
