// msd_stage_b.h -- what stage B (the ordering pass over a distinct key set, key slots) adds: 4-byte records after
// level 2 (k_bucket_base, k_bucket_dist_nb), level 1 read in place from stage A's buckets (BucketView) and the late
// tag (4-byte records from level 1 on).  Launched by Pass::level1_from_view, level1_late_tag, level2_scatter,
// first_pass, launch_buckets and give_up_key_slots (msd.hip); 8-byte keys only.
#pragma once

#include "msd_bucket_tail.h"

namespace bbk {

// ---- narrow stage B (8-byte keys, key slots, no payload): 4-byte records from level 2 on
// The KEYS prefix is the key's top 32 bits, p = key >> (w0bits - 32).  Bucket g = bin j of the nb bins of segment s holds
// exactly the keys whose prefix lies in [s*P + q_j, s*P + q_(j+1)), with P = 2^(32 - b1) and q_j = ceil(j * P / nb): the
// inverse of bin_of, whose bin is umulhi(q << b1, nb) = floor(q * nb / P) for the low 32 - b1 prefix bits q.  Its smallest
// key is base[g] = (s*P + q_j) << (w0bits - 32).  When no bucket spans more than 2^32 keys (ceil(P / nb) << (w0bits - 32)
// <= 2^32 for every non-empty segment: the host checks) a key of bucket g is base[g] + (uint32_t)(lo - (uint32_t)base[g]),
// lo being its low word.  So level 2 stores lo only (k_part<..., NOUT>) and k_bucket_dist_nb sorts the 32-bit offsets
// lo - (uint32_t)base[g] and widens them on the way out.  (w0bits <= 32: the key is its low word, base 0.)
__global__ void k_bucket_base(const uint32_t *__restrict__ seg_nb2, const uint32_t *__restrict__ seg_bin, uint32_t nseg,
                              uint32_t nbuckets, int b1, int w0bits, uint64_t *__restrict__ base) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nbuckets) return;
    const uint32_t lo = last_le(seg_bin, nseg, g);  // its segment (every segment has at least one bin)
    const uint64_t P = 1ull << (32 - b1), nb = seg_nb2[lo], j = g - seg_bin[lo];
    const uint64_t p = lo * P + (j * P + nb - 1) / nb;
    base[g] = w0bits > 32 ? p << (w0bits - 32) : 0ull;
}

// k_bucket_dist (OP 0, sorted result written directly) on those 4-byte records: the same distribution sort and in-bin
// ranking over 32-bit offsets, with half the LDS (38 KB against 61 KB) and at most 64 registers (62: two records per
// ranking round instead of six), so that four workgroups fit a CU instead of two.  A bucket it turns down, a duplicate or a spill
// sends the call back to the exact mode, as on the 8-byte key slots, so no second-chance kernel needs this form.
// WIDE: 16-byte loads of the first eight records of a lane (below; 57 registers), for buckets in slots.
template <int NT, int ITEMS, bool WIDE>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_bucket_dist_nb(const uint32_t *__restrict__ buf, const uint64_t *__restrict__ base,
                                                       BucketArgs A) {
    constexpr int CAP = NT * ITEMS;
    constexpr int NWAVES = NT / 64;
    constexpr int DB = DistBins<1, 0>::N;
    constexpr int BPT = DB / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: bins[DB] | scan[32] | mm[2 * NWAVES] | skeys[CAP] (offsets from the bucket's base)
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem);
    uint32_t *scan_tmp = bins + DB;
    uint32_t *mm = scan_tmp + 32;
    uint32_t *skeys = mm + 2 * NWAVES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > (uint32_t)CAP) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    for (uint32_t q = tid; q < (uint32_t)DB; q += NT) bins[q] = 0;
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#endif

    // Rows: record p = i * NT + tid lies in row i of the lane.  A bucket is planned ~70 % full, so the last rows of
    // nearly every bucket hold no record in any wave: every per-row phase below runs for i < rows only, behind a
    // branch that is uniform across the workgroup and skips the whole body.  Only the last row in use is partial.
    const uint32_t rows = bucket_rows(n, NT);
    const uint64_t kbase = base[b];
    uint32_t keys[ITEMS];  // offsets from the base: the key order
    // WIDE (bucket slots, which start on 16-byte boundaries): the first eight records of a lane arrive as two 16-byte
    // loads, item i < 8 being record (i / 4) * 4 NT + 4 tid + i % 4, and a "row" of those items is in use when its
    // group of 4 NT records is; items 8 .. ITEMS - 1 keep their rows (8 NT = 2 * 4 NT: no record twice).  The loads
    // stay unconditional, a lane past the last group of four re-reads it: up to three words behind record n - 1,
    // inside the slot's own slack, which pos(i) < n keeps out of everything below.
    static_assert(!WIDE || (ITEMS >= 8 && ITEMS <= 12), "two groups of four, then single rows");
    auto pos = [&](int i) -> uint32_t {
        return WIDE && i < 8 ? (uint32_t)(i >> 2) * (4u * NT) + 4u * (uint32_t)tid + (uint32_t)(i & 3) : (uint32_t)(i * NT + tid);
    };
    auto used = [&](int i) -> bool { return WIDE && i < 8 ? (uint32_t)(i >> 2) * (4u * NT) < n : (uint32_t)i < rows; };
    if (WIDE) {
        const uint32_t last = (n - 1u) & ~3u;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (used(4 * g)) {
                const uint32_t p = (uint32_t)g * (4u * NT) + 4u * (uint32_t)tid;
                const uint4 q = *reinterpret_cast<const uint4 *>(buf + start + (p < last ? p : last));
                keys[4 * g] = q.x, keys[4 * g + 1] = q.y, keys[4 * g + 2] = q.z, keys[4 * g + 3] = q.w;
            }
        }
    }
#pragma unroll
    for (int i = WIDE ? 8 : 0; i < ITEMS; ++i) {  // the loads of the rows in use are issued up front, the last one clamped
        if (used(i)) {
            const uint32_t p = pos(i);
            keys[i] = buf[start + (p < n ? p : n - 1u)];
        }
    }
    uint32_t mn = ~0u, mx = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {  // clamped duplicates do not change min / max
        if (used(i)) {
            keys[i] -= (uint32_t)kbase;
            if (!WIDE || pos(i) < n) {  // (a re-read last group of four may reach past n)
                mn = keys[i] < mn ? keys[i] : mn;
                mx = keys[i] > mx ? keys[i] : mx;
            }
        }
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        const uint32_t a = __shfl_xor(mn, dd, 64), c = __shfl_xor(mx, dd, 64);
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    if (lane == 0) {
        mm[2 * wave] = mn;
        mm[2 * wave + 1] = mx;
    }
    __syncthreads();  // bins zeroed, min / max of every wave visible
    mn = ~0u;
    mx = 0;
#pragma unroll
    for (int j = 0; j < NWAVES; ++j) {
        mn = mm[2 * j] < mn ? mm[2 * j] : mn;
        mx = mm[2 * j + 1] > mx ? mm[2 * j + 1] : mx;
    }
    BBK_PH(3, 0, t_prev);  // loads + min/max
    const uint32_t kmin = mn;
    const int rbits = 32 - __builtin_clz((mx - mn) | 1u);
    const int sh = rbits > DistBins<1, 0>::LOG ? rbits - DistBins<1, 0>::LOG : 0;  // digit = (offset - min) >> sh < bins

#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (used(i)) {
            const uint32_t p = pos(i);
            if (p < n) atomicAdd(&bins[(keys[i] - kmin) >> sh], 1u);
        }
    }
    __syncthreads();
    BBK_PH(3, 1, t_prev);  // count
    uint32_t c[BPT];
    uint32_t sum = 0;
    bool big = false;
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        c[q] = bins[tid * BPT + q];
        sum += c[q];
        big = big || c[q] > kDistMaxBin;
    }
    uint32_t incl = sum;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    if (__syncthreads_or(big)) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    uint32_t first = incl - sum;
    for (int j = 0; j < wave; ++j) first += scan_tmp[j];
    {
        uint32_t ex = first;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            bins[tid * BPT + q] = ex;
            ex += c[q];
        }
    }
    __syncthreads();
    BBK_PH(3, 2, t_prev);  // scan
    uint32_t at[ITEMS];  // where the scatter put the record (breaks ties between equal offsets), then its final place
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (used(i)) {
            const uint32_t p = pos(i);
            if (p < n) {
                const uint32_t pos = atomicAdd(&bins[(keys[i] - kmin) >> sh], 1u);
                skeys[pos] = keys[i];
                at[i] = pos;
            }
        }
    }
    __syncthreads();
    BBK_PH(3, 3, t_prev);  // scatter
    // in-bin ranking as in k_bucket_dist: bin d = [bins[d-1], bins[d]) after the scatter, RB records per round with the
    // first four candidates of every bin read unconditionally (one array for both places saves eleven registers).  A
    // round whose first row is not in use is skipped as a whole; inside a round there is no branch per row, so that
    // its LDS reads stay batched.
    // (RB = 6 as in k_bucket_dist: 93 registers, two workgroups per CU; 4: 80, three; 3 needs scratch at 64; 2: 62
    // registers, four workgroups per CU -- 1.42 -> 1.29 ms at the flagship size against RB = 4)
    constexpr int RB = 2;
#pragma unroll
    for (int i0 = 0; i0 < ITEMS; i0 += RB) {
        if (used(i0)) {
            uint32_t sb[RB], e[RB];
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int i = i0 + u;
                sb[u] = e[u] = 0;
                if (i < ITEMS) {
                    const uint32_t p = pos(i);
                    if (p < n) {
                        const uint32_t d = (keys[i] - kmin) >> sh;
                        sb[u] = d ? bins[d - 1] : 0u;
                        e[u] = bins[d];
                    }
                }
            }
            uint32_t o[RB][4];
#pragma unroll
            for (int u = 0; u < RB; ++u) {
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const uint32_t y = sb[u] + c4;
                    o[u][c4] = skeys[y < e[u] ? y : (e[u] ? e[u] - 1u : 0u)];
                }
            }
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int i = i0 + u;
                if (i < ITEMS) {
                    const uint32_t p = pos(i);
                    if (p < n) {
                        uint32_t before = 0;
#pragma unroll
                        for (int c4 = 0; c4 < 4; ++c4) {
                            const uint32_t y = sb[u] + c4;
                            if (y < e[u]) before += (o[u][c4] < keys[i] || (o[u][c4] == keys[i] && y < at[i])) ? 1u : 0u;
                        }
                        for (uint32_t y = sb[u] + 4; y < e[u]; ++y) {  // bins above four records
                            const uint32_t ok = skeys[y];
                            before += (ok < keys[i] || (ok == keys[i] && y < at[i])) ? 1u : 0u;
                        }
                        at[i] = sb[u] + before;
                    }
                }
            }
        }
    }
    __syncthreads();  // every rank is computed from the scattered order: only now overwrite it
    BBK_PH(3, 4, t_prev);  // rank
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (used(i)) {
            const uint32_t p = pos(i);
            if (p < n) skeys[at[i]] = keys[i];
        }
    }
    uint32_t ostart = A.out_off ? A.out_off[b] : start;
    __syncthreads();
    BBK_PH(3, 5, t_prev);  // write
    asm volatile("" : "+v"(ostart));  // awaited here, not inside the store loop (see bucket_reduce)

    // The input is distinct by construction (the caller requires the direct output, assume_distinct), and all the host
    // takes from a bucket is whether that held: the sorted offsets leave as they lie, widened, position s to dst[s]
    // (coalesced), and equal neighbours raise the duplicate flag -- no heads, no scan, no compaction.  Any duplicate
    // sends the whole call to give_up_key_slots() and the result is released, so what a bucket that holds one stores
    // inside its own [ostart, ostart + n) does not matter.  dcount is n: the bucket was sorted here.
    // (Two positions per lane and one 16-byte store for both -- half as many stores -- were measured: the kernel's
    // average fell by 2-3 %, inside its own launch range, and the form was not kept: profiles/level2_tail.)
    uint64_t *dst = reinterpret_cast<uint64_t *>(A.sorted_keys) + ostart;
    bool dup = false;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if ((uint32_t)i < rows) {
            const uint32_t s = (uint32_t)(i * NT + tid);
            if (s < n) dup = dist_tail_at(skeys, s, kbase, A.strip_mask, dst) || dup;
        }
    }
    // (one lane of a wave that saw a pair: rare, and a workgroup-wide verdict would cost one more barrier)
    if (__any(dup) && lane == 0) atomicOr(A.dup_flag, 1u);
    if (tid == 0) A.dcount[b] = n;
    BBK_PH(3, 6, t_prev);  // copy-out
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[3][7], 1ull);
#endif
}

template <int NT, int ITEMS>
static size_t bucket_dist_nb_smem() {
    return sizeof(uint32_t) * (DistBins<1, 0>::N + 32 + 2 * (NT / 64) + (size_t)NT * ITEMS);
}

// ------------------------------------------------------------------------------------------
// stage B's level 1 straight from stage A's buckets (BucketView, msd.h)
// ------------------------------------------------------------------------------------------
// Tile t of the both-strand records covers the canonical keys c in [t * TILE/2, (t+1) * TILE/2) of the dense order:
// record 2c is key c, record 2c+1 its reverse complement, as in tile_load's expand_k branch.  Key c is the 4-byte word
// slots[b * stride + c - off[b]] of the bucket b with off[b] <= c < off[b + 1], widened with the bucket's segment.
// A tile spans ~6 buckets of ~690 keys at the flagship size; their offsets and segments are staged in LDS.
constexpr int kViewSpan = 64;  // buckets of one tile staged in LDS (more: the lanes search the global table)

// largest b in [lo, hi) with off[b] <= c (off[lo] <= c).  (last_le over off + lo changes the address arithmetic of
// k_part_view and k_part_view_lt, which inline this: kept as its own loop.)
__device__ inline uint32_t view_bucket(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t c) {
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one thread per tile: the buckets of its first and last key
__global__ void k_view_tile_desc(const uint64_t *__restrict__ off, uint32_t nbuckets, uint64_t D, uint32_t keys_per_tile,
                                 uint32_t ntiles, uint2 *__restrict__ desc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const uint64_t c0 = (uint64_t)t * keys_per_tile;
    const uint64_t c1 = (c0 + keys_per_tile < D ? c0 + keys_per_tile : D) - 1u;
    const uint32_t b0 = view_bucket(off, 0, nbuckets, c0);
    desc[t] = make_uint2(b0, view_bucket(off, b0, nbuckets, c1));
}

// k_part (8-byte keys, level-1 scatter, no payload) whose tile comes from the view.  TAG: the XXH3 bucket of 16 above
// the k-mer (M.expand_tag).  Each lane loads a key once and emits it and its reverse complement as its adjacent pair.
template <bool TAG>
__global__ __launch_bounds__(PartCfg<1>::THREADS) void k_part_view(const uint32_t *__restrict__ slots,
                                                                   const uint64_t *__restrict__ off,
                                                                   const uint16_t *__restrict__ seg,
                                                                   const uint2 *__restrict__ vdesc, uint32_t stride,
                                                                   int hb, TileMap M, PartLevel L,
                                                                   uint32_t *__restrict__ cursor,
                                                                   Key<1> *__restrict__ out) {
    constexpr int kItems = PartCfg<1>::ITEMS, kTile = PartCfg<1>::TILE, kThreads = PartCfg<1>::THREADS, MAXB = 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: k_part's (lhist | lstart | goff | scan | stage) | toff[kViewSpan] | tseg[kViewSpan]
    uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
    uint32_t *lstart = lhist + MAXB;
    uint32_t *goff = lstart + MAXB;
    uint32_t *scan_tmp = goff + MAXB;
    Key<1> *stage = reinterpret_cast<Key<1> *>(scan_tmp + 32);
    uint32_t *toff = reinterpret_cast<uint32_t *>(stage + kTile);
    uint16_t *tseg = reinterpret_cast<uint16_t *>(toff + kViewSpan);
    uint32_t *vals_unused = nullptr;

    const int tid = threadIdx.x;
    const TileInfo T = tile_info(M, L, blockIdx.x, (uint32_t)kTile);
    const uint32_t count = T.count, nb = T.nb;  // count: records, even
    const uint2 d = vdesc[blockIdx.x];
    const uint32_t b0 = d.x, span = d.y - d.x + 1u;
    const bool staged = span <= (uint32_t)kViewSpan;  // uniform
    for (uint32_t b = tid; b < nb; b += kThreads) lhist[b] = 0;
    if (staged && tid < (int)span) {
        toff[tid] = (uint32_t)off[b0 + tid];  // key offsets < 2^32: one pass holds fewer records
        tseg[tid] = seg[b0 + tid];
    }
    __syncthreads();

    // item pair j of a lane = records 2c, 2c+1 of local key j * THREADS + tid (tile_local's pairs)
    const uint32_t c0 = (uint32_t)(T.begin >> 1), nkeys = count >> 1;
    uint32_t lo[kItems / 2], sg[kItems / 2];
#pragma unroll
    for (int j = 0; j < kItems / 2; ++j) {
        const uint32_t cl = (uint32_t)(j * kThreads + tid);
        const uint32_t c = c0 + (cl < nkeys ? cl : nkeys - 1u);  // clamped into the tile
        uint32_t b, base;
        if (staged) {
            uint32_t i = 0, hi = span;
            while (hi - i > 1) {
                const uint32_t mid = (i + hi) >> 1;
                if (toff[mid] <= c) i = mid;
                else hi = mid;
            }
            b = b0 + i;
            base = toff[i];
            sg[j] = tseg[i];
        } else {
            b = view_bucket(off, b0, d.y + 1u, c);
            base = (uint32_t)off[b];
            sg[j] = seg[b];
        }
        lo[j] = slots[(size_t)b * stride + (c - base)];
    }
    Key<1> keys[kItems];
    uint32_t binrank[kItems];
#pragma unroll
    for (int j = 0; j < kItems / 2; ++j) {
        Key<1> x, r;
        x.w[0] = nw_key(sg[j], lo[j], hb);
        r = kmer_rc<1>(x, M.expand_k);
        if (TAG) {
            x.w[0] |= __umul64hi(xxh3_64<1>(x), 16ull) << (2 * M.expand_k);
            r.w[0] |= __umul64hi(xxh3_64<1>(r), 16ull) << (2 * M.expand_k);
        }
        keys[2 * j] = x;
        keys[2 * j + 1] = r;
    }
    // in registers through the LDS reorder (see k_part)
#pragma unroll
    for (int i = 0; i < kItems; ++i) asm volatile("" : "+v"(keys[i].w[0]));
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const uint32_t local = tile_local<1, kThreads>(i, tid);
        binrank[i] = 0xFFFFFFFFu;
        if (local < count) {
            uint32_t pfx = prefix_of<1>(keys[i], L.dmode, L.w0bits);
            if (select_prefix(pfx, L)) {
                const uint32_t b = bin_of(pfx, L, nb);
                const uint32_t rank = atomicAdd(&lhist[b], 1u);
                binrank[i] = (b << 16) | rank;
            }
        }
    }
    __syncthreads();
    uint32_t vals[kItems] = {};
    part_tail<1, kItems, kThreads, MAXB, false, false>(keys, vals, binrank, lhist, lstart, goff, scan_tmp, stage,
                                                       vals_unused, nb, T.gbin0, L, cursor, out, nullptr, 0, 0ull);
}

static size_t part_view_smem() {
    return part_smem(1, PartCfg<1>::TILE, false, false, true) + (size_t)kViewSpan * (4 + 2);
}

// A key-slot give-up after the view's slots were released: the canonical keys again, from the level-1 records
// (both strands of every key, tag above bit 2k; odd k, so exactly one of a pair is canonical), in any order.  One
// workgroup per level-1 sub-slot; cap bounds the writes.
__global__ void k_view_recanon(const uint64_t *__restrict__ in, const uint32_t *__restrict__ seg_off,
                               const uint32_t *__restrict__ seg_size, int k, uint64_t *__restrict__ out, uint64_t cap,
                               uint32_t *__restrict__ count) {
    const uint32_t o = seg_off[blockIdx.x], n = seg_size[blockIdx.x];
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    const int lane = threadIdx.x & 63;
    for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) {  // uniform trip count: the ballot sees whole waves
        const uint32_t i = i0 + threadIdx.x;
        Key<1> x;
        x.w[0] = 0;
        bool keep = false;
        if (i < n) {
            x.w[0] = in[o + i] & mask;
            keep = !kmer_less_nucl<1>(kmer_rc<1>(x, k), x);
        }
        const uint64_t bal = __ballot(keep);
        uint32_t base = 0;
        if (lane == 0 && bal) base = atomicAdd(count, (uint32_t)__popcll(bal));
        base = __shfl(base, 0);
        const uint64_t at = (uint64_t)base + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && at < cap) out[at] = x.w[0];
    }
}

// ------------------------------------------------------------------------------------------
// stage B with the tag taken late (tagged sort of the both-strand set, fed from a BucketView, k <= 21)
// ------------------------------------------------------------------------------------------
// The tagged key is (tag: XXH3 bucket of 16) << 2k | k-mer, and the tag is a function of the k-mer.  Level 1 above
// bins by the top bits of the TAGGED key, so its records keep 37 of the 46 bits: 8 bytes each.  Here level 1 bins by the
// top ten bits of the k-mer alone (1024 segments, kMaxBins) and stores the remaining lobits = 2k - 10 <= 32 bits: 4-byte
// records, as in narrow stage A.  Level 2 knows the whole k-mer (segment, lo), takes the tag there and sends the record
// to bin tag * nsub + sub of its segment (sub: the next bits of lo, monotone, as bin_of).  Buckets then lie in memory
// as (segment, tag, sub) while the result is ordered (tag, segment, sub): the dense offsets come from a scan of the
// bucket fills gathered in that order (k_bucket_base_lt's perm).  A bucket holds lo in [q_j, q_(j+1)) of one segment
// and one tag, q_j = ceil(j * 2^lobits / nsub): fewer than 2^32 keys by construction, so level 2 stores the k-mer's low
// word and k_bucket_dist_nb sorts and widens it against base = tag << 2k | segment << lobits | q_j, unchanged.
// Both kernels share one tail, the one of k_part_reads_narrow: the staged order is bin-major, a bit per position
// marks where a non-empty bin starts, and what a store needs of its bin is one 8-byte LDS entry -- the bin of a
// staged record (ten dropped bits at level 1, a hash at level 2) is never computed twice.
constexpr int kLtThreads = 1024;  // == kMaxBins: one bin per thread in the scans
// records per lane.  Level 1: 14 336 records = 56 KB staged, 76 KB of LDS with the tables: two workgroups per CU (16
// records per lane would be 84 KB, one workgroup); a (tile, bin) run is 14 records = 56 bytes.  Level 2: as
// k_part_narrow2.
constexpr int kLt1Items = 14;
constexpr int kLt2Items = 12;

static size_t lt_smem(int items, size_t more) {
    const size_t tile = (size_t)kLtThreads * items;
    return mark_smem(tile) + tile * 4 + more;
}
// what k_part_view_lt keeps of its tile's buckets behind the stage: a word of marks per 64 keys, an entry per bucket
static size_t lt_view_tables() {
    return ((size_t)kLtThreads * kLt1Items / 2 / 64) * sizeof(MarkWord) + (size_t)kViewSpan * sizeof(uint2);
}

// the tagged key of (segment, lo): what the spill list and the give-up path need
__device__ inline uint64_t lt_tagged(uint32_t seg, uint32_t lo, int lobits, int k) {
    Key<1> x;
    x.w[0] = ((uint64_t)seg << lobits) | lo;
    return x.w[0] | (__umul64hi(xxh3_64<1>(x), 16ull) << (2 * k));
}

// bin of item i of a lane: two 16-bit bins per register, 0xFFFF = no record
template <int ITEMS>
__device__ __forceinline__ uint32_t lt_bin(const uint32_t (&bins)[ITEMS / 2], int i) {
    const uint32_t bin = (bins[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    return bin != 0xFFFFu ? bin : 0xFFFFFFFFu;
}

// Level 1.  Tile t covers the canonical keys [t * KPT, (t + 1) * KPT) of the view's dense order (DENSE: of a key array,
// the view's overflow records); a lane loads a key once and emits it and its reverse complement.  No tag here.
template <bool DENSE>
__global__ __launch_bounds__(kLtThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_part_view_lt(
    const uint32_t *__restrict__ slots, const uint64_t *__restrict__ off, const uint16_t *__restrict__ seg,
    const uint2 *__restrict__ vdesc, uint32_t stride, int hb, const uint64_t *__restrict__ dense, uint64_t nkeys_all, int k,
    PartLevel L, uint32_t *__restrict__ cursor, uint32_t *__restrict__ out) {
    constexpr int NT = kLtThreads, ITEMS = kLt1Items, KPT = NT * ITEMS / 2, VW = KPT / 64;
    static_assert(KPT % 64 == 0 && VW <= 128, "whole words of marks, two per lane of one wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MarkLds S = mark_lds<NT * ITEMS>(smem);
    // the buckets of the tile: a mark where a non-empty one starts among the tile's KPT positions, and the r-th of them
    // as (first key offset, index in the span | segment << 16) -- what bucket a key lies in is its run's rank
    MarkWord *vmw = reinterpret_cast<MarkWord *>(S.stage + NT * ITEMS);
    uint2 *vent = reinterpret_cast<uint2 *>(vmw + VW);
    const uint32_t tid = threadIdx.x;
    uint32_t xcc = 0;  // the XCD this workgroup runs on (placement is for speed only: any value gives a correct result)
    if (L.xcd_shift) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= (1u << L.xcd_shift) - 1u;
    }
    const int lobits = 2 * k - 10;
    const uint32_t lomask = lobits >= 32 ? 0xFFFFFFFFu : (1u << lobits) - 1u;
    const uint64_t c0 = (uint64_t)blockIdx.x * KPT;
    const uint64_t left = nkeys_all - c0;
    const uint32_t nkeys = left < (uint64_t)KPT ? (uint32_t)left : (uint32_t)KPT;
    uint32_t b0 = 0, span = 0;
    bool staged_tab = false;
    if (!DENSE) {
        const uint2 d = vdesc[blockIdx.x];
        b0 = d.x;
        span = d.y - d.x + 1u;
        staged_tab = span <= (uint32_t)kViewSpan;  // uniform
        if (staged_tab && tid < 64u) {
            // Wave 0 alone, ahead of the barrier below: zero, marks, prefixes.  One wave's LDS operations execute in
            // order, and the fences keep the compiler from moving them across each other.
            uint64_t o = 0, on = 0;
            uint32_t sg = 0;
            if (tid < span) {
                o = off[b0 + tid];  // key offsets < 2^32: one pass holds fewer records
                if (tid + 1u < span) on = off[b0 + tid + 1u];
                sg = seg[b0 + tid];
            }
#ifdef BBK_AB_VIEW_SEARCH  // (A/B: every bucket of the span listed, the lanes search the list)
            (void)on;
            if (tid < span) vent[tid] = make_uint2((uint32_t)o, tid | (sg << 16));
#else
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t idx = tid * 2u + (uint32_t)j;
                if (idx < (uint32_t)VW) *reinterpret_cast<uint4 *>(&vmw[idx]) = make_uint4(0u, 0u, 0u, 0u);
            }
            __threadfence_block();
            // (the span's first bucket holds the tile's first key: it is live, starts at 0 and needs no mark)
            const bool live = tid < span && view_bucket_live(tid, span, o, on);
            const unsigned long long lv = __ballot(live);
            if (live) {
                vent[__popcll(lv & ((1ull << tid) - 1ull))] = make_uint2((uint32_t)o, tid | (sg << 16));
                const uint32_t start = view_run_start(o, c0);
                if (start) atomicOr(&reinterpret_cast<uint32_t *>(vmw)[mark_slot32(start)], mark_bit32(start));
            }
            __threadfence_block();
            mark_prefix<VW>(vmw, (int)tid);
#endif
        }
    }
    mark_clear<NT * ITEMS>(S, tid);  // NT == kMaxBins
    __syncthreads();

    // all loads first (index clamped into the tile)
    uint64_t x[ITEMS / 2];
    if (DENSE) {
#pragma unroll
        for (int j = 0; j < ITEMS / 2; ++j) {
            const uint32_t cl = (uint32_t)(j * NT) + tid;
            x[j] = dense[c0 + (cl < nkeys ? cl : nkeys - 1u)];
        }
    } else {
        uint32_t w[ITEMS / 2], sg[ITEMS / 2];
#pragma unroll
        for (int j = 0; j < ITEMS / 2; ++j) {
            const uint32_t cl = (uint32_t)(j * NT) + tid;
            const uint32_t c = (uint32_t)c0 + (cl < nkeys ? cl : nkeys - 1u);
            uint32_t b, base;
            if (staged_tab) {
#ifdef BBK_AB_VIEW_SEARCH
                uint32_t i = 0, hi = span;
                while (hi - i > 1) {
                    const uint32_t mid = (i + hi) >> 1;
                    if (vent[mid].x <= c) i = mid;
                    else hi = mid;
                }
                const uint2 e = vent[i];
#else
                // the bucket of key position cl: the rank of its run (cl is NOT clamped here -- the wave's word is
                // j * 16 + wave for all its lanes; past the tile's last key there is no mark, so such a lane gets the
                // last bucket, which holds the key it is clamped to)
                const uint4 m = *reinterpret_cast<const uint4 *>(&vmw[j * (NT / 64) + (int)(tid >> 6)]);
                const uint2 e = vent[mark_rank(m.x, m.y, m.z, tid & 63u)];
#endif
                b = b0 + (e.y & 0xFFFFu);
                base = e.x;
                sg[j] = e.y >> 16;
            } else {
                b = view_bucket(off, b0, b0 + span, c);
                base = (uint32_t)off[b];
                sg[j] = seg[b];
            }
            w[j] = slots[(size_t)b * stride + (c - base)];
        }
#pragma unroll
        for (int j = 0; j < ITEMS / 2; ++j) x[j] = nw_key(sg[j], w[j], hb);
    }
    uint32_t lo[ITEMS], bins[ITEMS / 2];
#pragma unroll
    for (int j = 0; j < ITEMS / 2; ++j) {
        Key<1> a;
        a.w[0] = x[j];
        const uint64_t r = kmer_rc<1>(a, k).w[0];
        const uint32_t ba = (uint32_t)(x[j] >> lobits), br = (uint32_t)(r >> lobits);  // k-mers < 4^k: bins < 1024
        lo[2 * j] = (uint32_t)x[j] & lomask;
        lo[2 * j + 1] = (uint32_t)r & lomask;
        bins[j] = 0xFFFFFFFFu;
        if ((uint32_t)(j * NT) + tid < nkeys) {
            bins[j] = ba | (br << 16);
            atomicAdd(&S.lhist[ba], 1u);  // count only: the place inside the bin is taken after the scan
            atomicAdd(&S.lhist[br], 1u);
        }
    }
    __syncthreads();
    const uint64_t slot_end = (uint64_t)tid * L.slot_stride + (L.xcd_shift ? (uint64_t)(xcc + 1u) * L.sub_cap : (uint64_t)L.slot_cap);
    mark_tail<NT * ITEMS, ITEMS, false>(
        S, lo, tid, (uint32_t)kMaxBins, &cursor[(tid << L.xcd_shift) + xcc], slot_end, 0u, L, out, nullptr,
        [&](int i) { return lt_bin<ITEMS>(bins, i); }, [](int) { return 0u; },
        [&](uint32_t bin, uint32_t rec) { return lt_tagged(bin, rec, lobits, k); }, []() {});
}

// Level 2: one tile of one segment's sub-slot (k_tile_desc<true>'s descriptors) -> the buckets of that segment.  The
// tag is taken here, once per record.
__global__ __launch_bounds__(kLtThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_part_lt2(
    const uint32_t *__restrict__ in, const uint4 *__restrict__ desc, int k, PartLevel L, uint32_t *__restrict__ cursor,
    uint32_t *__restrict__ out) {
    constexpr int NT = kLtThreads, ITEMS = kLt2Items;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MarkLds S = mark_lds<NT * ITEMS>(smem);
    const uint32_t tid = threadIdx.x;
    const uint4 d = desc[blockIdx.x];  // first record, records, bins of the segment | segment << 16, flat index of bin 0
    const uint32_t begin = d.x, count = d.y, nb = d.z & 0xFFFFu, sgm = d.z >> 16, gbin0 = d.w;
    if (count == 0) return;  // an unused place of the XCD-wise order (k_tile_desc)
    const int lobits = 2 * k - 10;
    const uint32_t nsub = nb >> 4;
    const uint64_t segbits = (uint64_t)sgm << lobits;
    mark_clear<NT * ITEMS>(S, tid);  // NT == kMaxBins
    __syncthreads();
    uint32_t lo[ITEMS], bins[ITEMS / 2];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {  // all loads first (index clamped into the tile)
        const uint32_t local = (uint32_t)i * NT + tid;
        lo[i] = in[begin + (local < count ? local : count - 1u)];
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) asm volatile("" : "+v"(lo[i]));
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        Key<1> x;
        x.w[0] = segbits | lo[i];
        const uint32_t tag = (uint32_t)__umul64hi(xxh3_64<1>(x), 16ull);
        const uint32_t b = tag * nsub + __umulhi(lo[i] << (32 - lobits), nsub);
        const bool valid = (uint32_t)i * NT + tid < count;
        if (valid) atomicAdd(&S.lhist[b], 1u);
        const uint32_t b16 = valid ? b : 0xFFFFu;
        if (i & 1) bins[i >> 1] |= b16 << 16;
        else bins[i >> 1] = b16;
    }
    __syncthreads();
    const uint64_t slot_end = (uint64_t)(gbin0 + tid) * L.slot_stride + L.slot_cap;
    mark_tail<NT * ITEMS, ITEMS, false>(
        S, lo, tid, nb, &cursor[gbin0 + tid], slot_end, (uint32_t)segbits, L, out, nullptr,
        [&](int i) { return lt_bin<ITEMS>(bins, i); }, [](int) { return 0u; },
        [&](uint32_t, uint32_t rec) { return lt_tagged(sgm, rec, lobits, k); }, []() {});
}

// one thread per bucket g = bin tag * nsub + j of segment s: its smallest tagged key, and its place in the order of the
// result, (tag, segment, sub) -- the segments' bin counts are multiples of 16, so a tag owns nbuckets / 16 places
__global__ void k_bucket_base_lt(const uint32_t *__restrict__ seg_nb2, const uint32_t *__restrict__ seg_bin, uint32_t nseg,
                                 uint32_t nbuckets, int lobits, int k, uint64_t *__restrict__ base,
                                 uint32_t *__restrict__ perm) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nbuckets) return;
    const uint32_t lo = last_le(seg_bin, nseg, g);  // its segment (every segment has at least one bin)
    const uint32_t nsub = seg_nb2[lo] >> 4, r = g - seg_bin[lo], tag = r / nsub, j = r - tag * nsub;
    const uint64_t q = (((uint64_t)j << lobits) + nsub - 1u) / nsub;
    base[g] = ((uint64_t)tag << (2 * k)) | ((uint64_t)lo << lobits) | q;
    perm[g] = tag * (nbuckets >> 4) + (seg_bin[lo] >> 4) + j;
}

// the slot fills (as SCAN_SLOT_FILL reads them from the cursors) in the order of the result
__global__ void k_lt_fill_perm(const uint32_t *__restrict__ cursor, const uint32_t *__restrict__ perm, uint32_t n,
                               uint32_t stride, uint32_t cap, uint32_t *__restrict__ fill) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t c = cursor[g] - g * stride;
    fill[perm[g]] = c < cap ? c : cap;
}

// ... and their exclusive scan back at the buckets
__global__ void k_lt_unperm(const uint64_t *__restrict__ scanned, const uint32_t *__restrict__ perm, uint32_t n,
                            uint32_t *__restrict__ out_off) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) out_off[g] = (uint32_t)scanned[perm[g]];
}

// k_view_recanon over the 4-byte level-1 records: the segment comes from the sub-slot, lo from the record
__global__ void k_view_recanon_lt(const uint32_t *__restrict__ in, const uint32_t *__restrict__ seg_off,
                                  const uint32_t *__restrict__ seg_size, int sub_shift, int k, uint64_t *__restrict__ out,
                                  uint64_t cap, uint32_t *__restrict__ count) {
    const uint32_t o = seg_off[blockIdx.x], n = seg_size[blockIdx.x];
    const uint64_t segbits = (uint64_t)(blockIdx.x >> sub_shift) << (2 * k - 10);
    const int lane = threadIdx.x & 63;
    for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) {  // uniform trip count: the ballot sees whole waves
        const uint32_t i = i0 + threadIdx.x;
        Key<1> x;
        x.w[0] = 0;
        bool keep = false;
        if (i < n) {
            x.w[0] = segbits | in[o + i];
            keep = !kmer_less_nucl<1>(kmer_rc<1>(x, k), x);
        }
        const uint64_t bal = __ballot(keep);
        uint32_t base = 0;
        if (lane == 0 && bal) base = atomicAdd(count, (uint32_t)__popcll(bal));
        base = __shfl(base, 0);
        const uint64_t at = (uint64_t)base + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && at < cap) out[at] = x.w[0];
    }
}

void BucketView::materialise(bbk_ctx *ctx) {
    if (!live()) return;
    keys.alloc(n() * 8 + 16);
    if (nbuckets) {
        KernelTimer t(ctx, "compact", (double)D * (4 + 8));
        hipLaunchKernelGGL(k_compact_narrow<false>, dim3((unsigned)(((uint64_t)nbuckets * 64 + 255) / 256)), dim3(256), 0,
                           ctx->stream, slots.as<uint32_t>(), nullptr, dcount.as<uint32_t>(), off.as<uint64_t>(), nbuckets,
                           stride, seg.as<uint16_t>(), hb, keys.as<uint64_t>(), nullptr);
        check_launch("compact");
    }
    if (n_extra)
        BBK_HIP(bbk::copy_async(keys.as<uint64_t>() + D, extra.p, n_extra * 8, hipMemcpyDeviceToDevice, ctx->stream));
    stream_wait(ctx);
    release_slots();
}

}  // namespace bbk
