// msd_bucket.h -- one workgroup per bucket in LDS (every route's last step on 8-byte and wider records): the sorting
// kernels k_bucket_dist / k_bucket, the hash dedup k_bucket_hash / k_bucket_hashidx, the compaction and the small
// per-bucket planning kernels.  Launched by Pass::level2_scatter, first_pass, overflow and compact (msd.hip).
#pragma once

namespace bbk {

// ------------------------------------------------------------------------------------------
// bucket kernel
// ------------------------------------------------------------------------------------------
__device__ inline uint64_t match8(uint32_t d, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

struct BucketArgs {
    const uint32_t *boff;        // nbuckets + 1 record offsets
    uint32_t *dcount;            // distinct per bucket; 0xFFFFFFFF = overflow (left untouched)
    const uint32_t *bucket_ids;  // null: bucket = blockIdx.x; else the list of buckets to process
    int k;
    uint32_t *dbg;               // optional counters (BBK_VERBOSE): [0] buckets that took the all-words fallback
    // slot mode: bucket b lies at [b*slot_cap, b*slot_cap + min(reserved, slot_cap)), reserved = cursor[b] - b*slot_cap;
    // a bucket that reserved more than its slot is left alone (dcount = 0xFFFFFFFF): the host reprocesses it together
    // with the spill list
    uint32_t slot_cap, slot_stride;
    const uint32_t *cursor;
    // (the hash-dedup kernels write the distinct records back to the head of their bucket; until round 3 they could also
    // reserve a place in the dense result with an atomicAdd on one counter -- 2.6 ms for the 227 210 buckets of BASELINE
    // configs[1], tools/probes/single_counter_probe.hip)
    // sorting kernels, input known to hold (almost certainly) no duplicates: bucket b's records go straight to
    // sorted_keys[boff[b] ...] (the dense result: same offsets as the input when nothing is removed), word 0 masked
    // with strip_mask; a bucket that did remove a duplicate raises *dup_flag and the caller redoes the pass in place
    void *sorted_keys;
    uint32_t *sorted_vals;
    uint32_t *dup_flag;
    uint64_t strip_mask;
    // hash-dedup kernels: a probe sequence longer than this means the table is (nearly) full and the bucket is left to
    // the caller (kHashMaxProbes; tests lower it through BBK_HASH_MAX_PROBES to force that path on half-empty slots)
    uint32_t max_probes;
    // sorting kernels reading slots (stage B without histograms): bucket b's sorted records go to sorted_keys[out_off[b]
    // ...] (exclusive scan of the slot fills); null: the dense layout, output offset = input offset
    const uint32_t *out_off;
};

// first record and record count of bucket b (count 0xFFFFFFFF: the slot overflowed)
__device__ inline void bucket_range(const BucketArgs &A, uint32_t b, uint32_t *start, uint32_t *n) {
    if (A.slot_cap) {
        *start = b * A.slot_stride;
        const uint32_t reserved = A.cursor[b] - *start;
        *n = reserved > A.slot_cap ? 0xFFFFFFFFu : reserved;
    } else {
        *start = A.boff[b];
        *n = A.boff[b + 1] - *start;
    }
}

// ODD on purpose: in the blocked phases thread t reads records t*ITEMS + i, i.e. lanes are ITEMS*W*2
// dwords apart; with an even ITEMS that stride is a multiple of 16 dwords and a wave hits 2-4 LDS banks
// (16- to 32-way conflicts); with an odd ITEMS the ds_read_b64/b128 of a lane group are conflict-free.
// First pass (k_bucket_dist): 512 threads x 11 records of 8 bytes (CAP 5632), x 7 of 16 bytes (CAP 3584) -- two
// workgroups per CU and few records per lane (the kernel is issue-bound: 256 x 23 was 20 % slower, 512 x 11
// records of 16 bytes, one workgroup per CU, 75 % slower).  Second chance (k_bucket, radix): 512 x 23 / 512 x 11.
template <int W>
struct BktCfg {
#ifndef BBK_BKT_NT
#define BBK_BKT_NT 512
#define BBK_BKT_ITEMS 11
#endif
#ifndef BBK_BKT2_NT
#define BBK_BKT2_NT 512
#define BBK_BKT2_ITEMS 7
#endif
    static constexpr int NT = (W == 1) ? BBK_BKT_NT : BBK_BKT2_NT;
    static constexpr int ITEMS = (W == 1) ? BBK_BKT_ITEMS : (W == 2 ? BBK_BKT2_ITEMS : (W == 3 ? 5 : 3));
    static constexpr uint32_t CAP = NT * ITEMS;
    static constexpr int NT2 = 512;                               // second-chance kernel
    static constexpr int ITEMS2 = (W == 1) ? 23 : (W == 2 ? 11 : (W == 3 ? 7 : 5));
    static constexpr uint32_t CAP2 = NT2 * ITEMS2;
};
// mean bucket = 0.70 CAP: a bucket holds ~100 distinct genomic k-mers x their multiplicity (~40 at 50x
// coverage), so its size varies far more than Poisson on the record count would suggest
constexpr double kBucketFill = 0.70;

// OP: 0 unique only, 1 COUNT (run length), 2 SUM of vals, 3 OR of vals.  NT threads, CAP = NT * ITEMS.
// Heads + segmented reduce of a bucket that lies sorted in LDS (skeys[0, n), svals alongside when the records
// carry a payload); the distinct records are written back in place at buf[start ...], their reduced payloads
// to vals, the count to dcount[b].  Blocked ownership: thread t owns [t*ITEMS, (t+1)*ITEMS).
template <int W, int NT, int ITEMS, int OP>
__device__ __forceinline__ void bucket_reduce(Key<W> *skeys, uint32_t *svals, uint32_t *scan_tmp, uint32_t n, uint32_t start,
                                              uint32_t b, Key<W> *__restrict__ buf, uint32_t *__restrict__ vals,
                                              const BucketArgs &A) {
    constexpr int NWAVES = NT / 64;
    constexpr bool IN_VAL = OP >= 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t ostart = (A.sorted_keys && A.out_off) ? A.out_off[b] : start;  // where the sorted records go
    Key<W> mine[ITEMS];
    uint32_t mv[ITEMS];
    const uint32_t p0 = (uint32_t)tid * ITEMS;
    Key<W> prev;
#pragma unroll
    for (int j = 0; j < W; ++j) prev.w[j] = ~0ull;  // cannot equal a real key: unused high bits are 0
    if (p0 > 0 && p0 - 1 < n) prev = key_load<W>(&skeys[p0 - 1]);
    uint32_t nheads = 0;
    uint32_t headbits = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
#pragma unroll
        for (int j = 0; j < W; ++j) mine[i].w[j] = 0;
        mv[i] = 0;
        if (p0 + i < n) {
            mine[i] = key_load<W>(&skeys[p0 + i]);
            if (IN_VAL) mv[i] = svals[p0 + i];
            const bool h = (i == 0) ? !key_eq<W>(mine[0], prev) : !key_eq<W>(mine[i], mine[i - 1]);
            if (h) {
                headbits |= 1u << i;
                ++nheads;
            }
        }
    }
    uint32_t excl, total;
    {
        uint32_t incl = nheads;
        incl = wave_scan_incl(incl);
        __syncthreads();  // everyone has its keys in registers: skeys may be reused below
        if (lane == 63) scan_tmp[wave] = incl;
        __syncthreads();
        uint32_t wbase, tot;
        wave_totals<NWAVES>(scan_tmp, lane, wave, wbase, tot);
        excl = wbase + incl - nheads;
        total = tot;
        // the loaded offset is awaited HERE by every lane: left to the compiler, the wait (vmcnt 0) lands in the
        // conditional blocks of the store loop below and makes every store wait for the one before
        asm volatile("" : "+v"(ostart));
    }
#ifndef BBK_AB_BLOCKED_REDUCE  // (A/B: -DBBK_AB_BLOCKED_REDUCE stores straight from the blocked ownership, as before round 3)
    if constexpr (OP == 0) {
        // No payload: the distinct keys go back into LDS at their place in the result (a place at or before the thread's
        // own records, all of which are in registers by now) and leave it with coalesced stores -- 512 contiguous bytes
        // per wave instruction.  Straight from the blocked ownership every lane stored its ITEMS keys 8 ITEMS bytes from
        // its neighbour's: 64 separate pieces per instruction.
        int seg = (int)excl - 1;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            if (p0 + i < n && (headbits & (1u << i))) {
                ++seg;
                Key<W> kx = mine[i];
                if (A.sorted_keys) kx.w[0] &= A.strip_mask;
                key_store<W>(&skeys[seg], kx);
            }
        }
        __syncthreads();
        Key<W> *dstk = A.sorted_keys ? reinterpret_cast<Key<W> *>(A.sorted_keys) + ostart : buf + start;
        for (uint32_t s = tid; s < total; s += NT) key_store<W>(&dstk[s], key_load<W>(&skeys[s]));
        if (tid == 0 && A.sorted_keys && total != n) atomicOr(A.dup_flag, 1u);
        if (tid == 0) A.dcount[b] = total;
        return;
    }
#endif
    uint32_t *acc = reinterpret_cast<uint32_t *>(skeys);  // CAP u32 fit in the key buffer
    if (OP != 0) {
        for (uint32_t s = tid; s < total; s += NT) acc[s] = 0;
        __syncthreads();
    }
    {
        int seg = (int)excl - 1;  // segment of the records before my first head
        uint32_t a = 0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            if (p0 + i < n) {
                if (headbits & (1u << i)) {
                    if (OP != 0 && any) {
                        if (OP == 3) atomicOr(&acc[seg], a);
                        else atomicAdd(&acc[seg], a);
                    }
                    ++seg;
                    a = 0;
                    if (A.sorted_keys) {
                        Key<W> kx = mine[i];
                        kx.w[0] &= A.strip_mask;
                        key_store<W>(&reinterpret_cast<Key<W> *>(A.sorted_keys)[ostart + (uint32_t)seg], kx);
                    } else {
                        key_store<W>(&buf[start + (uint32_t)seg], mine[i]);  // distinct keys, in place
                    }
                }
                any = true;
                if (OP == 1) a += 1;
                else if (OP == 2) a += mv[i];
                else if (OP == 3) a |= mv[i];
            }
        }
        if (OP != 0 && any) {
            if (OP == 3) atomicOr(&acc[seg], a);
            else atomicAdd(&acc[seg], a);
        }
    }
    if (OP != 0) {
        __syncthreads();
        uint32_t *vdst = A.sorted_keys ? A.sorted_vals : vals;
        const uint32_t vstart = A.sorted_keys ? ostart : start;
        for (uint32_t s = tid; s < total; s += NT) vdst[vstart + s] = acc[s];
    }
    if (tid == 0 && A.sorted_keys && total != n) atomicOr(A.dup_flag, 1u);
    if (tid == 0) A.dcount[b] = total;
}

template <int W, int NT, int ITEMS, int OP>
__global__ __launch_bounds__(NT) void k_bucket(Key<W> *__restrict__ buf, uint32_t *__restrict__ vals, BucketArgs A) {
    constexpr int CAP = NT * ITEMS;
    constexpr int NWAVES = NT / 64;
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: wave_cnt[NWAVES][256] | dstart[256] | scan[32] | skeys[CAP] | svals[CAP] (IN_VAL)
    uint32_t(*wave_cnt)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
    uint32_t *dstart = reinterpret_cast<uint32_t *>(smem) + NWAVES * 256;
    uint32_t *scan_tmp = dstart + 256;
    Key<W> *skeys = reinterpret_cast<Key<W> *>(scan_tmp + 32);
    uint32_t *svals = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(skeys) + sizeof(Key<W>) * CAP);

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
    {
        // all loads first (unconditional, index clamped into the bucket), then the LDS stores: a load inside the
        // `p < n` branch is waited for before the next one is issued -- one memory latency per record
        Key<W> rk[ITEMS];
        uint32_t rv[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            const uint32_t at = start + (p < n ? p : n - 1u);
            rk[i] = key_load<W>(&buf[at]);
            rv[i] = IN_VAL ? vals[at] : 0u;
        }
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            if (p < n) {
                key_store<W>(&skeys[p], rk[i]);
                if (IN_VAL) svals[p] = rv[i];
            }
        }
    }
    __syncthreads();

    // ---- LSD radix sort inside LDS.  Only word 0 is radix-sorted, and only over the bits in which the
    // bucket's keys differ (keys of a KEYS-mode bucket share their top ~16 bits): subtract the bucket
    // minimum, sort the bits of (max - min).  Wider keys then order the (short) runs of equal word 0 by
    // their remaining words with an insertion sort; a bucket with a long run (> 48 keys sharing 32
    // bases) falls back to radix passes over every word.
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int lastbits = 2 * A.k - 64 * (W - 1);
    uint64_t kmin = 0;
    int sortbits = (W == 1) ? lastbits : 64;
    {
        uint64_t mn = ~0ull, mx = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            if (p < n) {
                const uint64_t x = skeys[p].w[0];
                mn = x < mn ? x : mn;
                mx = x > mx ? x : mx;
            }
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            const uint64_t a = __shfl_xor(mn, dd, 64), c = __shfl_xor(mx, dd, 64);
            mn = a < mn ? a : mn;
            mx = c > mx ? c : mx;
        }
        uint64_t *mm = reinterpret_cast<uint64_t *>(wave_cnt);  // counters are not live yet
        if (lane == 0) {
            mm[2 * wave] = mn;
            mm[2 * wave + 1] = mx;
        }
        __syncthreads();
        mn = ~0ull;
        mx = 0;
        for (int j = 0; j < NWAVES; ++j) {
            mn = mm[2 * j] < mn ? mm[2 * j] : mn;
            mx = mm[2 * j + 1] > mx ? mm[2 * j + 1] : mx;
        }
        __syncthreads();
        kmin = mn;
        sortbits = 64 - __builtin_clzll((mx - mn) | 1ull);
    }
    // stable radix passes over bits [0, nbits) of (word `wsel` - base)
    auto radix_passes = [&](int wsel, uint64_t base, int nbits) {
        for (int shift = 0; shift < nbits; shift += 8) {
            Key<W> keys[ITEMS];
            uint32_t v[ITEMS];
            uint32_t dr[ITEMS];  // digit << 16 | rank-in-wave
            if (tid < 256) {
#pragma unroll
                for (int j = 0; j < NWAVES; ++j) wave_cnt[j][tid] = 0;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t p = (uint32_t)(wave * (ITEMS * 64) + i * 64 + lane);
                const bool valid = p < n;
                uint32_t d = 0;
#pragma unroll
                for (int j = 0; j < W; ++j) keys[i].w[j] = 0;
                v[i] = 0;
                if (valid) {
                    keys[i] = key_load<W>(&skeys[p]);
                    if (IN_VAL) v[i] = svals[p];
                    const uint64_t word = (W == 1) ? keys[i].w[0]
                                                   : reinterpret_cast<const uint64_t *>(&skeys[p])[wsel];
                    d = (uint32_t)((word - base) >> shift) & 0xFFu;
                }
                const uint64_t peers = match8(d, valid);
                const uint32_t pre = wave_cnt[wave][d];
                dr[i] = (d << 16) | (pre + (uint32_t)__popcll(peers & lt_mask));
                if (valid && (peers >> lane) == 1ull) wave_cnt[wave][d] = pre + (uint32_t)__popcll(peers);
            }
            __syncthreads();
            {
                uint32_t tot = 0, incl = 0;
                if (tid < 256) {
#pragma unroll
                    for (int j = 0; j < NWAVES; ++j) {
                        const uint32_t c = wave_cnt[j][tid];
                        wave_cnt[j][tid] = tot;
                        tot += c;
                    }
                    incl = tot;
                    incl = wave_scan_incl(incl);
                    if (lane == 63) scan_tmp[wave] = incl;
                }
                __syncthreads();
                if (tid < 256) {
                    uint32_t wbase = 0;
                    for (int j = 0; j < wave; ++j) wbase += scan_tmp[j];
                    dstart[tid] = wbase + incl - tot;
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t p = (uint32_t)(wave * (ITEMS * 64) + i * 64 + lane);
                if (p < n) {
                    const uint32_t d = dr[i] >> 16;
                    const uint32_t pos = dstart[d] + wave_cnt[wave][d] + (dr[i] & 0xFFFFu);
                    key_store<W>(&skeys[pos], keys[i]);
                    if (IN_VAL) svals[pos] = v[i];
                }
            }
            __syncthreads();
        }
    };
    radix_passes(0, kmin, sortbits);
    if (W >= 2) {
        // runs of equal word 0: the thread that owns a run's first record orders the run by words 1..W-1
        bool bad = false;
        const uint32_t q0 = (uint32_t)tid * ITEMS;
        for (uint32_t p = q0; p < q0 + ITEMS && p < n; ++p) {
            const uint64_t w0 = skeys[p].w[0];
            if (p > 0 && skeys[p - 1].w[0] == w0) continue;  // not a run start
            uint32_t e = p + 1;
            while (e < n && skeys[e].w[0] == w0) ++e;
            if (e - p <= 1) continue;
            if (e - p > 48) {
                bad = true;
                continue;
            }
            for (uint32_t x = p + 1; x < e; ++x) {
                const Key<W> kx = key_load<W>(&skeys[x]);
                const uint32_t vx = IN_VAL ? svals[x] : 0u;
                uint32_t y = x;
                while (y > p) {
                    const Key<W> ky = key_load<W>(&skeys[y - 1]);
                    if (!key_less_words<W>(kx, ky)) break;
                    key_store<W>(&skeys[y], ky);
                    if (IN_VAL) svals[y] = svals[y - 1];
                    --y;
                }
                key_store<W>(&skeys[y], kx);
                if (IN_VAL) svals[y] = vx;
            }
        }
        if (__syncthreads_or(bad)) {
            if (A.dbg && tid == 0) atomicAdd(&A.dbg[0], 1u);
            for (int w = W - 1; w >= 0; --w) radix_passes(w, 0ull, (w == W - 1) ? lastbits : 64);
        }
    }

    bucket_reduce<W, NT, ITEMS, OP>(skeys, svals, scan_tmp, n, start, b, buf, vals, A);
}

// ---- first-choice bucket kernel: ONE distribution pass instead of ballot-ranked radix passes.
// The records of a bucket are spread evenly over its key range (KEYS/REF mode: a contiguous range of k-mers
// of a genome), so DistBins::N bins over the top bits of (word 0 - bucket minimum) hold about one record
// each: count with LDS atomics, scan, scatter with returning atomics (the order inside a bin is arbitrary),
// then the owner of a bin puts it in order by insertion on the whole key.  A bin above kDistMaxBin (skewed
// keys, a k-mer repeated hundreds of times in an unreduced stream) marks the bucket as overflowing and the
// host hands it to k_bucket, which takes any distribution.
// 4096 bins; wide keys WITH a payload: 2048, so that keys + payloads + bins stay below 80 KB and TWO workgroups fit a CU
// (16-byte keys: 57 + 14 + 8 KB).  With 4096 bins the sort of an extension index of 16-byte keys (k-mer + edge mask) ran
// one workgroup per CU: 8.1 ms against 5.0 ms for 257 M records.  (8-byte keys with a payload stay at 4096 bins and
// one workgroup per CU: with 5632 records per bucket the fuller bins cost more than the second workgroup gains.)
template <int W, int OP>
struct DistBins {
    static constexpr int N = (W >= 2 && OP >= 2) ? 2048 : 4096;
    static constexpr int LOG = (W >= 2 && OP >= 2) ? 11 : 12;
};
constexpr uint32_t kDistMaxBin = 96;  // equal keys insert in linear time; only distinct keys cost n^2

template <int W, int NT, int ITEMS, int OP>
__global__ __launch_bounds__(NT) void k_bucket_dist(Key<W> *__restrict__ buf, uint32_t *__restrict__ vals, BucketArgs A) {
    constexpr int CAP = NT * ITEMS;
    constexpr int NWAVES = NT / 64;
    constexpr int DB = DistBins<W, OP>::N;
    constexpr int BPT = DB / NT;
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: bins[DB] | scan[32] | mm[2 * NWAVES] (u64) | skeys[CAP] | svals[CAP] (IN_VAL)
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem);
    uint32_t *scan_tmp = bins + DB;
    uint64_t *mm = reinterpret_cast<uint64_t *>(scan_tmp + 32);
    Key<W> *skeys = reinterpret_cast<Key<W> *>(mm + 2 * NWAVES);
    uint32_t *svals = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(skeys) + sizeof(Key<W>) * CAP);

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

    // records of this thread (striped over the bucket); all loads issued before the first use
    Key<W> keys[ITEMS];
    uint32_t v[IN_VAL ? ITEMS : 1];
    uint64_t mn = ~0ull, mx = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        const uint32_t at = start + (p < n ? p : n - 1u);
        keys[i] = key_load<W>(&buf[at]);
        if (IN_VAL) v[i] = vals[at];
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {  // clamped duplicates do not change min / max
        const uint64_t x = keys[i].w[0];
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        const uint64_t a = __shfl_xor(mn, dd, 64), c = __shfl_xor(mx, dd, 64);
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    if (lane == 0) {
        mm[2 * wave] = mn;
        mm[2 * wave + 1] = mx;
    }
    __syncthreads();  // bins zeroed, min / max of every wave visible
    mn = ~0ull;
    mx = 0;
#pragma unroll
    for (int j = 0; j < NWAVES; ++j) {
        mn = mm[2 * j] < mn ? mm[2 * j] : mn;
        mx = mm[2 * j + 1] > mx ? mm[2 * j + 1] : mx;
    }
    BBK_PH(3, 0, t_prev);  // loads + min/max
    const uint64_t kmin = mn;
    const int rbits = 64 - __builtin_clzll((mx - mn) | 1ull);
    const int sh = rbits > DistBins<W, OP>::LOG ? rbits - DistBins<W, OP>::LOG : 0;  // digit = (word 0 - min) >> sh < bins

#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        if (p < n) atomicAdd(&bins[(uint32_t)((keys[i].w[0] - kmin) >> sh)], 1u);
    }
    __syncthreads();
    BBK_PH(3, 1, t_prev);  // count
    // exclusive scan of the bins; thread t owns bins [t*BPT, (t+1)*BPT)
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
    if (__syncthreads_or(big)) {  // nothing has been written: the second-chance kernel takes the bucket
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
    uint32_t pos_of[ITEMS];  // where the scatter put the record (breaks ties between equal keys)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        pos_of[i] = 0;
        if (p < n) {
            const uint32_t pos = atomicAdd(&bins[(uint32_t)((keys[i].w[0] - kmin) >> sh)], 1u);
            key_store<W>(&skeys[pos], keys[i]);
            pos_of[i] = pos;
        }
    }
    __syncthreads();
    BBK_PH(3, 3, t_prev);  // scatter
    // order inside the bins, record-parallel: a record's final place is its bin's start plus the number of
    // records of the bin that go before it (smaller key; equal key: scattered to a lower position).  After the
    // scatter bins[d] is the END of bin d, so bin d = [bins[d-1], bins[d]).
    // Batched so that the LDS reads of several records are in flight together (one record at a time is three
    // dependent LDS round trips: bin bounds, candidates, compare): RB records per round, the first four candidates
    // of every bin read unconditionally; the rare fuller bins finish in a loop.
    uint32_t dest[ITEMS];
    if constexpr (W == 1) {
        constexpr int RB = 6;
    #pragma unroll
        for (int i0 = 0; i0 < ITEMS; i0 += RB) {
            uint32_t sb[RB], e[RB];
    #pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int i = i0 + u;
                sb[u] = e[u] = 0;
                if (i < ITEMS) {
                    const uint32_t p = (uint32_t)(i * NT + tid);
                    if (p < n) {
                        const uint32_t d = (uint32_t)((keys[i].w[0] - kmin) >> sh);
                        sb[u] = d ? bins[d - 1] : 0u;
                        e[u] = bins[d];
                    }
                }
            }
            Key<W> o[RB][4];
    #pragma unroll
            for (int u = 0; u < RB; ++u) {
    #pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t y = sb[u] + c;
                    o[u][c] = key_load<W>(&skeys[y < e[u] ? y : (e[u] ? e[u] - 1u : 0u)]);
                }
            }
    #pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int i = i0 + u;
                if (i < ITEMS) {
                    dest[i] = 0xFFFFFFFFu;
                    const uint32_t p = (uint32_t)(i * NT + tid);
                    if (p < n) {
                        uint32_t before = 0;
    #pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const uint32_t y = sb[u] + c;
                            if (y < e[u]) {
                                const bool lt = key_less_words<W>(o[u][c], keys[i]);
                                const bool eq = key_eq<W>(o[u][c], keys[i]);
                                before += (lt || (eq && y < pos_of[i])) ? 1u : 0u;
                            }
                        }
                        for (uint32_t y = sb[u] + 4; y < e[u]; ++y) {  // bins above four records
                            const Key<W> ok = key_load<W>(&skeys[y]);
                            const bool lt = key_less_words<W>(ok, keys[i]);
                            const bool eq = key_eq<W>(ok, keys[i]);
                            before += (lt || (eq && y < pos_of[i])) ? 1u : 0u;
                        }
                        dest[i] = sb[u] + before;
                    }
                }
            }
        }
    } else {
        // wider keys: one record at a time, four candidates in flight (the batched form costs more registers than
        // it saves: measured 8 % slower for 16-byte keys)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            dest[i] = 0xFFFFFFFFu;
            if (p < n) {
                const uint32_t d = (uint32_t)((keys[i].w[0] - kmin) >> sh);
                const uint32_t sb = d ? bins[d - 1] : 0u, e = bins[d];
                uint32_t before = 0;
                if (e - sb > 1) {
                    for (uint32_t y = sb; y < e; y += 4) {
                        Key<W> o[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) o[u] = key_load<W>(&skeys[y + u < e ? y + u : e - 1]);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if (y + u < e) {
                                const bool lt = key_less_words<W>(o[u], keys[i]);
                                const bool eq = key_eq<W>(o[u], keys[i]);
                                before += (lt || (eq && y + u < pos_of[i])) ? 1u : 0u;
                            }
                        }
                    }
                }
                dest[i] = sb + before;
            }
        }
    }
    __syncthreads();  // every rank is computed from the scattered order: only now overwrite it
    BBK_PH(3, 4, t_prev);  // rank
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (dest[i] != 0xFFFFFFFFu) {
            key_store<W>(&skeys[dest[i]], keys[i]);
            if (IN_VAL) svals[dest[i]] = v[i];
        }
    }
    __syncthreads();
    BBK_PH(3, 5, t_prev);  // write
    bucket_reduce<W, NT, ITEMS, OP>(skeys, svals, scan_tmp, n, start, b, buf, vals, A);
    BBK_PH(3, 6, t_prev);  // heads + reduce + output
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[3][7], 1ull);
#endif
}

template <int W, int NT, int ITEMS, int OP>
static size_t bucket_dist_smem() {
    return sizeof(uint32_t) * (DistBins<W, OP>::N + 32) + sizeof(uint64_t) * 2 * (NT / 64) + (size_t)W * 8 * NT * ITEMS +
           (OP >= 2 ? 4 * NT * ITEMS : 0);
}

template <int W, int NT, int ITEMS, int OP>
static size_t bucket_smem() {
    return sizeof(uint32_t) * ((NT / 64) * 256 + 256 + 32) + (size_t)W * 8 * NT * ITEMS + (OP >= 2 ? 4 * NT * ITEMS : 0);
}

// ---- dedup by an LDS hash table (8-byte keys): when the caller only needs the distinct set (the
// hash-partitioned first stage: a second stage sorts the survivors anyway) the bucket does not have
// to be sorted.  Records are streamed from HBM straight into an open-addressing table with 64-bit
// ds_cmpst; with 50x coverage ~8 of 9 records find their key already there on the first probe.
// ~30 instructions per record instead of 6 radix passes.  The distinct keys (+ reduced payload)
// are written back in place in table order.
#ifdef BBK_AB_TABLE_WALK  // (A/B: the distinct keys always collected by a walk over the table's slots, as before round 3)
constexpr bool kHashDirectOut = false;
#else
constexpr bool kHashDirectOut = true;
#endif
constexpr int kHashThreads = 512;
#ifndef BBK_HASH_ITEMS
#define BBK_HASH_ITEMS 16
#endif
constexpr int kHashItems = BBK_HASH_ITEMS;          // 512 x 16 = 8192 records per bucket (x 12: 2 % slower, and the
                                                    // fullest bucket of a 10 M-read batch then overflows its slot)
constexpr uint32_t kHashSlots = 8192;               // distinct keys of a bucket: ~n / multiplicity, far below the slots
                                                    // for read data; all-distinct input fills ~0.7 of them
constexpr uint32_t kHashMaxProbes = 256;            // a probe sequence this long means the table is (nearly) full: the
                                                    // bucket holds more distinct keys than slots -> left to the caller

template <int OP>
__global__ __launch_bounds__(kHashThreads) void k_bucket_hash(Key<1> *__restrict__ buf, uint32_t *__restrict__ vals,
                                                             BucketArgs A) {
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *tab = reinterpret_cast<unsigned long long *>(smem);
    uint32_t *pay = reinterpret_cast<uint32_t *>(smem + sizeof(unsigned long long) * kHashSlots);
    uint32_t *scan_tmp = pay + (OP != 0 ? kHashSlots : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > (uint32_t)(kHashThreads * kHashItems)) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    constexpr unsigned long long EMPTY = ~0ull;
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#endif
    uint64_t kk[kHashItems];
    uint32_t vv[kHashItems];
#pragma unroll
    for (int i = 0; i < kHashItems; ++i) {  // all loads first: independent, in flight together -- and while the table
        const uint32_t p = (uint32_t)(i * kHashThreads + tid);  // is cleared below
        kk[i] = EMPTY;
        vv[i] = 0;
        if (p < n) {
            kk[i] = buf[start + p].w[0];
            if (IN_VAL) vv[i] = vals[start + p];
        }
    }
    for (uint32_t s = tid; s < kHashSlots; s += kHashThreads) {
        tab[s] = EMPTY;
        if (OP != 0) pay[s] = 0;
    }
    if (tid == 0) scan_tmp[14] = 0;
    __syncthreads();
    BBK_PH(4, 0, t_prev);  // table init
    uint32_t firsts = 0;  // bit i: record i of this lane was the first of its key in the table
    static_assert(kHashItems <= 32, "one bit per record of a lane");
#pragma unroll
    for (int i = 0; i < kHashItems; ++i) {
        if (kk[i] != EMPTY) {
            // 32-bit mix with multipliers of its own (the partition levels consumed the top bits of part_hash32)
            uint32_t h = ((uint32_t)kk[i] ^ 0x7F4A7C15u) * 0x2C1B3C6Du;
            h ^= h >> 15;
            h += (uint32_t)(kk[i] >> 32) * 0x297A2D39u;
            h ^= h >> 14;
            h *= 0x9E3779B1u;
            uint32_t slot = (h >> 19) & (kHashSlots - 1);
            // (probing all records of a lane in rounds, 12 ds_cmpst in flight, was measured 15 % slower)
            uint32_t probes = 0;
            for (;;) {
                const unsigned long long old = atomicCAS(&tab[slot], EMPTY, (unsigned long long)kk[i]);
                if (old == EMPTY) firsts |= 1u << i;
                if (old == EMPTY || old == kk[i]) break;
                slot = (slot + 1) & (kHashSlots - 1);
                if (kHashItems * kHashThreads > (int)(kHashSlots * 3 / 4) && ++probes > A.max_probes) {
                    scan_tmp[14] = 1;  // give up on this bucket (benign race: everyone writes 1)
                    break;
                }
            }
            if (OP == 1) atomicAdd(&pay[slot], 1u);
            else if (OP == 2) atomicAdd(&pay[slot], vv[i]);
            else if (OP == 3) atomicOr(&pay[slot], vv[i]);
        }
    }
    __syncthreads();
    if (scan_tmp[14]) {  // more distinct keys than the table takes: nothing has been written, the caller takes over
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    BBK_PH(4, 1, t_prev);  // loads + insert
    // compaction of the occupied slots: thread t owns slots t, t + 512, ... (consecutive lanes read
    // consecutive 8-byte slots: no LDS bank conflicts; the output order is free, the set is unsorted)
    constexpr int SPT = kHashSlots / kHashThreads;
    uint32_t cnt = 0;
    if constexpr (OP == 0 && kHashDirectOut) {
        cnt = (uint32_t)__popc(firsts);  // no payload to fetch: whoever put a key into the table writes it out
    } else {
#pragma unroll
        for (int j = 0; j < SPT; ++j) cnt += tab[j * kHashThreads + tid] != EMPTY ? 1u : 0u;
    }
    uint32_t incl = cnt;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    __syncthreads();
    uint32_t wbase, total;
    wave_totals<kHashThreads / 64>(scan_tmp, lane, wave, wbase, total);
    Key<1> *obuf = buf;  // back to the head of the bucket (every record has been read before the barrier above)
    uint32_t *ovals = vals;
    const uint32_t obase = start;
    uint32_t o = obase + wbase + incl - cnt;
    if constexpr (OP == 0 && kHashDirectOut) {
#pragma unroll
        for (int i = 0; i < kHashItems; ++i) {
            if (firsts & (1u << i)) obuf[o++].w[0] = kk[i];
        }
    } else {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const unsigned long long key = tab[j * kHashThreads + tid];
            if (key != EMPTY) {
                obuf[o].w[0] = key;
                if (OP != 0) ovals[o] = pay[j * kHashThreads + tid];
                ++o;
            }
        }
    }
    BBK_PH(4, 2, t_prev);  // compaction + output
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[4][7], 1ull);
#endif
    if (tid == 0) A.dcount[b] = total;
}

// Same idea for wider keys: the bucket's keys are staged in LDS and the table holds record INDICES
// (32-bit ds_cmpst); a probe that finds a different index compares the two keys.  All keys are in
// LDS before the first insertion, so there is no partially written slot to race with.
constexpr int kHashIdxThreads = 512;
// 16-byte keys: 512 x 8 = 4096 records per bucket, 8192 slots; 24/32-byte keys: 512 x 4 = 2048 records, 4096 slots
// (keys + table + payload table must fit the 160 KB of LDS)
template <int W>
struct HashIdxCfg {
    static constexpr int ITEMS = (W <= 2) ? 8 : 4;
    static constexpr uint32_t CAP = kHashIdxThreads * ITEMS;
    static constexpr uint32_t SLOTS = 2 * CAP;
};

template <int W, int OP>
__global__ __launch_bounds__(kHashIdxThreads) void k_bucket_hashidx(Key<W> *__restrict__ buf,
                                                                   uint32_t *__restrict__ vals, BucketArgs A) {
    constexpr int kHashIdxItems = HashIdxCfg<W>::ITEMS;
    constexpr uint32_t kHashIdxCap = HashIdxCfg<W>::CAP, kHashIdxSlots = HashIdxCfg<W>::SLOTS;
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    uint32_t *pay = tab + kHashIdxSlots;
    uint32_t *scan_tmp = pay + (OP != 0 ? kHashIdxSlots : 0);
    Key<W> *skeys = reinterpret_cast<Key<W> *>(scan_tmp + 32);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > kHashIdxCap) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    for (uint32_t s = tid; s < kHashIdxSlots; s += kHashIdxThreads) {
        tab[s] = EMPTY;
        if (OP != 0) pay[s] = 0;
    }
    uint32_t vv[kHashIdxItems];
    {
        // loads first, unconditional (see k_bucket)
        Key<W> rk[kHashIdxItems];
#pragma unroll
        for (int i = 0; i < kHashIdxItems; ++i) {
            const uint32_t p = (uint32_t)(i * kHashIdxThreads + tid);
            const uint32_t at = start + (p < n ? p : n - 1u);
            rk[i] = key_load<W>(&buf[at]);
            vv[i] = IN_VAL ? vals[at] : 0u;
        }
#pragma unroll
        for (int i = 0; i < kHashIdxItems; ++i) {
            const uint32_t p = (uint32_t)(i * kHashIdxThreads + tid);
            if (p < n) key_store<W>(&skeys[p], rk[i]);
            else vv[i] = 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kHashIdxItems; ++i) {
        const uint32_t p = (uint32_t)(i * kHashIdxThreads + tid);
        if (p < n) {
            const Key<W> key = key_load<W>(&skeys[p]);
            // bits of the hash other than the ones the partition consumed (its top ~20)
            uint32_t slot = (part_hash32<W>(key) * 0x9E3779B1u >> 7) & (kHashIdxSlots - 1);
            for (;;) {
                const uint32_t old = atomicCAS(&tab[slot], EMPTY, p);
                if (old == EMPTY) break;
                if (key_eq<W>(key_load<W>(&skeys[old]), key)) break;
                slot = (slot + 1) & (kHashIdxSlots - 1);
            }
            if (OP == 1) atomicAdd(&pay[slot], 1u);
            else if (OP == 2) atomicAdd(&pay[slot], vv[i]);
            else if (OP == 3) atomicOr(&pay[slot], vv[i]);
        }
    }
    __syncthreads();
    constexpr int SPT = kHashIdxSlots / kHashIdxThreads;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) cnt += tab[j * kHashIdxThreads + tid] != EMPTY ? 1u : 0u;  // no bank conflicts
    uint32_t incl = cnt;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    __syncthreads();
    uint32_t wbase, total;
    wave_totals<kHashIdxThreads / 64>(scan_tmp, lane, wave, wbase, total);
    Key<W> *obuf = buf;  // back to the head of the bucket (every record has been read before the barrier above)
    uint32_t *ovals = vals;
    const uint32_t obase = start;
    uint32_t o = obase + wbase + incl - cnt;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        const uint32_t idx = tab[j * kHashIdxThreads + tid];
        if (idx != EMPTY) {
            key_store<W>(&obuf[o], key_load<W>(&skeys[idx]));
            if (OP != 0) ovals[o] = pay[j * kHashIdxThreads + tid];
            ++o;
        }
    }
    if (tid == 0) A.dcount[b] = total;
}

template <int W, int OP>
static size_t bucket_hashidx_smem() {
    return 4 * HashIdxCfg<W>::SLOTS + (OP != 0 ? 4 * HashIdxCfg<W>::SLOTS : 0) + 128 + (size_t)W * 8 * HashIdxCfg<W>::CAP;
}

template <int OP>
static size_t bucket_hash_smem() {
    return sizeof(unsigned long long) * kHashSlots + (OP != 0 ? 4 * kHashSlots : 0) + 64;
}

// one wave per bucket: dense output
template <int W, bool HAS_VAL>
__global__ __launch_bounds__(256) void k_compact(const Key<W> *__restrict__ buf, const uint32_t *__restrict__ vals,
                                                const uint32_t *__restrict__ boff, const uint32_t *__restrict__ dcount,
                                                const uint64_t *__restrict__ doff, uint32_t nbuckets,
                                                Key<W> *__restrict__ out, uint32_t *__restrict__ vout,
                                                uint64_t mask0,  // cleared from word 0 (sort tag), else ~0
                                                uint32_t slot_cap) {  // boff == null: bucket b starts at b*slot_cap
    const uint32_t b = (uint32_t)((BBK_GID()) >> 6);
    if (b >= nbuckets) return;
    const int lane = threadIdx.x & 63;
    uint32_t c = dcount[b];
    if (c == 0xFFFFFFFFu) c = 0;  // left to the caller (reprocessed with the spill list)
    const uint32_t s = boff ? boff[b] : b * slot_cap;
    const uint64_t d = doff[b];
    for (uint32_t i = lane; i < c; i += 64) {
        Key<W> key = key_load<W>(&buf[s + i]);
        key.w[0] &= mask0;
        key_store<W>(&out[d + i], key);
        if (HAS_VAL) vout[d + i] = vals[s + i];
    }
}

// ids of the buckets the first-pass kernel left alone (dcount == 0xFFFFFFFF); *count may run past cap
__global__ void k_flagged(const uint32_t *__restrict__ dcount, uint32_t n, uint32_t *__restrict__ ids, uint32_t cap,
                          uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && dcount[i] == 0xFFFFFFFFu) {
        const uint32_t at = atomicAdd(count, 1u);
        if (at < cap) ids[at] = i;
    }
}

// slot mode, one thread per bucket: its cursor starts at its slot; bucket_seg (narrow path, else null) gets the level-1
// segment the bucket belongs to, the largest s in [0, nseg) with seg_bin[s] <= bucket
__global__ void k_bucket_init(uint32_t *__restrict__ cursor, uint32_t n, uint32_t stride,
                              const uint32_t *__restrict__ seg_bin, uint32_t nseg, uint16_t *__restrict__ bucket_seg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cursor[i] = i * stride;
    if (bucket_seg) {
        uint32_t lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (seg_bin[mid] <= i) lo = mid;
            else hi = mid;
        }
        bucket_seg[i] = (uint16_t)lo;
    }
}

__global__ void k_u32_to_u64(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, uint32_t clampv) {
    const uint64_t i = BBK_GID();
    if (i < n) out[i] = in[i] == 0xFFFFFFFFu ? (uint64_t)clampv : (uint64_t)in[i];
}

// d_total (optional): the total is still on the device
__global__ void k_scan_to_u32(const uint64_t *__restrict__ in, uint64_t n, uint64_t total,
                              const uint64_t *__restrict__ d_total, uint32_t *__restrict__ out) {
    const uint64_t i = BBK_GID();
    if (i < n) out[i] = (uint32_t)in[i];
    if (i == n) out[n] = (uint32_t)(d_total ? *d_total : total);
}

}  // namespace bbk
