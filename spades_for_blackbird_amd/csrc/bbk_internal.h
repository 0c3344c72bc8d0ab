// bbk_internal.h -- the one internal include of the HIP translation units: errors, device buffers, the context with its
// timers, launch helpers and waits, copies, the handle structs, and the scan / sort / unique primitives.  Each section is
// headed by the file that defines what it declares.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/bbk.h"

// ---- errors (context.hip) -------------------------------------------------------------------------------------------
namespace bbk {

void set_error(const char *fmt, ...);
const char *get_error();

struct Error {
    int code;
};

#define BBK_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            ::bbk::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                             __LINE__);                                                        \
            throw ::bbk::Error{BBK_ERR_HIP};                                                   \
        }                                                                                      \
    } while (0)

#define BBK_REQUIRE(cond, code, ...)         \
    do {                                     \
        if (!(cond)) {                       \
            ::bbk::set_error(__VA_ARGS__);   \
            throw ::bbk::Error{code};        \
        }                                    \
    } while (0)

// Runs f(), maps exceptions to a status code: no exception crosses the C ABI.
template <class F>
int guarded(F &&f) {
    try {
        f();
        return BBK_OK;
    } catch (const Error &e) {
        return e.code;
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed");
        return BBK_ERR_NOMEM;
    } catch (const std::exception &e) {
        set_error("internal error: %s", e.what());
        return BBK_ERR_INTERNAL;
    }
}

// ---- device allocator (pool.hip) ------------------------------------------------------------------------------------
void *pool_alloc(size_t bytes, size_t *granted, int *device);  // on the current device
void pool_free(void *p, size_t bytes, int device);
void pool_trim(int device);  // gives the free memory this (device, host thread) holds back to the driver
void pool_report();          // allocator statistics to stderr
size_t pool_mapped_bytes(int device);  // device memory the arenas of all host threads hold mapped on `device`
// *mapped_now: what the calling thread's arenas on `device` hold mapped; *mapped_total, *map_seconds: bytes mapped and
// seconds spent mapping since the process started, by every thread on every device
void pool_stats(int device, uint64_t *mapped_now, uint64_t *mapped_total, double *map_seconds);
bool pool_owns(const void *p);  // the address lies in an arena of the allocator

// Owning device buffer.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int dev = 0;  // device the block lives on (it returns to that device's free list)
    DevBuf() = default;
    explicit DevBuf(size_t n) { alloc(n); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), dev(o.dev) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            bytes = o.bytes;
            dev = o.dev;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // Device memory comes from a caching pool (pool.hip) keyed by (device, host thread): hipMalloc/hipFree of
    // multi-GB buffers cost far more than the kernels that use them, and every step of the path
    // asks for the same sizes again.  All work of a context is issued on one stream, so handing a
    // released block to the next request of the same context is stream-ordered and needs no synchronisation.
    void alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        size_t got = 0;
        p = pool_alloc(n, &got, &dev);
        bytes = got;
    }
    void release() {
        if (p) pool_free(p, bytes, dev);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
};

// ---- context, timers, launches, waits (context.hip) -----------------------------------------------------------------
struct FamilyStat {
    double ms = 0;
    uint64_t launches = 0;
    double bytes = 0;
};

}  // namespace bbk

struct bbk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool profiling = false;
    int num_cus = 256;
    // XCDs the workgroups of a launch are seen to run on (HW_REG_XCC_ID of a probe launch at context creation): the
    // per-XCD fill fronts of the partition kernels assume eight; anything else (a partitioned device) turns them off
    int num_xcds = 8;
    // pending (start, stop, family, bytes) event pairs; resolved lazily
    struct Pending {
        hipEvent_t a, b;
        std::string family;
        double bytes;
    };
    std::vector<Pending> pending;
    std::map<std::string, bbk::FamilyStat> stats;
    void resolve_pending();
    // event counters of the path (read back like a kernel family: launches = events, bytes_total = summed value)
    void add_stat(const char *name, double value) {
        if (!profiling) return;
        bbk::FamilyStat &f = stats[name];
        f.launches += 1;
        f.bytes += value;
    }
    // pinned staging for large device-to-host copies (pageable copies run at a fraction of PCIe)
    void *pinned[2] = {nullptr, nullptr};
    size_t pinned_bytes = 0;
    // pinned staging of a pass's planning arrays (msd.hip: the level-2 layout goes to the device in one copy).  Written
    // only right after a wait on the stream, so the copy queued from it before that wait has finished
    void *plan_pinned = nullptr;
    size_t plan_pinned_bytes = 0;
    // free device memory as the driver last reported it, and the arena figures it was read at: asked again only after the
    // arena has mapped or trimmed
    size_t mem_free = 0;
    uint64_t mem_free_mapped_now = ~0ull, mem_free_mapped_total = ~0ull;
    // super-k-mer stage A (superk.hip): instances / distinct keys of the last batch it finished (0: none yet).  The
    // buckets of the next batch are planned for that multiplicity instead of the worst case 1
    double superk_dup = 0;
};

namespace bbk {

// RAII timer around one kernel launch (or a short run of launches) of a named family.
struct KernelTimer {
    bbk_ctx *ctx;
    hipEvent_t a = nullptr, b = nullptr;
    std::string family;
    double bytes;
    KernelTimer(bbk_ctx *c, const char *fam, double algorithmic_bytes = 0) : ctx(c), family(fam), bytes(algorithmic_bytes) {
        if (ctx->profiling) {
            BBK_HIP(hipEventCreate(&a));
            BBK_HIP(hipEventCreate(&b));
            BBK_HIP(hipEventRecord(a, ctx->stream));
        }
    }
    ~KernelTimer() {
        if (a) {
            (void)hipEventRecord(b, ctx->stream);
            ctx->pending.push_back({a, b, family, bytes});
        }
    }
};

inline void check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("kernel launch %s failed: %s", what, hipGetErrorString(e));
        throw Error{BBK_ERR_HIP};
    }
}

// Every timed kernel launch: LDS limit, timer, launch, check
template <class K, class... Args>
void launch_timed(bbk_ctx *ctx, K fn, const char *name, double bytes, uint32_t grid, uint32_t threads, size_t lds,
                  Args... args) {
    if (lds)
        BBK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    KernelTimer t(ctx, name, bytes);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, ctx->stream, args...);
    check_launch(name);
}

// The one switch on the key width: f(std::integral_constant<int, W>) for W in 1..4, so the body names its templates
// with `decltype(w)::value`.  words_of(k) of a legal k is always one of the four.
template <class F>
void dispatch_w(unsigned W, F &&f) {
    switch (W) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: BBK_REQUIRE(false, BBK_ERR_ARG, "unsupported key width %u", W);
    }
}

// Every wait of the host for the context's stream in the counting path goes through here: "stat_host_waits" counts
// them (the device idles ~20 us around each), so a test can hold the path to its number of decisions
inline void stream_wait(bbk_ctx *ctx) {
    ctx->add_stat("stat_host_waits", 1);
    BBK_HIP(hipStreamSynchronize(ctx->stream));
}

// a device -> host copy on the context's stream that the host waits for (outside the counting path: not a counted wait)
inline void d2h_sync(bbk_ctx *ctx, void *dst, const void *src, size_t bytes) {
    BBK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipStreamSynchronize(ctx->stream));
}

// a numeric BBK_* knob: `unset` when the variable is not set (an empty value reads as 0)
inline uint64_t env_u64(const char *v, uint64_t unset) { return v ? strtoull(v, nullptr, 10) : unset; }

inline unsigned words_of(unsigned k) { return (k + 31) >> 5; }

// One thread per item over billions of items.  A launch whose x dimension holds 2^32 threads or more is neither refused
// nor run in full: the thread count is taken modulo 2^32 and the rest of the items is silently skipped (an index of
// 4 968 413 780 k-mers had its last 4.29 G masks never converted, its start edges never counted:
// profiles/r03/d2d_copy_above_4GiB.log -- the first untouched item is n - 2^32).  Per-item kernels therefore get their
// blocks in two dimensions (grid_blocks) and read their item through BBK_GID(); every one of them checks it against n.
#define BBK_GID() ((((uint64_t)blockIdx.y * gridDim.x) + blockIdx.x) * blockDim.x + threadIdx.x)
inline dim3 grid_blocks(uint64_t blocks) {
    constexpr uint64_t kMaxX = 1ull << 21;  // x 1024 threads at most: 2^31 threads in x
    if (blocks <= kMaxX) return dim3((unsigned)(blocks ? blocks : 1));
    return dim3((unsigned)kMaxX, (unsigned)((blocks + kMaxX - 1) / kMaxX));
}

// One thread per item (or per fixed group of items): n_threads threads in blocks of 256 (grid_blocks), no LDS, the
// context's stream, then the launch check.  Untimed: a caller that wants the launch in a family of its own uses
// launch_items_timed, one that times several launches together opens a KernelTimer around them.
template <class K, class... Args>
void launch_items(bbk_ctx *ctx, const char *name, K fn, uint64_t n_threads, Args... args) {
    hipLaunchKernelGGL(fn, grid_blocks((n_threads + 255) / 256), dim3(256), 0, ctx->stream, args...);
    check_launch(name);
}
template <class K, class... Args>
void launch_items_timed(bbk_ctx *ctx, const char *family, K fn, uint64_t n_threads, Args... args) {
    KernelTimer t(ctx, family);
    launch_items(ctx, family, fn, n_threads, args...);
}

// free device memory (see bbk_ctx::mem_free)
size_t device_free_cached(bbk_ctx *ctx);
// the context's pinned planning block, at least `bytes` long
void *plan_staging(bbk_ctx *ctx, size_t bytes);

// ---- copies (context.hip) -------------------------------------------------------------------------------------------
// Device-to-device / default-kind copies of the library: one place to change how they are done.
hipError_t copy_async(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream);

// std::vector whose resize() does not zero-fill (multi-hundred-MB host buffers that are about to
// be overwritten by a device-to-host copy)
template <class T>
struct default_init_alloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = default_init_alloc<U>;
    };
    template <class U, class... A>
    void construct(U *p, A &&...a) {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U;
        else ::new ((void *)p) U(std::forward<A>(a)...);
    }
};
template <class T>
using raw_vector = std::vector<T, default_init_alloc<T>>;

// Large device -> host copy through the context's pinned staging buffers (chunked, two buffers:
// the copy of chunk i+1 overlaps the host memcpy of chunk i).
void d2h_big(bbk_ctx *ctx, void *dst, const void *src, size_t bytes);
// Device -> file through the same pump (the copy of chunk i+1 overlaps the positional writes of chunk i, several writers
// per chunk).  Returns false on a short write.
bool d2f_big(bbk_ctx *ctx, int fd, uint64_t file_off, const void *src, size_t bytes);

}  // namespace bbk

// ---- handles (bbk_extindex: below, behind its PrefixIndex) ----------------------------------------------------------
struct bbk_reads {
    bbk_ctx *ctx = nullptr;
    uint64_t n = 0;        // reads
    uint64_t n_words = 0;  // packed words
    uint64_t bases = 0;    // total bases (sum of len)
    const uint64_t *d_words = nullptr;
    const uint64_t *d_woff = nullptr;  // n+1
    const uint32_t *d_len = nullptr;   // n
    bbk::DevBuf own_words, own_woff, own_len;
};

struct bbk_kmerset {
    unsigned k = 0, W = 0;
    unsigned flags = 0;
    uint64_t n = 0;          // distinct records
    uint64_t instances = 0;  // k-mer instances that entered the sort
    bbk::DevBuf keys;        // n * W u64, ascending
    bbk::DevBuf counts;      // n u32 (optional)
    bool has_counts = false;
    bool sorted = true;      // false: distinct but in hash-bucket order (BBK_UNSORTED)
    bool ref_order = false;  // true: final_kmers order (16 XXH3 buckets, ascending inside) instead of ascending
};

namespace bbk {

// ---- scan (scan.hip) ------------------------------------------------------------------------------------------------
// Exclusive scan of n u64 values (in place allowed); returns the total.
uint64_t exclusive_scan_u64(bbk_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n);
// Two arrays of n values in the same launches and ONE wait; out0[n] and out1[n] receive the totals as well (the
// outputs hold n + 1 entries).
void exclusive_scan2_u64(bbk_ctx *ctx, const uint64_t *in0, uint64_t *out0, const uint64_t *in1, uint64_t *out1,
                         uint64_t n, uint64_t totals[2]);
// What the first level of a scan reads: u64 values, u32 values (SCAN_U32_FLAGGED: 0xFFFFFFFF counts 0), the fill of
// slot i from its cursor, min(p[i] - i * stride, cap) (SCAN_SLOT_FILL), or the units of read i computed from its length
// p[i] (SCAN_READ_UNITS: ceil(max(0, len - k + 1) / C) with k = stride and C = cap -- C = 1: k-mers, C = CH: chunks,
// C = the segment length: super-k-mer segments).  A SCAN_READ_UNITS source with `woff` also checks the order of the
// packed words in its reduce pass (in the one-workgroup scan when n fits a single tile and there is none): *unordered
// is set when woff[i + 1] < woff[i] + ceil(len[i] / 32) for some read
enum { SCAN_U64 = 0, SCAN_U32_FLAGGED = 1, SCAN_SLOT_FILL = 2, SCAN_READ_UNITS = 3 };
struct ScanSrc {
    const void *p;
    uint32_t kind, stride, cap;
    const uint64_t *woff = nullptr;
    uint32_t *unordered = nullptr;
};
// The scan without its wait: narr (1 or 2) arrays are scanned into out[a] (u64), the totals are left in d_total[a] on
// the device (tail: also in out[a][n]).  out[a] == nullptr makes array a TOTAL-ONLY: its reduce pass still sums it, its
// apply pass neither loads nor stores below the top level.  The scratch buffers go into `keep`, which must live until
// the caller has waited for the stream.
void exclusive_scan_enqueue(bbk_ctx *ctx, int narr, const ScanSrc *src, uint64_t *const *out, uint64_t n,
                            uint64_t *d_total, bool tail, std::vector<DevBuf> &keep);

// What a pass over a read set needs before its first tile: the k-mers of the reads, their units of C k-mer positions
// (chunks of the level-1 kernels, super-k-mer segments; C = 1: the k-mers themselves) and the exclusive scan of the
// units per read.  One fused scan straight from the read lengths (SCAN_READ_UNITS: no per-read array is materialised,
// the k-mers are a total-only array of the same launches) and ONE wait for both totals; coff[n] is written on the
// device.  The tile descriptors of a caller are one launch of its tile kernel over coff once `units` has given the
// tile count (kmer_ops.h: read_of_unit).
struct ReadPlan {
    DevBuf coff;                    // n + 1 entries: units before read i; coff[n] = units
    uint64_t kmers = 0, units = 0;  // totals over the reads
    // d_unordered: a zeroed device word, set when the packed words of the reads are not in read order (null: not asked)
    void run(bbk_ctx *ctx, const bbk_reads *rd, unsigned k, unsigned C, uint32_t *d_unordered);
};

// ---- sort (sort.hip) ------------------------------------------------------------------------------------------------
// One LSD pass selector: kind 0 = bits [shift, shift+bits) of key word `word`;
// kind 1 = XXH3 bucket (kmer_buckets.hpp:28-33) with nb <= 256 buckets;
// kind 2 = owner(mix(key), nb) for the multi-GPU partition.
struct PassDesc {
    int kind;
    int word;
    int shift;
    int bits;
    unsigned nb;
};

// Key-bit passes that sort records of W words into the reference order (word 0 most
// significant, adt/array_vector.hpp:114-123) given that only the low 2k bits are populated.
std::vector<PassDesc> key_passes(unsigned k);

// Stable LSD radix sort of n records (W u64 words each, optional u32 payload). keys/vals are
// sorted in place; tmp buffers must hold n records.  n < 2^32.
void sort_records(bbk_ctx *ctx, int W, void *keys, void *keys_tmp, uint32_t *vals, uint32_t *vals_tmp, uint64_t n,
                  const std::vector<PassDesc> &passes);
// one stable counting pass src -> dst (device buffers, not aliased) on the digit `pd`; h_digit_totals (256 entries,
// optional) receives the number of records of every digit value
void partition_records(bbk_ctx *ctx, int W, const void *src, void *dst, const uint32_t *vsrc, uint32_t *vdst, uint64_t n,
                       const PassDesc &pd, uint64_t *h_digit_totals = nullptr);

// ---- unique (unique.hip) --------------------------------------------------------------------------------------------
enum ReduceOp { REDUCE_COUNT = 0, REDUCE_SUM = 1, REDUCE_OR = 2 };
// Unique of a sorted record array: distinct keys to out_keys (may alias nothing), per-key reduction of
// vals (COUNT: run length, SUM: sum of vals, OR: or of vals) to out_vals (may be null for COUNT-less).
// Returns the number of distinct keys.
uint64_t unique_records(bbk_ctx *ctx, int W, const void *keys, const uint32_t *vals, uint64_t n, void *out_keys,
                        uint32_t *out_vals, ReduceOp op);
// The (key, val) pairs with val != 0, in their order, into out_* (allocated only when something is dropped); returns how
// many were kept.
uint64_t drop_zero_vals(bbk_ctx *ctx, int W, const void *keys, const uint32_t *vals, uint64_t n, DevBuf &out_keys,
                        DevBuf &out_vals);

// ---- prefix table (extindex.hip) ------------------------------------------------------------------------------------
// The prefix table over an ascending key array of n records (W words, k-mer size k) that table_find
// (kmer_ops.h) reads: (1 << bits) + 1 entries, u32 (u64 when `wide`: 2^32 - 2 records or more).  It remembers the W and
// k it was built for, so table() is the only place that derives the shift a lookup applies to word 0.
struct PrefixTable;
struct PrefixIndex {
    DevBuf buf;
    unsigned bits = 0;
    bool wide = false;
    unsigned W = 0, k = 0;
    void build(bbk_ctx *ctx, const uint64_t *keys, unsigned W, unsigned k, uint64_t n);  // waits for the stream
    PrefixTable table() const;
};

}  // namespace bbk

// (the one handle down here: it holds a PrefixIndex by value)
struct bbk_extindex {
    unsigned k = 0, W = 0;
    uint64_t n = 0;
    uint64_t instances = 0;
    bbk::DevBuf keys;   // n * W u64 ascending (canonical k-mers)
    bbk::DevBuf masks;  // n u8
    bbk::PrefixIndex prefix;  // lookup accelerator over keys
};

// ---- exported for the tests only (not declared in bbk.h) ------------------------------------------------------------
// scan.hip: exclusive_scan2_u64 in place over two device arrays of n + 1 u64 each (entries 0..n-1 are the input, entry n
// receives the total); totals[2] on the host receives the two sums.
extern "C" int bbk_scan2_u64(bbk_ctx *ctx, void *d_a, void *d_b, uint64_t n, uint64_t *totals);
// context.hip: `bytes` of device memory through d2h_big into h_dst (when not NULL) and through d2f_big to offset 0 of fd
// (when fd >= 0)
extern "C" int bbk_staged_copy(bbk_ctx *ctx, const void *d_src, uint64_t bytes, void *h_dst, int fd);
// unique.hip: the ordered selection of select.h with per_item(vals[i] >= min) over n u32 values: the index (u64) and the
// value of every kept item at its rank, *kept their number; waits for the stream
extern "C" int bbk_select_u32(bbk_ctx *ctx, const void *d_vals, uint64_t n, uint32_t min, void *d_idx_out, void *d_val_out,
                              uint64_t *kept);
// msd.hip: the tile geometry of the counting paths at k, and the plan of a read set with the descriptors of its tiles,
// copied to the host
extern "C" int bbk_read_plan_geometry(unsigned k, uint32_t *out);
extern "C" int bbk_read_plan(bbk_ctx *ctx, const bbk_reads *rd, unsigned k, unsigned C, unsigned tile, int superk,
                             uint64_t *coff, uint64_t *totals, uint32_t *unordered, void *tiles, uint64_t tile_cap,
                             uint64_t *n_tiles);
