// pool.hip -- the device allocator behind every DevBuf: arenas of mapped virtual memory per (device, host thread), with
// the size-matching block cache as the fallback.  Host code only.  It stands where the reference leans on malloc: its
// buckets and merge buffers come and go per call (common/utils/kmer_mph/kmer_splitter.hpp), which the device cannot afford.
#include <hip/hip_runtime.h>

#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "arena.h"
#include "bbk_internal.h"

namespace bbk {

// ---- device allocator --------------------------------------------------------------------------
// hipMalloc of fresh memory costs ~30 ms/GiB on this platform (page tables, not bandwidth): a configs[2]-size call
// allocates hundreds of GB of working buffers whose sizes never repeat exactly, and a block cache that matches sizes
// either misses or fills the device and has to be trimmed -- allocation was 70 % of the wall time there.  The allocator
// is therefore an ARENA per (device, host thread): one reserved virtual range (hipMemAddressReserve), physical memory
// mapped into it in 1 GiB chunks as the high-water mark grows (hipMemCreate + hipMemMap), and a best-fit free list
// with coalescing inside the range.  Physical memory is paid for once; every later request of any size is carved out
// of what is already mapped.  (Fallback when the virtual-memory API is unavailable: the size-matching block cache.)
//
// bbk_ctx_trim / context destruction unmap and release the chunks at the end of the arena that are entirely free.
// A virtual address that was unmapped is never mapped again (arena.h: ArenaIndex::top only grows): on this platform a
// range that is unmapped and then given NEW physical memory is not coherent afterwards -- a kernel that fills and
// re-reads it finds words of the wrong chunk, a small host->device copy does not arrive where the next kernel reads
// (tools/probes/vmm_remap_copy_probe.hip, profiles/r03/vmm_remap_probe.log; the round-2 "abort after trim").  New
// chunks at fresh addresses are clean.  When the reserved range is used up the arena gets a new GENERATION (another
// reservation); an old generation only takes its blocks back and disappears when the last one has returned.
//
// Keys are (device, host thread).  The ABI's contract is one context per GPU per host thread, all of a context's work
// is issued on its one stream, and every entry point returns with that stream idle or with the released blocks' last
// use already queued on it -- so inside one key, handing released memory to the next request is stream-ordered.
// Memory never crosses devices nor threads.  bbk_ctx_set_stream drains the old stream first.
namespace {
struct PoolKey {
    int device;
    std::thread::id thread;
    bool operator<(const PoolKey &o) const { return device != o.device ? device < o.device : thread < o.thread; }
};
constexpr size_t kPoolGranule = 2ull << 20;   // request sizes are rounded to 2 MiB
constexpr size_t kArenaChunk = 1ull << 30;    // physical memory is mapped in 1 GiB chunks

struct Arena : ArenaIndex {  // bookkeeping in arena.h (host-only, fuzzed by tests/test_arena.py)
    char *base = nullptr;
    size_t va_bytes = 0;  // size of the reservation
    std::vector<hipMemGenericAllocationHandle_t> chunks;  // parallel to chunk_off
    bool contains(const void *p) const { return base && (const char *)p >= base && (const char *)p < base + va_bytes; }
};
struct ArenaGens {
    std::vector<std::unique_ptr<Arena>> gens;  // the last one serves requests
};

struct Pool {
    std::mutex mu;
    int vmm = -1;  // -1 undecided, 0 block cache, 1 arenas
    std::map<PoolKey, ArenaGens> arenas;
    std::map<PoolKey, std::multimap<size_t, void *>> free_blocks;  // block-cache fallback: key -> size -> block
    // statistics (BBK_VERBOSE prints them when a context is destroyed)
    double malloc_s = 0, free_s = 0;
    uint64_t mallocs = 0, frees = 0, hits = 0, generations = 0;
    double malloc_bytes = 0;
};
inline double wall_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
Pool &pool() {
    static Pool p;
    return p;
}
int current_device() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}

// reservation of a new generation: as large as the platform grants (BBK_ARENA_VA_GB: tests make it small)
std::unique_ptr<Arena> arena_reserve() {
    auto A = std::make_unique<Arena>();
    const char *e = getenv("BBK_ARENA_VA_GB");
    // 4 TiB: hundreds of trim cycles of a 288 GB device before a new generation is needed, and eight rank threads of one
    // process (spades-kmercount --devices) together stay far below the 128 TiB of user address space
    const size_t first = e ? (size_t)strtoull(e, nullptr, 10) << 30 : (4ull << 40);
    for (size_t sz = first; sz >= (e ? first : (1ull << 38)); sz >>= 1) {
        void *p = nullptr;
        if (hipMemAddressReserve(&p, sz, 0, nullptr, 0) == hipSuccess && p) {
            A->base = (char *)p;
            A->va_bytes = sz;
            ++pool().generations;
            return A;
        }
        (void)hipGetLastError();
        if (e) break;
    }
    return nullptr;
}

// unmaps and releases the chunks at the END of the backed range that are completely free (all of them when nothing
// is allocated); caller holds the lock and has made sure the device is idle.  Their addresses are retired.
void arena_shrink(Arena &A) {
    const double t0 = wall_s();
    size_t at = 0;
    bool unmapped = false;
    while (!A.chunks.empty() && A.shrink_one(kArenaChunk, &at)) {
        const hipError_t eu = hipMemUnmap(A.base + at, kArenaChunk);
        if (eu != hipSuccess) {  // still mapped, but no longer in the index: the chunk is lost to this arena, not reused
            fprintf(stderr, "[bbk] arena: hipMemUnmap(+%zu GiB) failed: %s\n", at >> 30, hipGetErrorString(eu));
            (void)hipGetLastError();
        } else {
            const hipError_t er = hipMemRelease(A.chunks.back());
            if (er != hipSuccess) {
                fprintf(stderr, "[bbk] arena: hipMemRelease failed: %s\n", hipGetErrorString(er));
                (void)hipGetLastError();
            }
        }
        A.chunks.pop_back();
        ++pool().frees;
        unmapped = true;
    }
    if (unmapped) {
        // an ordinary allocation freed after the unmaps makes the driver invalidate the device's address translations
        // (probe modes flush_before / flush_after: a re-mapped range is coherent again after this).  The arena does not
        // depend on it -- it never maps at a retired address -- but whoever gets the freed memory next should not meet
        // stale translations of ours either.
        void *o = nullptr;
        if (hipMalloc(&o, 64ull << 20) == hipSuccess) {
            (void)hipMemset(o, 0, 64ull << 20);
            (void)hipDeviceSynchronize();
            (void)hipFree(o);
        }
        (void)hipGetLastError();
    }
    pool().free_s += wall_s() - t0;
}

// maps `n` more chunks at the top of the arena; false on out-of-memory or when the reservation is used up (nothing is
// left half-mapped: the chunks that were mapped stay and are usable)
bool arena_grow(Arena &A, int dev, size_t n) {
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    const double t0 = wall_s();
    size_t done = 0;
    for (; done < n; ++done) {
        if (A.top + kArenaChunk > A.va_bytes) break;
        hipMemGenericAllocationHandle_t h;
        if (hipMemCreate(&h, kArenaChunk, &prop, 0) != hipSuccess) break;
        if (hipMemMap(A.base + A.top, kArenaChunk, 0, h, 0) != hipSuccess ||
            hipMemSetAccess(A.base + A.top, kArenaChunk, &acc, 1) != hipSuccess) {
            (void)hipMemRelease(h);
            break;
        }
        A.chunks.push_back(h);
        A.grown(kArenaChunk);
    }
    (void)hipGetLastError();
    pool().malloc_s += wall_s() - t0;
    pool().mallocs += done;
    pool().malloc_bytes += (double)done * kArenaChunk;
    return done == n;
}

// gives every cached block of `device` (all threads) back to the driver (block-cache fallback)
void trim_device_blocks(int device) {
    for (auto &kv : pool().free_blocks) {
        if (kv.first.device != device) continue;
        const double t0 = wall_s();
        for (auto &b : kv.second) (void)hipFree(b.second);
        pool().free_s += wall_s() - t0;
        pool().frees += kv.second.size();
        kv.second.clear();
    }
}

// trims every generation of a key; generations other than the serving one go away once nothing is backed in them
// (their reservation stays reserved: a freed range could be handed out again by the driver -- the reuse to avoid)
void gens_shrink(ArenaGens &G) {
    for (size_t i = 0; i < G.gens.size();) {
        arena_shrink(*G.gens[i]);
        if (i + 1 < G.gens.size() && G.gens[i]->mapped == 0) G.gens.erase(G.gens.begin() + (long)i);
        else ++i;
    }
}
}  // namespace

void pool_report() {
    std::lock_guard<std::mutex> g(pool().mu);
    size_t mapped = 0, retired = 0;
    for (auto &kv : pool().arenas)
        for (auto &A : kv.second.gens) {
            mapped += A->mapped;
            retired += A->top - A->mapped;
        }
    fprintf(stderr, "[bbk] allocator (%s): %llu %s (%.1f GB, %.3f s), %llu requests served from mapped memory, %llu releases "
                    "(%.3f s), %.1f GB mapped now, %.1f GB of addresses retired, %llu reservation(s)\n",
            pool().vmm == 1 ? "arena" : "block cache", (unsigned long long)pool().mallocs,
            pool().vmm == 1 ? "chunks mapped" : "hipMalloc", pool().malloc_bytes / 1e9, pool().malloc_s,
            (unsigned long long)pool().hits, (unsigned long long)pool().frees, pool().free_s, (double)mapped / 1e9,
            (double)retired / 1e9, (unsigned long long)pool().generations);
}

bool pool_owns(const void *p) {
    std::lock_guard<std::mutex> g(pool().mu);
    for (auto &kv : pool().arenas)
        for (auto &A : kv.second.gens)
            if (A->contains(p)) return true;
    return false;
}

void pool_stats(int device, uint64_t *mapped_now, uint64_t *mapped_total, double *map_seconds) {
    std::lock_guard<std::mutex> g(pool().mu);
    const PoolKey key{device, std::this_thread::get_id()};
    uint64_t now = 0;
    auto it = pool().arenas.find(key);
    if (it != pool().arenas.end())
        for (auto &A : it->second.gens) now += A->mapped;
    if (mapped_now) *mapped_now = now;
    if (mapped_total) *mapped_total = (uint64_t)pool().malloc_bytes;
    if (map_seconds) *map_seconds = pool().malloc_s;
}

size_t pool_mapped_bytes(int device) {
    std::lock_guard<std::mutex> g(pool().mu);
    size_t mapped = 0;
    for (auto &kv : pool().arenas)
        if (kv.first.device == device)
            for (auto &A : kv.second.gens) mapped += A->mapped;
    return mapped;
}

static void *pool_alloc_impl(size_t bytes, size_t *granted, int *device);

// BBK_POOL_POISON=1 (tests): every block handed out is filled with 0xCD first, so that code which reads device memory
// it never wrote -- and got away with it on the driver's zero-filled fresh allocations -- fails deterministically
void *pool_alloc(size_t bytes, size_t *granted, int *device) {
    void *p = pool_alloc_impl(bytes, granted, device);
    static const bool poison = getenv("BBK_POOL_POISON") != nullptr;
    if (poison) {
        (void)hipDeviceSynchronize();
        (void)hipMemset(p, 0xCD, *granted);
        (void)hipDeviceSynchronize();
    }
    return p;
}

static void *pool_alloc_impl(size_t bytes, size_t *granted, int *device) {
    const size_t want = bytes <= kPoolGranule ? kPoolGranule : ((bytes + kPoolGranule - 1) / kPoolGranule) * kPoolGranule;
    const int dev = current_device();
    *device = dev;
    const PoolKey key{dev, std::this_thread::get_id()};
    std::unique_lock<std::mutex> g(pool().mu);
    if (pool().vmm == -1) pool().vmm = getenv("BBK_NO_VMM") ? 0 : 1;
    if (pool().vmm == 1) {
        ArenaGens &G = pool().arenas[key];
        if (G.gens.empty()) {
            auto A = arena_reserve();
            if (!A) {
                bool others = false;
                for (auto &kv : pool().arenas) others = others || !kv.second.gens.empty();
                pool().arenas.erase(key);
                if (others) {
                    set_error("hipMemAddressReserve failed");
                    throw Error{BBK_ERR_HIP};
                }
                pool().vmm = 0;  // no virtual-memory API on this platform: block cache
            } else {
                G.gens.push_back(std::move(A));
            }
        }
    }
    if (pool().vmm == 1) {
        ArenaGens &G = pool().arenas[key];
        for (int attempt = 0;; ++attempt) {
            Arena &A = *G.gens.back();
            size_t off = 0;
            if (A.take(want, &off)) {
                ++pool().hits;
                *granted = want;
                return A.base + off;
            }
            // grow: the request may start in the free tail of the backed range
            const size_t tail = A.free_tail();
            const size_t need = (want - tail + kArenaChunk - 1) / kArenaChunk;
            if (A.top + need * kArenaChunk > A.va_bytes) {
                // the reservation is used up (retired addresses are not reused): a new generation serves from here on
                BBK_REQUIRE(attempt == 0 && want + kArenaChunk <= A.va_bytes, BBK_ERR_NOMEM,
                            "request of %zu bytes does not fit a reservation of %zu", want, A.va_bytes);
                auto N = arena_reserve();
                BBK_REQUIRE(N != nullptr, BBK_ERR_HIP, "hipMemAddressReserve failed for a new arena generation");
                G.gens.push_back(std::move(N));
                continue;
            }
            if (!arena_grow(A, dev, need)) {
                // out of device memory: give back what the arenas of this device hold unused -- other threads' and our
                // own free chunks (their owners' streams may still have the last use of that memory queued: wait for
                // the device first)
                (void)hipDeviceSynchronize();
                for (auto &kv : pool().arenas)
                    if (kv.first.device == dev) gens_shrink(kv.second);
                Arena &B = *G.gens.back();
                const size_t tail2 = B.free_tail();
                const size_t need2 = want > tail2 ? (want - tail2 + kArenaChunk - 1) / kArenaChunk : 0;
                if (B.top + need2 * kArenaChunk > B.va_bytes || !arena_grow(B, dev, need2)) {
                    set_error("device memory exhausted: %zu bytes requested, %.1f GB mapped, %.1f GB of it free but fragmented",
                              want, (double)B.mapped / 1e9, (double)B.free_bytes() / 1e9);
                    throw Error{BBK_ERR_NOMEM};
                }
            }
            if (!G.gens.back()->take(want, &off)) {
                set_error("arena: internal error after growing");
                throw Error{BBK_ERR_INTERNAL};
            }
            *granted = want;
            return G.gens.back()->base + off;
        }
    }
    // ---- block-cache fallback
    {
        auto &fl = pool().free_blocks[key];
        auto it = fl.lower_bound(want);
        if (it != fl.end() && it->first <= want + want / 8) {  // accept a cached block up to 12.5 % larger than asked
            void *p = it->second;
            *granted = it->first;
            fl.erase(it);
            ++pool().hits;
            return p;
        }
    }
    void *p = nullptr;
    const double t0 = wall_s();
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        trim_device_blocks(dev);  // give cached blocks back and retry once
        e = hipMalloc(&p, want);
    }
    pool().malloc_s += wall_s() - t0;
    ++pool().mallocs;
    pool().malloc_bytes += (double)want;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
        throw Error{e == hipErrorOutOfMemory ? BBK_ERR_NOMEM : BBK_ERR_HIP};
    }
    *granted = want;
    return p;
}

void pool_free(void *p, size_t bytes, int device) {
    std::lock_guard<std::mutex> g(pool().mu);
    const PoolKey key{device, std::this_thread::get_id()};
    if (pool().vmm == 1) {
        // the block returns to the arena it came from: a generation of this (device, thread), or -- a handle released
        // by another thread -- whichever arena of the device contains the address
        for (auto &kv : pool().arenas) {
            if (kv.first.device != device) continue;
            for (auto &A : kv.second.gens)
                if (A->contains(p)) {
                    A->add_free((size_t)((char *)p - A->base), bytes);
                    return;
                }
        }
        return;  // not ours (cannot happen)
    }
    pool().free_blocks[key].emplace(bytes, p);
}

// gives the unused memory of this (device, calling thread) back to the driver: what a context being destroyed (or
// bbk_ctx_trim) leaves behind.  The caller has drained the context's stream; the device is synchronised here because
// unmapping under a running kernel of another stream would fault it.
void pool_trim(int device) {
    std::lock_guard<std::mutex> g(pool().mu);
    const PoolKey key{device, std::this_thread::get_id()};
    if (pool().vmm == 1) {
        auto it = pool().arenas.find(key);
        if (it == pool().arenas.end() || getenv("BBK_ARENA_KEEP")) return;  // BBK_ARENA_KEEP=1: A/B switch, never unmap
        (void)hipDeviceSynchronize();
        gens_shrink(it->second);
        return;
    }
    auto it = pool().free_blocks.find(key);
    if (it == pool().free_blocks.end()) return;
    const double t0 = wall_s();
    for (auto &b : it->second) (void)hipFree(b.second);
    pool().free_s += wall_s() - t0;
    pool().frees += it->second.size();
    pool().free_blocks.erase(it);
}

}  // namespace bbk
