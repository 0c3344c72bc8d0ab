// context.hip -- what every call into the library starts from: the error string behind bbk_last_error, the bbk_ctx_*
// C ABI (stream, timers, memory figures, the XCD probe) and the copies of the library, among them the staged
// device -> host / device -> file pump through the context's pinned buffers.  Nothing of the reference stands behind
// it: there the data never leaves host memory.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdarg>
#include <cstring>

#include "bbk_internal.h"

namespace bbk {

static thread_local char g_err[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }

hipError_t copy_async(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    if (bytes == 0) return hipSuccess;
    return hipMemcpyAsync(dst, src, bytes, kind, stream);
}

// Device -> host through the context's two pinned buffers, 32 MiB at a time: consume(chunk, offset, bytes) gets the
// chunks in order, on the host, while the copy of the next one runs.  false from consume, or a copy that failed, ends it
// and is returned; a copy may then still be queued on the stream.
template <class Consume>
static bool staged_d2h(bbk_ctx *ctx, const void *src, size_t bytes, Consume consume) {
    constexpr size_t kChunk = 32ull << 20;
    if (!ctx->pinned[0]) {
        BBK_HIP(hipHostMalloc(&ctx->pinned[0], kChunk, hipHostMallocDefault));
        BBK_HIP(hipHostMalloc(&ctx->pinned[1], kChunk, hipHostMallocDefault));
        ctx->pinned_bytes = kChunk;
    }
    struct Events {  // destroyed on every way out
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    BBK_HIP(hipEventCreateWithFlags(&ev.e[0], hipEventDisableTiming));
    BBK_HIP(hipEventCreateWithFlags(&ev.e[1], hipEventDisableTiming));
    const size_t nchunks = (bytes + kChunk - 1) / kChunk;
    auto issue = [&](size_t c) {
        const size_t off = c * kChunk, sz = std::min(kChunk, bytes - off);
        (void)hipMemcpyAsync(ctx->pinned[c & 1], (const char *)src + off, sz, hipMemcpyDeviceToHost, ctx->stream);
        (void)hipEventRecord(ev.e[c & 1], ctx->stream);
    };
    issue(0);
    for (size_t c = 0; c < nchunks; ++c) {
        // chunk c + 1 goes to the other buffer before the wait for chunk c: that buffer held chunk c - 1, and consume()
        // returned from it in the last iteration (its readers, parallel or not, have ended by then)
        if (c + 1 < nchunks) issue(c + 1);
        const size_t off = c * kChunk, sz = std::min(kChunk, bytes - off);
        if (hipEventSynchronize(ev.e[c & 1]) != hipSuccess || !consume(ctx->pinned[c & 1], off, sz)) return false;
    }
    return true;
}

void d2h_big(bbk_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes < (4ull << 20)) {
        BBK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        stream_wait(ctx);
        return;
    }
    const bool ok = staged_d2h(ctx, src, bytes, [&](const void *chunk, size_t off, size_t sz) {
        memcpy((char *)dst + off, chunk, sz);
        return true;
    });
    BBK_REQUIRE(ok, BBK_ERR_HIP, "d2h_big: the staged copy of %zu bytes failed", bytes);
}

bool d2f_big(bbk_ctx *ctx, int fd, uint64_t file_off, const void *src, size_t bytes) {
    static const int kWriters = [] {
        const char *e = getenv("BBK_WRITE_THREADS");
        const int t = e ? atoi(e) : 4;  // measured on tmpfs: 2 -> 3.8, 4 -> 6.4, 8 -> 3.5, 16 -> 4.6 GB/s (one box; the writers share 16 cores)
        return t < 1 ? 1 : (t > 64 ? 64 : t);
    }();
    if (bytes == 0) return true;
    // reserve the file's pages in one call first: concurrent writers that each allocate page-cache pages contend (tmpfs:
    // 3-6 GB/s, noisy; pre-allocated: 6.1-6.6 GB/s whatever the writer count).  The raw syscall, not posix_fallocate: a
    // file system without support just says so (the glibc emulation would write zeros).  What remains is the kernel's
    // own page allocation for ONE tmpfs file (~7.5 GB/s, serialised on the inode): writing through a mapping of the
    // file, or letting the device copy straight into the registered mapping (no CPU copy at all), measured the same.
    if (!getenv("BBK_NO_FALLOCATE")) (void)fallocate(fd, 0, (off_t)file_off, (off_t)bytes);
    const bool ok = staged_d2h(ctx, src, bytes, [&](const void *chunk, size_t off, size_t sz) {
        // several writers per chunk: a single pwrite stream into tmpfs runs at ~1/3 of what the box can do
        const int T = kWriters;
        const size_t part = (((sz + T - 1) / T) + 4095) & ~(size_t)4095;  // page-aligned shares
        bool written = true;
#pragma omp parallel for num_threads(T) schedule(static)
        for (int t = 0; t < T; ++t) {
            size_t o = std::min(sz, (size_t)t * part);
            const size_t e = std::min(sz, o + part);
            while (o < e) {
                const ssize_t w = pwrite(fd, (const char *)chunk + o, e - o, (off_t)(file_off + off + o));
                if (w <= 0) {
#pragma omp atomic write
                    written = false;
                    break;
                }
                o += (size_t)w;
            }
        }
        return written;
    });
    (void)hipStreamSynchronize(ctx->stream);
    return ok;
}

size_t device_free_cached(bbk_ctx *ctx) {
    uint64_t now = 0, total = 0;
    pool_stats(ctx->device, &now, &total, nullptr);
    if (now != ctx->mem_free_mapped_now || total != ctx->mem_free_mapped_total) {
        size_t fr = 0, tot = 0;
        BBK_HIP(hipMemGetInfo(&fr, &tot));
        ctx->mem_free = fr;
        ctx->mem_free_mapped_now = now;
        ctx->mem_free_mapped_total = total;
    }
    return ctx->mem_free;
}

void *plan_staging(bbk_ctx *ctx, size_t bytes) {
    if (bytes > ctx->plan_pinned_bytes) {
        // (the block is replaced only here, by the caller's rule after a wait: no copy is reading the old one)
        if (ctx->plan_pinned) BBK_HIP(hipHostFree(ctx->plan_pinned));
        ctx->plan_pinned = nullptr;
        ctx->plan_pinned_bytes = 0;
        const size_t want = std::max<size_t>(2 * bytes, 256u << 10);
        BBK_HIP(hipHostMalloc(&ctx->plan_pinned, want, hipHostMallocDefault));
        ctx->plan_pinned_bytes = want;
    }
    return ctx->plan_pinned;
}

}  // namespace bbk

// ---- context (C ABI) -------------------------------------------------------------------------
void bbk_ctx::resolve_pending() {
    for (auto &p : pending) {
        (void)hipEventSynchronize(p.b);
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            auto &s = stats[p.family];
            s.ms += ms;
            s.launches += 1;
            s.bytes += p.bytes;
        }
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    pending.clear();
}

extern "C" {

const char *bbk_last_error(void) { return bbk::get_error(); }
const char *bbk_version(void) { return "bbk 0.1 (gfx950)"; }

// which XCDs the workgroups of a launch land on (one bit per HW_REG_XCC_ID value seen)
__global__ void k_xcd_probe(uint32_t *mask) {
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (threadIdx.x == 0) atomicOr(mask, 1u << (xcc & 15u));
}

int bbk_ctx_create(int device, bbk_ctx **out) {
    return bbk::guarded([&] {
        BBK_REQUIRE(out != nullptr, BBK_ERR_ARG, "bbk_ctx_create: out is NULL");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        BBK_REQUIRE(e == hipSuccess && ndev > 0, BBK_ERR_HIP,
                    "bbk_ctx_create: no HIP device available (%s); this engine has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        BBK_REQUIRE(device >= 0 && device < ndev, BBK_ERR_ARG, "bbk_ctx_create: device %d out of range [0,%d)", device,
                    ndev);
        BBK_HIP(hipSetDevice(device));
        bbk_ctx *c = new bbk_ctx();
        c->device = device;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
        BBK_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
        {
            uint32_t *d_mask = nullptr, h_mask = 0;
            if (hipMalloc(&d_mask, 4) == hipSuccess) {
                (void)hipMemsetAsync(d_mask, 0, 4, c->stream);
                hipLaunchKernelGGL(k_xcd_probe, dim3(4096), dim3(64), 0, c->stream, d_mask);
                if (hipMemcpyAsync(&h_mask, d_mask, 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                    hipStreamSynchronize(c->stream) == hipSuccess && h_mask)
                    c->num_xcds = __builtin_popcount(h_mask);
                (void)hipFree(d_mask);
            }
            (void)hipGetLastError();
        }
        *out = c;
    });
}

int bbk_ctx_destroy(bbk_ctx *ctx) {
    if (!ctx) return BBK_OK;
    (void)hipSetDevice(ctx->device);
    ctx->resolve_pending();
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    bbk::pool_trim(ctx->device);
    if (getenv("BBK_VERBOSE")) bbk::pool_report();
    if (ctx->pinned[0]) (void)hipHostFree(ctx->pinned[0]);
    if (ctx->pinned[1]) (void)hipHostFree(ctx->pinned[1]);
    if (ctx->plan_pinned) (void)hipHostFree(ctx->plan_pinned);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return BBK_OK;
}

int bbk_ctx_set_stream(bbk_ctx *ctx, void *hip_stream) {
    return bbk::guarded([&] {
        BBK_REQUIRE(ctx != nullptr, BBK_ERR_ARG, "bbk_ctx_set_stream: ctx is NULL");
        // drain the old stream: blocks this context has released (their last use queued on it) may be handed out
        // again for work on the new one
        BBK_HIP(hipSetDevice(ctx->device));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->own_stream && ctx->stream) BBK_HIP(hipStreamDestroy(ctx->stream));
        ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
        ctx->own_stream = false;
    });
}

int bbk_ctx_trim(bbk_ctx *ctx) {
    return bbk::guarded([&] {
        BBK_REQUIRE(ctx != nullptr, BBK_ERR_ARG, "bbk_ctx_trim: ctx is NULL");
        BBK_HIP(hipSetDevice(ctx->device));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        bbk::pool_trim(ctx->device);
    });
}

int bbk_ctx_memory_stats(bbk_ctx *ctx, uint64_t *mapped_now, uint64_t *mapped_total, double *map_seconds,
                         uint64_t *device_free, uint64_t *device_total) {
    return bbk::guarded([&] {
        BBK_REQUIRE(ctx != nullptr, BBK_ERR_ARG, "bbk_ctx_memory_stats: ctx is NULL");
        BBK_HIP(hipSetDevice(ctx->device));
        bbk::pool_stats(ctx->device, mapped_now, mapped_total, map_seconds);
        if (device_free || device_total) {
            size_t f = 0, t = 0;
            BBK_HIP(hipMemGetInfo(&f, &t));
            if (device_free) *device_free = f;
            if (device_total) *device_total = t;
        }
    });
}

int bbk_ctx_device_info(bbk_ctx *ctx, int *num_cus, int *num_xcds) {
    return bbk::guarded([&] {
        BBK_REQUIRE(ctx != nullptr, BBK_ERR_ARG, "bbk_ctx_device_info: ctx is NULL");
        if (num_cus) *num_cus = ctx->num_cus;
        if (num_xcds) *num_xcds = ctx->num_xcds;
    });
}

int bbk_ctx_synchronize(bbk_ctx *ctx) {
    return bbk::guarded([&] {
        BBK_REQUIRE(ctx != nullptr, BBK_ERR_ARG, "bbk_ctx_synchronize: ctx is NULL");
        BBK_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int bbk_ctx_profile_enable(bbk_ctx *ctx, int on) {
    if (!ctx) return BBK_ERR_ARG;
    ctx->profiling = on != 0;
    return BBK_OK;
}

int bbk_ctx_profile_reset(bbk_ctx *ctx) {
    if (!ctx) return BBK_ERR_ARG;
    ctx->resolve_pending();
    ctx->stats.clear();
    return BBK_OK;
}

int bbk_ctx_profile_get(bbk_ctx *ctx, const char *family, double *ms_total, uint64_t *launches, double *bytes_total) {
    if (!ctx || !family) return BBK_ERR_ARG;
    ctx->resolve_pending();
    auto it = ctx->stats.find(family);
    bbk::FamilyStat s;
    if (it != ctx->stats.end()) s = it->second;
    if (ms_total) *ms_total = s.ms;
    if (launches) *launches = s.launches;
    if (bytes_total) *bytes_total = s.bytes;
    return BBK_OK;
}

unsigned bbk_words(unsigned k) { return bbk::words_of(k); }

int bbk_staged_copy(bbk_ctx *ctx, const void *d_src, uint64_t bytes, void *h_dst, int fd) {
    return bbk::guarded([&] {
        BBK_REQUIRE(ctx && d_src && (h_dst || fd >= 0), BBK_ERR_ARG, "bbk_staged_copy: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        if (h_dst) bbk::d2h_big(ctx, h_dst, d_src, bytes);
        if (fd >= 0) BBK_REQUIRE(bbk::d2f_big(ctx, fd, 0, d_src, bytes), BBK_ERR_IO, "bbk_staged_copy: short write");
    });
}

}  // extern "C"
