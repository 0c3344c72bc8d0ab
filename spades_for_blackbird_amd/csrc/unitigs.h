// unitigs.h -- the unitig set and what unitigs.hip (build, coverage, to_reads), unitigs_write.hip (the writers) and
// edgeprof.hip share.  Internal: the C ABI sees bbk_unitigs as an opaque handle.
#pragma once

#include <string>
#include <vector>

#include "bbk_internal.h"

// Where a result lives.
//   ON THE DEVICE when d_bases / d_uoff / d_links are set: after a build without perfect loops.
//   ON THE HOST   when bases / offsets / links are filled (on_host): after a build with perfect loops (they are
//                 appended on the host), after a build of an empty index, or once a host export has run
//                 (bbk::ensure_host).
// It can be both; the two copies are then equal, and neither is dropped again.  The counters and total_bases hold in
// every state.  Consumers that work on the device take bbk::device_view(), consumers that work on the host call
// bbk::ensure_host() first; nobody else looks at on_host.
struct bbk_unitigs {
    unsigned k = 0;
    uint64_t n = 0, n_loops = 0, n_vertices = 0, n_links = 0;
    uint64_t total_bases = 0;  // bases of all unitigs together, wherever they are
    bool has_cov = false;
    std::vector<uint64_t> kc;  // per unitig: sum of (k+1)-mer multiplicities (KC:i:)
    // device copy
    bbk::DevBuf d_bases, d_uoff, d_links;  // ACGT back to back; n + 1 offsets; 2 words per link, as `links`
    bool on_device() const { return d_uoff.p != nullptr; }
    // host copy: written by build, or later by ensure_host (hence mutable)
    mutable bool on_host = false;
    mutable bbk::raw_vector<char> bases;        // concatenated ACGT
    mutable bbk::raw_vector<uint64_t> offsets;  // n + 1
    mutable bbk::raw_vector<uint64_t> links;    // 2 per link: (from << 1 | from_plus), (to << 1 | to_plus)
};

namespace bbk {

// device -> host on the context's stream (a plain hipMemcpy runs on the null stream and would not
// wait for kernels queued on a non-blocking stream)
void d2h(bbk_ctx *ctx, void *dst, const void *src, size_t bytes);

// fills the host copy of a result that is on the device only
void ensure_host(bbk_ctx *ctx, const bbk_unitigs *u);

// The sequences on the device: the device copy in place when there is one, else the host copy uploaded into the
// caller's buffers (which must outlive the kernels that read the view).
struct UnitigView {
    const char *bases;
    const uint64_t *uoff;  // n + 1
    uint64_t total;
};
UnitigView device_view(bbk_ctx *ctx, const bbk_unitigs &u, DevBuf &up_bases, DevBuf &up_off);

// ---- sequences as plain strings: the loop path and the SPAdes-binary writer (both rare or small) ----------------
inline char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

inline std::string str_rc(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = complement(c);
    return r;
}

// 2 bits per base, base i in bits 2 (i mod 32) of word i / 32 (a Key's layout, and Sequence::BinWrite's)
inline void pack_kmer(const char *s, uint64_t k, uint64_t *w, uint64_t W) {
    for (uint64_t i = 0; i < W; ++i) w[i] = 0;
    for (uint64_t i = 0; i < k; ++i) {
        const uint64_t c = s[i] == 'A' ? 0 : s[i] == 'C' ? 1 : s[i] == 'G' ? 2 : 3;
        w[i >> 5] |= c << ((i & 31) << 1);
    }
}

inline std::string unpack_kmer(const uint64_t *w, int k) {
    std::string s((size_t)k, 'A');
    for (int i = 0; i < k; ++i) s[(size_t)i] = "ACGT"[(w[i >> 5] >> ((i & 31) << 1)) & 3];
    return s;
}

}  // namespace bbk
