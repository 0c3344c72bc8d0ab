// edge_ops.h -- the rules of an oriented edge, once, for kernels and host code alike (pairinfo.hip, distest.hip,
// distest_host.hpp, pairinfo_host.hpp, edgeprof.hip).  An oriented edge is e = 2 * segment + strand, the numbering of
// bbk_path_range.edge; the segment table holds one word per segment: its (k+1)-mers | kSegSelfConj when the segment is
// its own conjugate, which then is the one edge 2 * segment.  Standard headers only (no HIP, no bbk_internal.h).
#pragma once

#include <cstdint>

#include "host_device.h"

namespace bbk {

constexpr uint32_t kSegSelfConj = 1u << 31;  // (a segment holds fewer than 2^31 (k+1)-mers: the index has < 2^32 in all)

BBK_HOST_DEVICE inline uint32_t edge_length(uint32_t segword) { return segword & ~kSegSelfConj; }
BBK_HOST_DEVICE inline bool edge_self_conj(uint32_t segword) { return (segword & kSegSelfConj) != 0; }
template <class E>
BBK_HOST_DEVICE inline E edge_conj(E e, uint32_t segword) {
    return edge_self_conj(segword) ? e : e ^ (E)1;
}
template <class E>
BBK_HOST_DEVICE inline bool edge_exists(E e, uint32_t segword) {
    return !(e & 1) || !edge_self_conj(segword);
}

// The pair (e1, e2) is its own conjugate (conj e2, conj e1).  conj is an involution, so e1 == conj e2 gives conj e1 == e2
// as well: one comparison decides.  Spelled out it is "the same segment, and the two strands of it or the one edge of a
// self-conjugate segment", the form same_seg && (e1 != e2 || self_conj) this replaces.
template <class E>
BBK_HOST_DEVICE inline bool pair_is_self_conj(E e1, E e2, const uint32_t *seg) {
    return e1 == edge_conj(e2, seg[e2 >> 1]);
}

// The pair under which the index stores (e1, e2): the smaller of (e1, e2) and (conj e2, conj e1)
// (PairedBufferBase::InsertWithConj, common/paired_info/paired_info_buffer.hpp:103-147).  Returns whether it swapped.
template <class E>
BBK_HOST_DEVICE inline bool canonical_pair(E e1, E e2, const uint32_t *seg, E *o1, E *o2) {
    const E c1 = edge_conj(e2, seg[e2 >> 1]), c2 = edge_conj(e1, seg[e1 >> 1]);
    const bool swap = c1 < e1 || (c1 == e1 && c2 < e2);
    *o1 = swap ? c1 : e1;
    *o2 = swap ? c2 : e2;
    return swap;
}

// PairInfoPathLengthLowerBound (pair_info_bounds.hpp:23-27) in integers
BBK_HOST_DEVICE inline uint64_t path_length_lower_bound(unsigned k, uint64_t l1, uint64_t l2, int64_t gap, uint64_t delta) {
    const int64_t a = gap + (int64_t)k + 2 - (int64_t)l1 - (int64_t)l2 - (int64_t)delta;
    return a > 0 ? (uint64_t)a : 0;
}

}  // namespace bbk
