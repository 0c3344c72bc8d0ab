// edgeindex.h -- the handles of the graph-mapping stage that more than one translation unit reads: the edge index
// (edgeprof.hip builds it; pairinfo.hip joins the paths of two mates over its segment table), the mapping paths of a
// batch and the paired-read info of a library.  The rules of an oriented edge over the segment table are edge_ops.h's,
// the point table of a library is pairinfo_host.hpp's.  Not part of the C ABI.
#pragma once

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "bbk_internal.h"
#include "edge_ops.h"
#include "pairinfo_host.hpp"

namespace bbk {

struct DeDeviceGraph;  // distest.hip: the graph as a CSR on the device

// one record of the edge index, 16 bytes: one dwordx4 load per found position
struct EdgePos {
    uint32_t seg;     // segment (S-line order)
    uint32_t off_fw;  // offset of the (k+1)-mer on the forward strand of the segment
    uint32_t off_rc;  // offset of its reverse complement on the reverse strand (len - 1 - off_fw)
    uint32_t flags;   // kEpCanonFw | kEpSelfConj | kEpLoop1 (gfa_graph.h)
};

}  // namespace bbk

struct bbk_edgeindex {
    unsigned k = 0, k1 = 0, W = 0;
    uint64_t n_seg = 0, n = 0;           // segments, indexed (k+1)-mers
    std::vector<std::string> names;      // segment names
    std::vector<uint64_t> len;           // (k+1)-mers per segment = |seq| - k (the reference's g.length(e))
    std::string bases;                   // the segments' ACGT back to back
    std::vector<uint64_t> off;           // n_seg + 1 offsets into bases
    std::vector<uint32_t> links;         // 4 x u32 per L line in file order: a, a is '+', b, b is '+'
    std::vector<uint32_t> kc;            // KC:i: of every segment (0 without one)
    bool has_graph = false;              // bases / off / links / kc are kept (bbk_edgeindex_from_gfa_with_graph)
    bbk::DevBuf keys;                    // n * W u64, ascending canonical (k+1)-mers
    bbk::DevBuf pos;                     // n EdgePos
    bbk::PrefixIndex prefix;             // over keys, built for k1
    bbk::DevBuf seg;                     // n_seg u32: len[s] | kSegSelfConj when the segment is its own conjugate
    std::vector<uint32_t> seg_h;         // the same on the host
    // the vertices and the CSR of the distance-estimation stage, built by the first bbk_pairinfo_cluster over the index
    mutable std::shared_ptr<bbk::DeDeviceGraph> de_graph;
    mutable std::mutex de_mutex;
};

struct bbk_profiles {
    bbk_ctx *ctx = nullptr;
    const bbk_edgeindex *ix = nullptr;
    unsigned samples = 0;
    bbk::DevBuf raw;  // n_seg * samples u64, [segment][sample]
};

struct bbk_paths {
    uint64_t n_reads = 0, n_ranges = 0;
    bbk::DevBuf ranges;  // n_ranges bbk_path_range in read order
};

// the paired-read info of one library (pairinfo.hip fills it, distest.hip clusters its points).  The calls are not a
// linear state machine: push_estimate after estimate clears `estimated`, fill_begin may be called again.
struct bbk_pairinfo {
    struct Run {  // reduced records: ascending distinct keys with their counts
        bbk::DevBuf keys, vals;
        uint64_t n = 0;
    };
    struct EstimatePass {
        uint64_t total = 0, mapped = 0, negative = 0, records = 0;
        std::vector<Run> is_runs, pair_runs;  // after bbk_pairinfo_estimate: one run each, the histogram and the pair table
        std::vector<int32_t> hist_is;
        std::vector<uint64_t> hist_count;
    };
    struct FillPass {
        uint64_t insert_size = 0, records = 0;
        uint32_t round_distance = 0, threshold = 0;
        std::vector<Run> point_runs;
    };
    bbk_ctx *ctx = nullptr;
    const bbk_edgeindex *ix = nullptr;
    uint64_t min_edge_length = 0;
    int edge_bits = 1;
    EstimatePass est;
    FillPass fill;
    bbk::PairPoints points;  // what bbk_pairinfo_fill_finish or bbk_pairinfo_import left
    bool estimated = false, filling = false, filled = false;
};

namespace bbk {
// `bytes` to the file `path` (pairinfo.hip): the end of bbk_pairinfo_write and bbk_clustered_write
void write_index_file(const char *path, const std::string &bytes);
}
