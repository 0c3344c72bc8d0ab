// subclust.hip -- BayesHammer's Bayesian subclustering of the Hamming clusters: the good bit of every k-mer (DESIGN.md
// f10, section 4.3e).
//
// Replaces KMerClustering::process / ProcessCluster / SubClusterSingle / lMeansClustering / ClusterBIC / Consensus /
// ConsensusWithMask (projects/hammer/kmer_cluster.cpp:49-633) over ExpandedKMer (kmer_stat.hpp:205-279), in the
// configuration of configs/hammer/config.info: bayes_initial_refine 1, bayes_use_hamming_dist 0, bayes_hammer_mode 0.  Inputs
// are the clusters of hamclust.hip and the statistics of kmerstat.hip.  Parity with tests/subcluster_restated.py is exact:
//   tables: logL(center) = sum over i = 0 .. k-1, from 0.0, of (center[i] == s[i] ? LP[q_i] : LR3[q_i]); LP[q] = log(1 - r(q)),
//     LR3[q] = log(r(q)) - log(3), r = hammer_error_prob (hammer.h), 64 entries each, computed on the host and uploaded.
//   log(total) of ClusterBIC: the totals of the non-singleton clusters are gathered (k_sc_totals), std::log is taken on
//     the host and the logs go back up.  The device's log is never called.
//   no contraction: `#pragma clang fp contract(off)` for the whole file; `loglik += count * logL` is a multiply and an add.
//   order: every sum or product across k-mers (totalLikelihood, curlik, loglik; cluster_quality in k_sc_mark) is taken by
//     ONE lane in member order from an LDS array the other lanes filled, one lane per k-mer.
// Kernels: k_sc_single (size 1: one lane per cluster, :463-491), k_sc_cluster<64> (2 .. 64 members: one wavefront per
// cluster) and k_sc_cluster<256> (65 .. 256: one workgroup), the same body; above 256 members -- and everything when
// BBK_SUBCLUSTER_HOST=1 -- the literal algorithm on the host under OpenMP (sc_host_cluster).  Every path leaves the lists
// of a cluster in a slab (2 x size member slots, size subcluster slots); k_sc_gather packs them in cluster order,
// k_sc_mark takes the decision of :508-556 per subcluster and k_sc_good lets the LAST subcluster that names a k-mer as its
// center set its bit, which is what the sequential loop over the clusters leaves.
#include <hip/hip_runtime.h>
#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "hammer.h"
#include "kmer_ops.h"
#include "select.h"

#pragma clang fp contract(off)

namespace bbk {

constexpr uint32_t kScNew = 0xFFFFFFFFu;  // a new k-mer in a slab (indices stay below 2^32 - 2)
constexpr int kScWave = 64, kScGroup = 256;
enum { SC_GSINGL, SC_TSINGL, SC_TCSINGL, SC_GCSINGL, SC_TCLS, SC_GCLS, SC_TKMERS, SC_TNCLS, SC_NEWKMERS };

struct ScParams {
    double singleton, nonsingleton, correct;
    int use_correct;
};

struct ScIn {
    const uint64_t *keys;
    const uint32_t *count;
    const float *tq;
    const uint64_t *qual;
    const uint32_t *members;
    const uint64_t *sizes, *off, *soff;  // per cluster: members, first member, first slab slot (non-singletons only)
    uint64_t n, clusters;
    int k, qw;
    ScParams p;
};

struct ScSlab {
    uint32_t *mem;   // 2 x slab slots
    uint32_t *size;  // slab slots
    uint64_t *nkey;  // slab slots
    uint64_t *nsub, *nmem, *nnew;  // per cluster
    double *bic;                   // per cluster
};

// SubClusterSingle:286-288 and ProcessCluster:477,545: 1 - total_qual is a float subtraction
__host__ __device__ inline bool sc_good_quality(float tq, const ScParams &p) {
    const float q = 1.0f - tq;
    return (double)q > p.singleton || (p.use_correct && (double)q > p.correct);
}

// ExpandedKMer::logL: tab[2 q + (center[i] != s[i])]; q0..q2 are the QualBitSet words of the k-mer
__host__ __device__ inline double sc_logl(uint64_t s, uint64_t c, uint64_t q0, uint64_t q1, uint64_t q2, int k,
                                          const double *tab) {
    double r = 0.0;
    uint64_t x = s ^ c;
    for (int i = 0; i < k; ++i) {
        r += tab[2 * (q0 & 63ull) + ((x & 3ull) ? 1 : 0)];
        x >>= 2;
        q0 = (q0 >> 6) | (q1 << 58);
        q1 = (q1 >> 6) | (q2 << 58);
        q2 >>= 6;
    }
    return r;
}

// bits 0..31 of v to the even bits of the result
__host__ __device__ inline uint64_t sc_spread(uint64_t v) {
    v &= 0xFFFFFFFFull;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// SubClusterSingle:330-443 after the l loop, by one lane (or one host thread): which centers are members, the merge of a
// center that duplicates another, the listing.  m members in rank order with global indices g; bestL centers bcen/bcnt;
// ind the indices of the LAST l tried (changed by the merge), bind those of the best l, cic[j] the member that is center j
// or -1.  A subcluster whose list comes out empty is dropped (:505).  Capacities: 2 m members, m subclusters, m new keys:
// the lists of several-member subclusters are disjoint (bind), every subcluster adds at most one more entry, bestL <= m.
template <class Find>
__host__ __device__ inline void sc_list(uint32_t m, uint32_t bestL, const uint64_t *bcen, uint32_t *bcnt, uint32_t *ind,
                                        const uint32_t *bind, const int *cic, const uint32_t *g, Find find, uint32_t *omem,
                                        uint32_t *osize, uint64_t *onew, uint64_t *nsub, uint64_t *nmem, uint64_t *nnew) {
    bool found_bad = true;
    while (found_bad) {
        found_bad = false;
        for (uint32_t kk = 0; kk < bestL; ++kk) {
            if (found_bad) break;
            if (bcnt[kk] == 0 || cic[kk] >= 0) continue;
            for (uint32_t s = 0; s < bestL; ++s) {
                if (s == kk || cic[s] < 0) continue;
                if (bcen[kk] != bcen[s]) continue;
                for (uint32_t i = 0; i < m; ++i)
                    if (ind[i] == kk) {
                        ind[i] = s;
                        ++bcnt[s];
                    }
                bcnt[kk] = 0;
                found_bad = true;
                break;
            }
        }
    }
    uint32_t subs = 0, pos = 0, news = 0;
    for (uint32_t kk = 0; kk < bestL; ++kk) {
        if (bcnt[kk] == 0) continue;
        uint32_t sz = 0;
        if (bcnt[kk] == 1) {
            for (uint32_t i = 0; i < m; ++i)
                if (ind[i] == kk) {
                    omem[pos + sz++] = g[i];
                    break;
                }
        } else {
            if (cic[kk] >= 0) {
                omem[pos + sz++] = g[cic[kk]];
            } else {
                const uint64_t f = find(bcen[kk]);
                if (f == ~0ull) {
                    omem[pos + sz++] = kScNew;
                    onew[news++] = bcen[kk];
                } else {
                    omem[pos + sz++] = (uint32_t)f;
                }
            }
            for (uint32_t i = 0; i < m; ++i)
                if (bind[i] == kk && (int)i != cic[kk]) omem[pos + sz++] = g[i];
        }
        if (sz == 0) continue;
        osize[subs++] = sz;
        pos += sz;
    }
    *nsub = subs;
    *nmem = pos;
    *nnew = news;
}

struct ScFindDev {
    const Key<1> *keys;
    PrefixTable P;
    __device__ uint64_t operator()(uint64_t key) const {
        Key<1> q;
        q.w[0] = key;
        return table_find<1>(keys, P, q);
    }
};

// ---- classes, offsets, totals --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sc_slab_sizes(const uint64_t *__restrict__ sizes, uint64_t C,
                                                      uint64_t *__restrict__ out) {
    const uint64_t c = BBK_GID();
    if (c < C) out[c] = sizes[c] == 1 ? 0ull : sizes[c];
}

// the clusters of a size class, in their order (an ordered selection, select.h)
struct ScSizeIn {
    const uint64_t *__restrict__ sizes;
    uint64_t lo, hi;
    __device__ bool operator()(uint64_t c) const { return sizes[c] >= lo && sizes[c] <= hi; }
};

struct ScListCluster {
    uint32_t *__restrict__ list;
    __device__ void operator()(uint64_t c, uint64_t rank) const { list[rank] = (uint32_t)c; }
};

// `unsigned total` of ClusterBIC:106-110: the sum of the counts, modulo 2^32
__global__ __launch_bounds__(256) void k_sc_totals(ScIn in, const uint32_t *__restrict__ list, uint64_t nlist,
                                                  uint32_t *__restrict__ total) {
    const uint64_t j = BBK_GID();
    if (j >= nlist) return;
    const uint32_t c = list[j];
    const uint64_t o = in.off[c], m = in.sizes[c];
    uint32_t t = 0;
    for (uint64_t i = 0; i < m; ++i) t += in.count[in.members[o + i]];
    total[j] = t;
}

// ---- size 1: ProcessCluster:463-491 -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sc_single(ScIn in, ScSlab out, uint8_t *__restrict__ cval,
                                                  unsigned long long *__restrict__ stats) {
    const uint64_t c = BBK_GID();
    const bool mine = c < in.clusters && in.sizes[c] == 1;
    bool good_singleton = false;
    if (mine) {
        const float q = 1.0f - in.tq[in.members[in.off[c]]];
        good_singleton = (double)q > in.p.singleton;
        cval[c] = good_singleton || (in.p.use_correct && (double)q > in.p.correct) ? 1 : 0;
        out.nsub[c] = 1;
        out.nmem[c] = 1;
        out.nnew[c] = 0;
        out.bic[c] = -__builtin_inf();
    }
    const unsigned long long t = __ballot(mine), gs = __ballot(good_singleton);
    if ((threadIdx.x & 63) == 0) {
        if (t) atomicAdd(&stats[SC_TSINGL], (unsigned long long)__popcll(t));
        if (gs) atomicAdd(&stats[SC_GSINGL], (unsigned long long)__popcll(gs));
    }
}

// ---- 2 .. NT members: SubClusterSingle, one lane per k-mer -----------------------------------------------------------
// ConsensusWithMask / Consensus for one center: integer scores in LDS, the first maximum of every position, the center
// as one key word.  Called by every lane of the workgroup.
template <int NT>
__device__ inline void sc_consensus(unsigned long long *sc, uint64_t *center, bool take, uint64_t key, uint32_t cnt, int k) {
    const int lane = threadIdx.x;
    for (int t = lane; t < 4 * k; t += NT) sc[t] = 0ull;
    __syncthreads();
    if (take) {
        uint64_t x = key;
        for (int i = 0; i < k; ++i) {
            atomicAdd(&sc[4 * i + (int)(x & 3ull)], (unsigned long long)cnt);
            x >>= 2;
        }
    }
    __syncthreads();
    uint32_t b = 0;
    if (lane < k) {
        unsigned long long best = sc[4 * lane];
#pragma unroll
        for (uint32_t j = 1; j < 4; ++j) {
            const unsigned long long v = sc[4 * lane + j];
            if (best < v) {
                best = v;
                b = j;
            }
        }
    }
    // k <= 32: the positions are lanes of the first wavefront
    const unsigned long long m0 = __ballot(lane < k && (b & 1u)), m1 = __ballot(lane < k && (b & 2u));
    if (lane == 0) *center = sc_spread(m0) | (sc_spread(m1) << 1);
    __syncthreads();
}

template <int NT>
__global__ __launch_bounds__(NT) void k_sc_cluster(ScIn in, PrefixTable P, const uint32_t *__restrict__ list,
                                                  uint64_t nlist, const double *__restrict__ logtot,
                                                  const double *__restrict__ tab, ScSlab out) {
    __shared__ uint64_t s_key[NT], s_cen[NT], s_bcen[NT];
    __shared__ double s_lik[NT], s_tab[128];
    __shared__ unsigned long long s_sc[128];
    __shared__ uint32_t s_cnt[NT], s_g[NT], s_ccnt[NT], s_bcnt[NT], s_ind[NT], s_bind[NT], s_chg[NT];
    __shared__ int s_cic[NT];
    __shared__ uint32_t s_ctl[2];
    const uint64_t li = ((uint64_t)blockIdx.y * gridDim.x) + blockIdx.x;
    if (li >= nlist) return;
    const uint32_t c = list[li];
    const uint32_t m = (uint32_t)in.sizes[c];  // 2 .. NT
    const uint64_t o = in.off[c], so = in.soff[c];
    const int lane = threadIdx.x, k = in.k;
    const bool active = (uint32_t)lane < m;
    const double ltot = logtot[li];

    // the members by (count descending, index ascending): they arrive ascending by index
    uint32_t g = 0, cn = 0;
    if (active) {
        g = in.members[o + lane];
        cn = in.count[g];
    }
    s_cnt[lane] = cn;
    for (int t = lane; t < 128; t += NT) s_tab[t] = tab[t];
    __syncthreads();
    if (active) {
        uint32_t r = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t cj = s_cnt[j];
            r += (cj > cn || (cj == cn && j < (uint32_t)lane)) ? 1u : 0u;
        }
        s_ind[r] = g;
    }
    __syncthreads();
    uint64_t key = 0, q0 = 0, q1 = 0, q2 = 0;
    float tq = 1.0f;
    cn = 0;
    if (active) {
        g = s_ind[lane];
        key = in.keys[g];
        cn = in.count[g];
        tq = in.tq[g];
        const uint64_t *q = in.qual + (uint64_t)g * (uint64_t)in.qw;
        q0 = q[0];
        if (in.qw > 1) q1 = q[1];
        if (in.qw > 2) q2 = q[2];
    }
    __syncthreads();
    s_key[lane] = key;
    s_cnt[lane] = cn;
    s_g[lane] = g;
    __syncthreads();
    // maxcls, SubClusterSingle:277-292
    const uint32_t top = s_cnt[0] / 10u;
    const uint32_t cntthr = top > 10u ? top : 10u;
    const uint32_t over = (uint32_t)__syncthreads_count(active && cn > cntthr);
    const uint32_t goodq = (uint32_t)__syncthreads_count(active && sc_good_quality(tq, in.p));
    const uint32_t maxcls = (over < goodq ? over : goodq) + 1u;

    uint32_t ind = 0, bind = 0, bestL = 0;
    double best_lik = -__builtin_inf();  // lane 0's
    for (uint32_t l = 1; l <= m; ++l) {
        if (l == 1) {
            sc_consensus<NT>(s_sc, &s_cen[0], active, key, cn, k);
            if (lane == 0) s_ccnt[0] = m;
            ind = 0;
        } else {
            // the initial approximation (bayes_initial_refine), lMeansClustering:140-152
            double total_lik = 0.0;  // lane 0's
            if (lane == 0) s_cen[l - 1] = s_key[l - 1];
            __syncthreads();
            if (active) {
                const uint32_t cdist = kmer_hamdist(key, s_cen[ind]);
                const uint32_t mdist = kmer_hamdist(key, s_cen[l - 1]);  // cut off at cdist there: only `<` is read
                if (mdist < cdist) ind = l - 1;
                s_lik[lane] = sc_logl(key, s_cen[ind], q0, q1, q2, k, s_tab);
            }
            __syncthreads();
            if (lane == 0)
                for (uint32_t i = 0; i < m; ++i) total_lik += s_lik[i];
            for (;;) {
                if ((uint32_t)lane < l) {
                    s_ccnt[lane] = 0;
                    s_chg[lane] = 0;
                }
                if (lane == 0) s_ctl[0] = 0;
                __syncthreads();
                if (active) {  // E step
                    double best = sc_logl(key, s_cen[0], q0, q1, q2, k, s_tab);
                    uint32_t bi = 0;
                    for (uint32_t j = 1; j < l; ++j) {
                        const double v = sc_logl(key, s_cen[j], q0, q1, q2, k, s_tab);
                        if (best < v) {
                            best = v;
                            bi = j;
                        }
                    }
                    s_lik[lane] = best;
                    if (ind != bi) {
                        s_chg[ind] = 1;
                        s_chg[bi] = 1;
                        s_ctl[0] = 1;
                        ind = bi;
                    }
                    atomicAdd(&s_ccnt[ind], 1u);
                }
                __syncthreads();
                if (lane == 0) {
                    double curlik = 0.0;
                    for (uint32_t i = 0; i < m; ++i) curlik += s_lik[i];
                    const bool improved = curlik > total_lik;
                    if (improved) total_lik = curlik;
                    s_ctl[1] = (s_ctl[0] && improved) ? 1u : 0u;
                }
                __syncthreads();
                for (uint32_t j = 0; j < l; ++j)  // M step
                    if (s_chg[j]) sc_consensus<NT>(s_sc, &s_cen[j], active && ind == j, key, cn, k);
                const bool go_on = s_ctl[1] != 0;
                __syncthreads();
                if (!go_on) break;
            }
            for (uint32_t j = 0; j < l; ++j) sc_consensus<NT>(s_sc, &s_cen[j], active && ind == j, key, cn, k);
        }
        // ClusterBIC
        if (active) s_lik[lane] = sc_logl(key, s_cen[ind], q0, q1, q2, k, s_tab);
        __syncthreads();
        if (lane == 0) {
            double loglik = 0.0;
            for (uint32_t i = 0; i < m; ++i) loglik += (double)s_cnt[i] * s_lik[i];
            const uint64_t nparams = (uint64_t)(l - 1) + (uint64_t)l * (uint64_t)k + 2ull * l * (uint64_t)k;
            const double cur = loglik - (double)nparams * ltot / 2.0;
            uint32_t what = 0;
            if (cur > best_lik) {
                best_lik = cur;
                what = 1;
            } else if (l >= maxcls) {
                what = 2;
            }
            s_ctl[0] = what;
        }
        __syncthreads();
        const uint32_t what = s_ctl[0];
        if (what == 1) {
            if ((uint32_t)lane < l) {
                s_bcen[lane] = s_cen[lane];
                s_bcnt[lane] = s_ccnt[lane];
            }
            bind = ind;
            bestL = l;
        }
        __syncthreads();
        if (what == 2) break;
    }
    // which centers are members of their own subcluster (:330-337): keys are distinct, so at most one member each
    s_ind[lane] = ind;
    s_bind[lane] = bind;
    if ((uint32_t)lane < bestL) s_cic[lane] = -1;
    __syncthreads();
    if (active && key == s_bcen[bind]) s_cic[bind] = lane;
    __syncthreads();
    if (lane == 0) {
        ScFindDev find{reinterpret_cast<const Key<1> *>(in.keys), P};
        sc_list(m, bestL, s_bcen, s_bcnt, s_ind, s_bind, s_cic, s_g, find, out.mem + 2 * so, out.size + so, out.nkey + so,
                &out.nsub[c], &out.nmem[c], &out.nnew[c]);
        out.bic[c] = best_lik;
    }
}

// ---- the host path: the literal algorithm, one cluster --------------------------------------------------------------
namespace {

struct ScHost {
    int k, qw;
    ScParams p;
    const double *tab;
    std::vector<uint64_t> keys, qual, sizes, off;
    std::vector<uint32_t> count, members;
    std::vector<float> tq;
};

struct HostKMer {  // ExpandedKMer
    uint64_t key;
    uint32_t count;
    uint64_t q[3];
};

uint64_t sc_host_consensus(const std::vector<HostKMer> &kmers, const std::vector<uint32_t> *mask, uint32_t val, int k) {
    if (kmers.size() == 1) return kmers[0].key;
    uint64_t scores[4 * 32] = {0};
    for (size_t j = 0; j < kmers.size(); ++j) {
        if (mask && (*mask)[j] != val) continue;
        for (int i = 0; i < k; ++i) scores[4 * i + ((kmers[j].key >> (2 * i)) & 3ull)] += kmers[j].count;
    }
    uint64_t res = 0;
    for (int i = 0; i < k; ++i)
        res |= (uint64_t)(std::max_element(scores + 4 * i, scores + 4 * i + 4) - (scores + 4 * i)) << (2 * i);
    return res;
}

double sc_host_logl(const HostKMer &km, uint64_t center, const ScHost &h) {
    return sc_logl(km.key, center, km.q[0], km.q[1], km.q[2], h.k, h.tab);
}

double sc_host_bic(const std::vector<uint64_t> &centers, const std::vector<uint32_t> &indices,
                   const std::vector<HostKMer> &kmers, const ScHost &h) {
    double loglik = 0;
    unsigned total = 0;
    for (size_t i = 0; i < kmers.size(); ++i) {
        loglik += kmers[i].count * sc_host_logl(kmers[i], centers[indices[i]], h);
        total += kmers[i].count;
    }
    const size_t clusters = centers.size(), K = (size_t)h.k;
    const size_t nparams = (clusters - 1) + clusters * K + 2 * clusters * K;
    return loglik - (double)nparams * std::log((double)total) / 2.0;
}

double sc_host_lmeans(unsigned l, const std::vector<HostKMer> &kmers, std::vector<uint32_t> &indices,
                      std::vector<uint64_t> &centers, std::vector<uint32_t> &ccount, const ScHost &h) {
    centers.resize(l);
    ccount.resize(l);
    if (l == 1) {
        centers[0] = sc_host_consensus(kmers, nullptr, 0, h.k);
        ccount[0] = (uint32_t)kmers.size();
        for (size_t i = 0; i < kmers.size(); ++i) indices[i] = 0;
        return sc_host_bic(centers, indices, kmers, h);
    }
    double totalLikelihood = 0.0;
    centers[l - 1] = kmers[l - 1].key;
    for (size_t i = 0; i < kmers.size(); ++i) {
        uint32_t cidx = indices[i];
        const uint32_t cdist = kmer_hamdist(kmers[i].key, centers[cidx]);
        const uint32_t mdist = kmer_hamdist(kmers[i].key, centers[l - 1]);
        if (mdist < cdist) {
            indices[i] = l - 1;
            cidx = l - 1;
        }
        totalLikelihood += sc_host_logl(kmers[i], centers[cidx], h);
    }
    bool changed = true, improved = true;
    std::vector<double> loglike(l);
    std::vector<char> changedCenter(l);
    while (changed && improved) {
        changed = false;
        std::fill(changedCenter.begin(), changedCenter.end(), 0);
        for (unsigned j = 0; j < l; ++j) ccount[j] = 0;
        double curlik = 0;
        for (size_t i = 0; i < kmers.size(); ++i) {
            for (unsigned j = 0; j < l; ++j) loglike[j] = sc_host_logl(kmers[i], centers[j], h);
            const uint32_t newInd = (uint32_t)(std::max_element(loglike.begin(), loglike.end()) - loglike.begin());
            curlik += loglike[newInd];
            if (indices[i] != newInd) {
                changed = true;
                changedCenter[indices[i]] = 1;
                changedCenter[newInd] = 1;
                indices[i] = newInd;
            }
            ++ccount[indices[i]];
        }
        improved = curlik > totalLikelihood;
        if (improved) totalLikelihood = curlik;
        for (unsigned j = 0; j < l; ++j)
            if (changedCenter[j]) centers[j] = sc_host_consensus(kmers, &indices, j, h.k);
    }
    for (unsigned j = 0; j < l; ++j) centers[j] = sc_host_consensus(kmers, &indices, j, h.k);
    return sc_host_bic(centers, indices, kmers, h);
}

// the lists of cluster c into its staging slots (2 m, m and m of them, zero so far), counts = {subclusters, members, new}
void sc_host_cluster(const ScHost &h, uint32_t c, uint32_t *mem, uint32_t *size, uint64_t *nkey, uint64_t *counts, double *bic) {
    const uint32_t m = (uint32_t)h.sizes[c];
    std::vector<uint32_t> g(h.members.begin() + h.off[c], h.members.begin() + h.off[c] + m);
    std::sort(g.begin(), g.end(), [&](uint32_t a, uint32_t b) {
        return h.count[a] != h.count[b] ? h.count[a] > h.count[b] : a < b;
    });
    size_t maxcls = 0, maxgcnt = 0;
    const size_t cntthr = std::max(10u, h.count[g[0]] / 10);
    for (uint32_t i : g) {
        maxcls += h.count[i] > cntthr;
        maxgcnt += sc_good_quality(h.tq[i], h.p);
    }
    maxcls = std::min(maxcls, maxgcnt) + 1;
    std::vector<HostKMer> kmers(m);
    for (uint32_t i = 0; i < m; ++i) {
        kmers[i].key = h.keys[g[i]];
        kmers[i].count = h.count[g[i]];
        for (int w = 0; w < 3; ++w) kmers[i].q[w] = w < h.qw ? h.qual[(uint64_t)g[i] * h.qw + w] : 0ull;
    }
    double bestLikelihood = -std::numeric_limits<double>::infinity();
    std::vector<uint64_t> centers, bestCenters;
    std::vector<uint32_t> ccount, bestCount, indices(m, 0), bestIndices(m, 0);
    for (unsigned l = 1; l <= m; ++l) {
        const double cur = sc_host_lmeans(l, kmers, indices, centers, ccount, h);
        if (cur > bestLikelihood) {
            bestLikelihood = cur;
            bestCenters = centers;
            bestCount = ccount;
            bestIndices = indices;
        } else if (l >= maxcls) {
            break;
        }
    }
    const uint32_t bestL = (uint32_t)bestCenters.size();
    std::vector<int> cic(bestL, -1);
    for (uint32_t i = 0; i < m; ++i)
        if (kmers[i].key == bestCenters[bestIndices[i]]) cic[bestIndices[i]] = (int)i;
    auto find = [&](uint64_t key) {
        const auto it = std::lower_bound(h.keys.begin(), h.keys.end(), key);
        return it != h.keys.end() && *it == key ? (uint64_t)(it - h.keys.begin()) : ~0ull;
    };
    sc_list(m, bestL, bestCenters.data(), bestCount.data(), indices.data(), bestIndices.data(), cic.data(), g.data(),
            find, mem, size, nkey, &counts[0], &counts[1], &counts[2]);
    *bic = bestLikelihood;
}

}  // namespace

// one lane per host cluster: its lists from the staging arrays into its slab
__global__ __launch_bounds__(256) void k_sc_host_scatter(ScIn in, const uint32_t *__restrict__ list, uint64_t nlist,
                                                        const uint64_t *__restrict__ hoff, const uint32_t *__restrict__ hmem,
                                                        const uint32_t *__restrict__ hsize, const uint64_t *__restrict__ hkey,
                                                        const uint64_t *__restrict__ hcounts, const double *__restrict__ hbic,
                                                        ScSlab out) {
    const uint64_t j = BBK_GID();
    if (j >= nlist) return;
    const uint32_t c = list[j];
    const uint64_t so = in.soff[c], ho = hoff[j];
    const uint64_t nsub = hcounts[3 * j], nmem = hcounts[3 * j + 1], nnew = hcounts[3 * j + 2];
    for (uint64_t i = 0; i < nmem; ++i) out.mem[2 * so + i] = hmem[2 * ho + i];
    for (uint64_t i = 0; i < nsub; ++i) out.size[so + i] = hsize[ho + i];
    for (uint64_t i = 0; i < nnew; ++i) out.nkey[so + i] = hkey[ho + i];
    out.nsub[c] = nsub;
    out.nmem[c] = nmem;
    out.nnew[c] = nnew;
    out.bic[c] = hbic[j];
}

// ---- the lists in cluster order, the decisions, the good bits -------------------------------------------------------
// per_cluster holds the subcluster counts: by now s.nsub / nmem / nnew hold the scanned offsets (sub_off, mem_off, new_off)
__global__ __launch_bounds__(256) void k_sc_gather(ScIn in, ScSlab s, const uint64_t *__restrict__ per_cluster,
                                                  const uint64_t *__restrict__ sub_off,
                                                  const uint64_t *__restrict__ mem_off, const uint64_t *__restrict__ new_off,
                                                  uint64_t *__restrict__ d_mem, uint64_t *__restrict__ d_size,
                                                  uint64_t *__restrict__ d_first, uint32_t *__restrict__ d_cluster,
                                                  uint64_t *__restrict__ d_new) {
    const uint64_t c = BBK_GID();
    if (c >= in.clusters) return;
    const uint64_t s0 = sub_off[c], m0 = mem_off[c], n0 = new_off[c];
    if (in.sizes[c] == 1) {
        d_mem[m0] = in.members[in.off[c]];
        d_size[s0] = 1;
        d_first[s0] = m0;
        d_cluster[s0] = (uint32_t)c;
        return;
    }
    const uint64_t so = in.soff[c], nsub = per_cluster[c];
    uint64_t p = 0, nn = 0;
    for (uint64_t t = 0; t < nsub; ++t) {
        const uint64_t sz = s.size[so + t];
        d_size[s0 + t] = sz;
        d_first[s0 + t] = m0 + p;
        d_cluster[s0 + t] = (uint32_t)c;
        for (uint64_t j = 0; j < sz; ++j) {
            const uint32_t v = s.mem[2 * so + p + j];
            if (v == kScNew) {
                d_new[n0 + nn] = s.nkey[so + nn];
                d_mem[m0 + p + j] = in.n + n0 + nn;
                ++nn;
            } else {
                d_mem[m0 + p + j] = v;
            }
        }
        p += sz;
    }
}

// ProcessCluster:503-574 for one subcluster per lane: the decision on its center, the counters, UpdateErrors
__global__ __launch_bounds__(256) void k_sc_mark(ScIn in, uint64_t subs, const uint64_t *__restrict__ d_mem,
                                                const uint64_t *__restrict__ d_size, const uint64_t *__restrict__ d_first,
                                                const uint32_t *__restrict__ d_cluster, const uint64_t *__restrict__ d_new,
                                                const uint8_t *__restrict__ cval, uint8_t *__restrict__ sval,
                                                unsigned long long *__restrict__ last, unsigned long long *__restrict__ stats,
                                                unsigned long long *__restrict__ errs) {
    __shared__ unsigned long long s_acc[32];
    if (threadIdx.x < 32) s_acc[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t s = BBK_GID();
    if (s < subs) {
        const uint64_t f = d_first[s], sz = d_size[s], cidx = d_mem[f];
        const uint32_t c = d_cluster[s];
        uint8_t val;
        if (in.sizes[c] == 1) {
            val = cval[c];
        } else {
            const float ctq = cidx < in.n ? in.tq[cidx] : 1.0f;  // a new k-mer is KMerStat(0, 1.0, NULL)
            const double center_quality = (double)(1.0f - ctq);
            double cluster_quality = 1;
            if (sz > 1) {
                for (uint64_t j = 1; j < sz; ++j) cluster_quality *= (double)in.tq[d_mem[f + j]];
                cluster_quality = 1 - cluster_quality;
            }
            const bool good_cluster = center_quality > in.p.singleton && cluster_quality > in.p.nonsingleton;
            val = good_cluster || (in.p.use_correct && center_quality > in.p.correct) ? 1 : 0;
            atomicAdd(&s_acc[sz == 1 ? SC_TCSINGL : SC_TCLS], 1ull);
            if (good_cluster) atomicAdd(&s_acc[sz == 1 ? SC_GCSINGL : SC_GCLS], 1ull);
            atomicAdd(&s_acc[SC_TKMERS], (unsigned long long)sz);
            const uint64_t ckey = cidx < in.n ? in.keys[cidx] : d_new[cidx - in.n];
            for (uint64_t j = 1; j < sz; ++j) {
                uint64_t a = ckey, b = in.keys[d_mem[f + j]];
                for (int i = 0; i < in.k; ++i) {
                    atomicAdd(&s_acc[16 + 4 * (int)(a & 3ull) + (int)(b & 3ull)], 1ull);
                    a >>= 2;
                    b >>= 2;
                }
            }
        }
        sval[s] = val;
        atomicMax(&last[cidx], (unsigned long long)(s + 1));
    }
    __syncthreads();
    if (threadIdx.x < 32 && s_acc[threadIdx.x]) {
        if (threadIdx.x < 16) atomicAdd(&stats[threadIdx.x], s_acc[threadIdx.x]);
        else atomicAdd(&errs[threadIdx.x - 16], s_acc[threadIdx.x]);
    }
}

// the later subcluster's mark stands (the sequential loop over clusters and subclusters)
__global__ __launch_bounds__(256) void k_sc_good(uint64_t subs, const uint64_t *__restrict__ d_mem,
                                                const uint64_t *__restrict__ d_first, const uint8_t *__restrict__ sval,
                                                const unsigned long long *__restrict__ last, uint8_t *__restrict__ good) {
    const uint64_t s = BBK_GID();
    if (s >= subs) return;
    const uint64_t cidx = d_mem[d_first[s]];
    if (last[cidx] == s + 1) good[cidx] = sval[s];
}

// ---- the driver: layout, solve, finish over one state ------------------------------------------------------------------
struct ScRun {
    bbk_ctx *ctx;
    bbk_subclusters *sc;
    PrefixTable P;  // over the keys of the set: is a center one of them?
    ScIn in;
    ScSlab slab;
    double tab[128];  // LP[q], LR3[q] interleaved (kmer_stat.hpp:211-213)
    DevBuf d_tab, off, soff, s_mem, s_size, s_nkey, nsub, nmem, nnew, cval, d_stats;  // d_stats: 16 counters, 16 error counts

    // offsets of the clusters in the member list and in the slabs, the kernels' view of the inputs, the slab buffers
    void layout(const bbk_kmerset *set, const bbk_hamclusters *hc, const bbk_kmerstats *ks, const ScParams &p) {
        const uint64_t C = hc->clusters, *sizes = hc->sizes.as<uint64_t>();
        P = ks->prefix.table();
        for (unsigned q = 0; q < 64; ++q) {
            const double r = hammer_error_prob(q);
            tab[2 * q] = log(1 - r);
            tab[2 * q + 1] = log(r) - log(3);
        }
        upload(ctx, d_tab, tab, 128);  // this outlives the waits below
        for (DevBuf *b : {&off, &soff}) b->alloc((C + 1) * 8);
        exclusive_scan_u64(ctx, sizes, off.as<uint64_t>(), C);
        launch_items(ctx, "sc_classes", k_sc_slab_sizes, C, sizes, C, soff.as<uint64_t>());
        const uint64_t slots = exclusive_scan_u64(ctx, soff.as<uint64_t>(), soff.as<uint64_t>(), C);
        in = ScIn{set->keys.as<uint64_t>(), ks->count.as<uint32_t>(), ks->total_qual.as<float>(), ks->qual.as<uint64_t>(),
                  hc->members.as<uint32_t>(), sizes, off.as<uint64_t>(), soff.as<uint64_t>(), set->n, C, (int)set->k,
                  (int)ks->qual_words, p};
        s_mem.alloc(2 * slots * 4);
        s_size.alloc(slots * 4);
        s_nkey.alloc(slots * 8);
        for (DevBuf *b : {&nsub, &nmem, &nnew}) b->alloc((C + 1) * 8);
        cval.alloc(C);
        d_stats.alloc(32 * 8);
        sc->bic.alloc(C * 8);
        slab = ScSlab{s_mem.as<uint32_t>(), s_size.as<uint32_t>(), s_nkey.as<uint64_t>(), nsub.as<uint64_t>(), nmem.as<uint64_t>(),
                      nnew.as<uint64_t>(), sc->bic.as<double>()};
        BBK_HIP(hipMemsetAsync(d_stats.p, 0, 32 * 8, ctx->stream));
    }

    // The clusters of `list` on the host; returns the k-mers they hold.
    uint64_t run_host(const DevBuf &list, uint64_t nlist) {
        ScHost h{in.k, in.qw, in.p, tab};
        std::vector<uint32_t> cl;
        auto fetch = [&](auto &v, const void *src, uint64_t cnt) { v.resize(cnt), d2h_big(ctx, v.data(), src, cnt * sizeof(v[0])); };
        fetch(h.keys, in.keys, in.n);
        fetch(h.count, in.count, in.n);
        fetch(h.tq, in.tq, in.n);
        fetch(h.qual, in.qual, in.n * in.qw);
        fetch(h.members, in.members, in.n);
        fetch(h.sizes, in.sizes, in.clusters);
        fetch(h.off, in.off, in.clusters);
        fetch(cl, list.p, nlist);
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint64_t> hoff(nlist + 1, 0);
        for (uint64_t j = 0; j < nlist; ++j) hoff[j + 1] = hoff[j] + h.sizes[cl[j]];
        const uint64_t slots = hoff[nlist];
        std::vector<uint32_t> hmem(2 * slots), hsize(slots);
        std::vector<uint64_t> hkey(slots), hcounts(3 * nlist);
        std::vector<double> hbic(nlist);
#pragma omp parallel for schedule(dynamic, 16)
        for (long long j = 0; j < (long long)nlist; ++j)
            sc_host_cluster(h, cl[j], &hmem[2 * hoff[j]], &hsize[hoff[j]], &hkey[hoff[j]], &hcounts[3 * j], &hbic[j]);
        ctx->add_stat("stat_sc_host_us", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        DevBuf d_hoff, d_hmem, d_hsize, d_hkey, d_hcounts, d_hbic;
        upload(ctx, d_hoff, hoff.data(), nlist + 1);
        upload(ctx, d_hmem, hmem.data(), 2 * slots);
        upload(ctx, d_hsize, hsize.data(), slots);
        upload(ctx, d_hkey, hkey.data(), slots);
        upload(ctx, d_hcounts, hcounts.data(), 3 * nlist);
        upload(ctx, d_hbic, hbic.data(), nlist);
        launch_items_timed(ctx, "sc_host_scatter", k_sc_host_scatter, nlist, in, list.as<uint32_t>(), nlist, d_hoff.as<uint64_t>(),
                           d_hmem.as<uint32_t>(), d_hsize.as<uint32_t>(), d_hkey.as<uint64_t>(), d_hcounts.as<uint64_t>(),
                           d_hbic.as<double>(), slab);
        BBK_HIP(hipStreamSynchronize(ctx->stream));  // the staging vectors are on this frame
        return slots;
    }

    // The clusters of `list` by k_sc_cluster<NT>; none of their k-mers is the host's.
    template <int NT>
    uint64_t run_device(const DevBuf &list, uint64_t nlist) {
        const char *family = NT == kScWave ? "sc_wave" : "sc_group";
        // log((double)total) of every cluster of the class, from the host's libm
        DevBuf d_total(nlist * 4), d_log(nlist * 8);
        launch_items(ctx, "sc_totals", k_sc_totals, nlist, in, list.as<uint32_t>(), nlist, d_total.as<uint32_t>());
        raw_vector<uint32_t> total(nlist);
        d2h_big(ctx, total.data(), d_total.p, nlist * 4);
        raw_vector<double> lg(nlist);
        for (uint64_t j = 0; j < nlist; ++j) lg[j] = std::log((double)total[j]);
        BBK_HIP(hipMemcpyAsync(d_log.p, lg.data(), nlist * 8, hipMemcpyHostToDevice, ctx->stream));
        {
            KernelTimer t(ctx, family);
            hipLaunchKernelGGL(k_sc_cluster<NT>, grid_blocks(nlist), dim3(NT), 0, ctx->stream, in, P, list.as<uint32_t>(), nlist,
                               d_log.as<double>(), d_tab.as<double>(), slab);
            check_launch(family);
        }
        BBK_HIP(hipStreamSynchronize(ctx->stream));  // lg is on this frame
        return 0;
    }

    // the singletons, then class after class: who solves the clusters of lo .. hi members, and the stat (may be null) that
    // receives how many there are.  Returns the number of non-singleton clusters.
    uint64_t solve() {
        struct Class {
            uint64_t lo, hi;
            uint64_t (ScRun::*run)(const DevBuf &list, uint64_t nlist);
            const char *stat;
        };
        const char *env = getenv("BBK_SUBCLUSTER_HOST");
        const bool host = env && atoi(env) != 0;  // then the last row takes every class
        const Class by_size[] = {{2, kScWave, &ScRun::run_device<kScWave>, "stat_sc_wave_clusters"},
                                 {kScWave + 1, kScGroup, &ScRun::run_device<kScGroup>, "stat_sc_group_clusters"},
                                 {host ? 2ull : kScGroup + 1ull, ~0ull, &ScRun::run_host, nullptr}};
        const uint64_t C = in.clusters;
        launch_items_timed(ctx, "sc_single", k_sc_single, C, in, slab, cval.as<uint8_t>(), d_stats.as<unsigned long long>());
        uint64_t non_singletons = 0;
        DevBuf list;
        for (const Class *c = by_size + (host ? 2 : 0); c < by_size + 3; ++c) {
            const auto in_class = per_item(ScSizeIn{in.sizes, c->lo, c->hi});
            const Selection sel = select_count(ctx, "sc_classes", C, in_class);
            const uint64_t cnt = sel.kept;
            list.alloc(cnt * 4);
            select_write(ctx, "sc_classes", sel, in_class, ScListCluster{list.as<uint32_t>()});
            non_singletons += cnt;
            if (c->stat) ctx->add_stat(c->stat, (double)cnt);
            if (cnt) sc->host_kmers += (this->*c->run)(list, cnt);
        }
        return non_singletons;
    }

    // the lists in cluster order, the decision per subcluster, the good bits, the counters
    void finish(uint64_t non_singletons) {
        const uint64_t C = in.clusters;
        unsigned long long *stats = d_stats.as<unsigned long long>(), *errs = stats + 16;
        uint64_t *sub_off = nsub.as<uint64_t>(), *mem_off = nmem.as<uint64_t>(), *new_off = nnew.as<uint64_t>();
        sc->per_cluster.alloc(C * 8);
        BBK_HIP(copy_async(sc->per_cluster.p, nsub.p, C * 8, hipMemcpyDeviceToDevice, ctx->stream));
        sc->subs = exclusive_scan_u64(ctx, sub_off, sub_off, C);
        sc->listed = exclusive_scan_u64(ctx, mem_off, mem_off, C);
        sc->new_kmers = exclusive_scan_u64(ctx, new_off, new_off, C);
        const uint64_t S = sc->subs, total = in.n + sc->new_kmers;
        sc->members.alloc(sc->listed * 8);
        sc->sizes.alloc(S * 8);
        sc->new_keys.alloc(sc->new_kmers * 8);
        sc->good.alloc(total);
        DevBuf first(S * 8), cluster(S * 4), sval(S), last(total * 8);
        BBK_HIP(hipMemsetAsync(sc->good.p, 0, total, ctx->stream));
        BBK_HIP(hipMemsetAsync(last.p, 0, total * 8, ctx->stream));
        {
            KernelTimer t(ctx, "sc_finish");
            launch_items(ctx, "sc_gather", k_sc_gather, C, in, slab, sc->per_cluster.as<uint64_t>(), sub_off, mem_off, new_off,
                         sc->members.as<uint64_t>(), sc->sizes.as<uint64_t>(), first.as<uint64_t>(), cluster.as<uint32_t>(),
                         sc->new_keys.as<uint64_t>());
            launch_items(ctx, "sc_mark", k_sc_mark, S, in, S, sc->members.as<uint64_t>(), sc->sizes.as<uint64_t>(),
                         first.as<uint64_t>(), cluster.as<uint32_t>(), sc->new_keys.as<uint64_t>(), cval.as<uint8_t>(),
                         sval.as<uint8_t>(), last.as<unsigned long long>(), stats, errs);
            launch_items(ctx, "sc_good", k_sc_good, S, S, sc->members.as<uint64_t>(), first.as<uint64_t>(), sval.as<uint8_t>(),
                         last.as<unsigned long long>(), sc->good.as<uint8_t>());
        }
        uint64_t h_stats[32];
        BBK_HIP(hipMemcpyAsync(h_stats, d_stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, ctx->stream));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        memcpy(sc->stats, h_stats, sizeof(sc->stats));
        memcpy(sc->errs, h_stats + 16, sizeof(sc->errs));
        sc->stats[SC_TNCLS] = non_singletons;
        sc->stats[SC_NEWKMERS] = sc->new_kmers;
    }
};

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_hamclusters_subcluster(bbk_ctx *ctx, const bbk_kmerset *set, const bbk_hamclusters *hamclusters,
                               const bbk_kmerstats *kmerstats, const bbk_subcluster_params *p, bbk_subclusters **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && hamclusters && kmerstats && out, BBK_ERR_ARG, "bbk_hamclusters_subcluster: NULL argument");
        BBK_REQUIRE(kmerstats->set == set, BBK_ERR_ARG,
                    "bbk_hamclusters_subcluster: the statistics were made for another k-mer set");
        BBK_REQUIRE(hamclusters->n == set->n && kmerstats->n == set->n, BBK_ERR_ARG,
                    "bbk_hamclusters_subcluster: the set has %llu k-mers, the clusters %llu, the statistics %llu",
                    (unsigned long long)set->n, (unsigned long long)hamclusters->n, (unsigned long long)kmerstats->n);
        BBK_REQUIRE(kmerstats->finished, BBK_ERR_ARG,
                    "bbk_hamclusters_subcluster: call bbk_kmerstats_finish after the last push");
        bbk_subcluster_params d = {0.995, 0.9, 0.98, 1};  // configs/hammer/config.info
        if (p) d = *p;
        for (double t : {d.singleton_threshold, d.nonsingleton_threshold, d.correct_threshold})
            BBK_REQUIRE(t >= 0.0 && t <= 1.0, BBK_ERR_ARG, "bbk_hamclusters_subcluster: threshold %g is outside [0, 1]", t);
        const ScParams sp{d.singleton_threshold, d.nonsingleton_threshold, d.correct_threshold, d.correct_use_threshold ? 1 : 0};
        BBK_HIP(hipSetDevice(ctx->device));
        auto sc = std::make_unique<bbk_subclusters>();
        sc->k = set->k;
        sc->n = set->n;
        sc->clusters = hamclusters->clusters;
        for (DevBuf *b : {&sc->good, &sc->members, &sc->sizes, &sc->per_cluster, &sc->new_keys, &sc->bic}) b->alloc(16);
        if (sc->n) {
            ScRun r{ctx, sc.get()};
            r.layout(set, hamclusters, kmerstats, sp);
            r.finish(r.solve());
        }
        *out = sc.release();
    });
}

uint64_t bbk_subclusters_count(const bbk_subclusters *s) { return s ? s->subs : 0; }
uint64_t bbk_subclusters_size(const bbk_subclusters *s) { return s ? s->listed : 0; }
uint64_t bbk_subclusters_new_kmers(const bbk_subclusters *s) { return s ? s->new_kmers : 0; }
uint64_t bbk_subclusters_host_kmers(const bbk_subclusters *s) { return s ? s->host_kmers : 0; }

int bbk_subclusters_export(bbk_ctx *ctx, const bbk_subclusters *s, uint8_t *h_good, uint64_t *h_members, uint64_t *h_sizes,
                           uint64_t *h_per_cluster, uint64_t *h_new_keys, double *h_bic, uint64_t *h_errs,
                           uint64_t *h_stats) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s, BBK_ERR_ARG, "bbk_subclusters_export: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        if (h_errs) memcpy(h_errs, s->errs, sizeof(s->errs));
        if (h_stats) memcpy(h_stats, s->stats, sizeof(s->stats));
        if (s->n == 0) return;
        if (h_good) d2h_big(ctx, h_good, s->good.p, s->n + s->new_kmers);
        if (h_members) d2h_big(ctx, h_members, s->members.p, s->listed * 8);
        if (h_sizes) d2h_big(ctx, h_sizes, s->sizes.p, s->subs * 8);
        if (h_per_cluster) d2h_big(ctx, h_per_cluster, s->per_cluster.p, s->clusters * 8);
        if (h_new_keys && s->new_kmers) d2h_big(ctx, h_new_keys, s->new_keys.p, s->new_kmers * 8);
        if (h_bic) d2h_big(ctx, h_bic, s->bic.p, s->clusters * 8);
    });
}

int bbk_subclusters_write(bbk_ctx *ctx, const bbk_subclusters *s, const bbk_kmerstats *ks, const char *prefix) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s && ks && prefix, BBK_ERR_ARG, "bbk_subclusters_write: NULL argument");
        BBK_REQUIRE(ks->finished && ks->n == s->n && ks->k == s->k, BBK_ERR_ARG,
                    "bbk_subclusters_write: these are not the statistics the subclusters were made from");
        const std::string pre(prefix);
        write_kmstat(ctx, "bbk_subclusters_write", pre + ".kmstat", ks, s->good.as<uint8_t>(), s->new_kmers);
        auto put = [&](const char *ext, const DevBuf &d, uint64_t count) {
            raw_vector<uint64_t> v(count);
            if (count) d2h_big(ctx, v.data(), d.p, count * 8);
            write_u64_file(pre + ext, v.data(), count);
        };
        put(".subclusters", s->members, s->listed);
        put(".subclusters.idx", s->sizes, s->subs);
        put(".newkmers", s->new_keys, s->new_kmers);
    });
}

void bbk_subclusters_free(bbk_subclusters *s) { delete s; }

}  // extern "C"
