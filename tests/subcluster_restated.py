"""A literal restatement of BayesHammer's Bayesian subclustering (projects/hammer/kmer_cluster.cpp), the parity target of
csrc/subclust.hip.  Not engine code: plain Python over the arrays the engine exports, function for function:

    tables()            the four probability tables of projects/hammer/main.cpp:103-108 (two are read: lprobs, lrprobs)
    ExpandedKMer        kmer_stat.hpp:205-279 (lprobs_ through getProb / getRevProb, globals.hpp:30-40)
    consensus, consensus_with_mask, cluster_bic, lmeans, subcluster_single, process_cluster   kmer_cluster.cpp:49-577
    process             kmer_cluster.cpp:590-633, the clusters one after the other

Doubles are Python floats (IEEE binary64, one rounding per operation), total_qual is numpy.float32 so that `1 - total_qual`
is the float subtraction the C++ does.  log / pow are libm's (math.log, math.pow), as std::log / std::pow are.

Where this differs from the reference on purpose: an index is a position in the ascending set; the members
of a cluster are ordered by (count descending, index ascending) -- the reference's std::sort is unstable; new k-mers are
numbered n, n + 1, ... in the order (cluster, subcluster) and not deduplicated; clusters are processed in their order, so
where two subclusters mark the same k-mer the later one stands.

Every function notes the branch it takes in `trace` (a set of names), so that a test can assert that a crafted input
went where it was built to go.
"""
import math

import numpy as np

NO_CENTER = -1
DEFAULTS = dict(singleton_threshold=0.995, nonsingleton_threshold=0.9, correct_use_threshold=1, correct_threshold=0.98)
NINF = float("-inf")


def tables():
    """(probs, lprobs, rprobs, lrprobs), 256 entries each: main.cpp:103-108"""
    rprobs = [0.75 if q < 3 else math.pow(10.0, -q / 10.0) for q in range(256)]
    probs = [1 - r for r in rprobs]
    lprobs = [math.log(p) if p > 0 else NINF for p in probs]
    lrprobs = [math.log(r) for r in rprobs]
    return probs, lprobs, rprobs, lrprobs


_T = tables()
LOG3 = math.log(3)
# what the device reads: LP[q] = log(1 - r(q)), LR3[q] = log(r(q)) - log(3), q a 6-bit sum
LP = [_T[1][q] for q in range(64)]
LR3 = [_T[3][q] - LOG3 for q in range(64)]


def bases(key, k):
    """Seq<K>: base i in bits [2i, 2i + 2)"""
    return [(key >> (2 * i)) & 3 for i in range(k)]


def key_of(seq):
    return sum(b << (2 * i) for i, b in enumerate(seq))


def quals_of(words, k):
    """QualBitSet: sum i in bits [6i, 6i + 6) of the little-endian word string (kmer_stat.hpp:80-93)"""
    v = 0
    for j, w in enumerate(words):
        v |= int(w) << (64 * j)
    return [(v >> (6 * i)) & 63 for i in range(k)]


def pack_quals(q):
    """the inverse: ceil(6k / 64) u64 words"""
    v = 0
    for i, x in enumerate(q):
        v |= (int(x) & 63) << (6 * i)
    return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range((6 * len(q) + 63) // 64)]


class ExpandedKMer:
    """kmer_stat.hpp:205-279"""

    def __init__(self, key, k, count, quals):
        self.k = k
        self.s = bases(key, k)
        self.lprobs = [0.0] * (4 * k)
        for i in range(k):
            for j in range(4):
                self.lprobs[4 * i + j] = (_T[3][quals[i]] - LOG3) if j != self.s[i] else _T[1][quals[i]]
        self.count = int(count)

    def logL(self, center):
        res = 0.0
        for i in range(self.k):
            res += self.lprobs[4 * i + center[i]]
        return res

    def hamdist(self, other, tau=None):
        tau = self.k if tau is None else tau
        dist = 0
        for i in range(self.k):
            if self.s[i] != other[i]:
                dist += 1
                if dist > tau:
                    return dist
        return dist


def _argmax_first(v):
    """std::max_element: the first of the largest"""
    b = 0
    for i in range(1, len(v)):
        if v[b] < v[i]:
            b = i
    return b


def _consensus_scores(kmers, take, k):
    scores = [0] * (4 * k)
    for j, km in enumerate(kmers):
        if not take(j):
            continue
        for i in range(k):
            scores[4 * i + km.s[i]] += km.count
    return [_argmax_first(scores[4 * i:4 * i + 4]) for i in range(k)]


def consensus(kmers, k):
    if len(kmers) == 1:
        return list(kmers[0].s)
    return _consensus_scores(kmers, lambda j: True, k)


def consensus_with_mask(kmers, mask, val, k, trace):
    if len(kmers) == 1:  # the size of the block, not the population of the mask
        return list(kmers[0].s)
    if not any(m == val for m in mask):
        trace.add("center_without_members")  # every score is 0: all-A
    return _consensus_scores(kmers, lambda j: mask[j] == val, k)


def host_log(x):
    return math.log(x) if x > 0 else NINF


def cluster_bic(centers, indices, kmers, k, mul_add=None):
    if not indices:
        return NINF
    loglik = 0.0
    total = 0
    for i, km in enumerate(kmers):
        ll = km.logL(centers[indices[i]][0])
        loglik = loglik + km.count * ll if mul_add is None else mul_add(float(km.count), ll, loglik)
        total = (total + km.count) & 0xFFFFFFFF  # `unsigned total`
    clusters = len(centers)
    nparams = (clusters - 1) + clusters * k + 2 * clusters * k
    return loglik - float(nparams) * host_log(float(total)) / 2.0


def lmeans(l, kmers, indices, centers, k, trace, mul_add=None):
    """centers: list of [seq, count], kept from one l to the next; indices likewise"""
    while len(centers) < l:
        centers.append([[0] * k, 0])
    del centers[l:]
    if l == 1:
        centers[0][0] = consensus(kmers, k)
        centers[0][1] = len(kmers)
        for i in range(len(kmers)):
            indices[i] = 0
        return cluster_bic(centers, indices, kmers, k, mul_add)
    total_likelihood = 0.0
    centers[l - 1][0] = list(kmers[l - 1].s)  # bayes_initial_refine
    for i, km in enumerate(kmers):
        cidx = indices[i]
        cdist = km.hamdist(centers[cidx][0], k)
        mdist = km.hamdist(centers[l - 1][0], cdist)
        if mdist < cdist:
            indices[i] = l - 1
            cidx = l - 1
        total_likelihood += km.logL(centers[cidx][0])
    changed = improved = True
    while changed and improved:
        changed = False
        changed_center = [False] * l
        for j in range(l):
            centers[j][1] = 0
        curlik = 0.0
        for i, km in enumerate(kmers):
            loglike = [km.logL(centers[j][0]) for j in range(l)]
            new_ind = _argmax_first(loglike)
            curlik += loglike[new_ind]
            if indices[i] != new_ind:
                changed = True
                changed_center[indices[i]] = True
                changed_center[new_ind] = True
                indices[i] = new_ind
            centers[indices[i]][1] += 1
        improved = curlik > total_likelihood
        if improved:
            total_likelihood = curlik
        for j in range(l):
            if changed_center[j]:
                centers[j][0] = consensus_with_mask(kmers, indices, j, k, trace)
    for j in range(l):
        centers[j][0] = consensus_with_mask(kmers, indices, j, k, trace)
    return cluster_bic(centers, indices, kmers, k, mul_add)


def _f32(x):
    return np.float32(x)


def subcluster_single(block, data, k, p, trace, mul_add=None):
    """block: indices by (count descending, index ascending).  data: dict with keys/count/tq/quals (lists) and `find`
    (key -> index or None).  Returns (lists, new_keys, best_bic); a new k-mer stands in a list as ("new", j)."""
    n0 = len(block)
    cntthr = max(10, int(data["count"][block[0]]) // 10)
    maxcls = sum(1 for i in block if int(data["count"][i]) > cntthr)
    maxgcnt = 0
    for i in block:
        center_quality = _f32(1) - _f32(data["tq"][i])  # float
        if float(center_quality) > p["singleton_threshold"] or \
                (p["correct_use_threshold"] and float(center_quality) > p["correct_threshold"]):
            maxgcnt += 1
    maxcls = min(maxcls, maxgcnt) + 1
    kmers = [ExpandedKMer(data["keys"][i], k, data["count"][i], data["quals"][i]) for i in block]
    best_lik = NINF
    best_centers = []
    indices = [0] * n0
    best_indices = [0] * n0
    centers = []
    stopped = False
    for l in range(1, n0 + 1):
        cur = lmeans(l, kmers, indices, centers, k, trace, mul_add)
        if cur > best_lik:
            if l > maxcls:
                trace.add("improves_past_maxcls")
            best_lik = cur
            best_centers = [[list(c[0]), c[1]] for c in centers]
            best_indices = list(indices)
        elif l >= maxcls:
            trace.add("maxcls_stop")
            stopped = True
            break
    if not stopped:
        trace.add("l_reached_block_size")
    nb = len(best_centers)
    cic = [NO_CENTER] * nb
    for i in range(n0):
        if kmers[i].hamdist(best_centers[best_indices[i]][0]) == 0:
            cic[best_indices[i]] = i
    found_bad = True
    while found_bad:
        found_bad = False
        for kk in range(nb):
            if found_bad:
                break
            if best_centers[kk][1] == 0 or cic[kk] != NO_CENTER:
                continue
            for s in range(nb):
                if s == kk or cic[s] == NO_CENTER:
                    continue
                if best_centers[kk][0] == best_centers[s][0]:
                    trace.add("duplicate_center_merged")
                    for i in range(n0):
                        if indices[i] == kk:  # `indices`, the last l tried
                            indices[i] = s
                            best_centers[s][1] += 1
                    best_centers[kk][1] = 0
                    found_bad = True
                    break
    vec, new_keys = [], []
    for kk in range(nb):
        if best_centers[kk][1] == 0:
            continue
        v = []
        if best_centers[kk][1] == 1:
            trace.add("one_member_subcluster")
            for i in range(n0):
                if indices[i] == kk:  # `indices` again
                    v.append(block[i])
                    break
        else:
            for i in range(n0):
                if best_indices[i] == kk:
                    if cic[kk] == i:
                        v.insert(0, block[i])
                    else:
                        v.append(block[i])
            if cic[kk] == NO_CENTER:
                key = key_of(best_centers[kk][0])
                idx = data["find"](key)
                if idx is None:
                    trace.add("new_kmer")
                    idx = ("new", len(new_keys))
                    new_keys.append(key)
                else:
                    trace.add("consensus_found_in_set")
                v.insert(0, idx)
        if not v:
            trace.add("empty_list_skipped")
        vec.append(v)
    return vec, new_keys, best_lik


def decide_singleton(tq, p):
    """kmer_cluster.cpp:463-491 -> good bit"""
    q = _f32(1) - _f32(tq)
    if float(q) > p["singleton_threshold"]:
        return 1, 1  # (good, counted in gsingl)
    return (1 if p["correct_use_threshold"] and float(q) > p["correct_threshold"] else 0), 0


def decide_center(center_tq, member_tqs, p):
    """kmer_cluster.cpp:508-556 -> (good bit, counted as a good cluster, cluster_quality)"""
    center_quality = float(_f32(1) - _f32(center_tq))  # float subtraction, then widened
    cluster_quality = 1.0
    if member_tqs:
        for t in member_tqs:
            cluster_quality *= float(_f32(t))
        cluster_quality = 1 - cluster_quality
    if center_quality > p["singleton_threshold"] and cluster_quality > p["nonsingleton_threshold"]:
        return 1, 1, cluster_quality
    return (1 if p["correct_use_threshold"] and center_quality > p["correct_threshold"] else 0), 0, cluster_quality


def process(keys, k, count, tq, qual_words, members, sizes, params=None, mul_add=None):
    """KMerClustering::process over the clusters in their order.  Returns a dict shaped like SubClusters.export() plus
    `trace`."""
    p = dict(DEFAULTS)
    p.update(params or {})
    n = len(keys)
    keys = [int(x) for x in keys]
    pos = {x: i for i, x in enumerate(keys)}
    data = dict(keys=keys, count=[int(c) for c in count], tq=[np.float32(t) for t in tq],
                quals=[quals_of(w, k) for w in qual_words], find=pos.get)
    trace = set()
    good = [0] * n
    out_members, out_sizes, per_cluster, new_keys, bic = [], [], [], [], []
    errs = [0] * 16
    st = dict.fromkeys("gsingl tsingl tcsingl gcsingl tcls gcls tkmers tncls newkmers".split(), 0)
    o = 0
    for size in (int(s) for s in sizes):
        cl = [int(m) for m in members[o:o + size]]
        o += size
        if size == 1:
            g, cnt = decide_singleton(data["tq"][cl[0]], p)
            good[cl[0]] = g
            st["gsingl"] += cnt
            st["tsingl"] += 1
            out_members.append(cl[0])
            out_sizes.append(1)
            per_cluster.append(1)
            bic.append(NINF)
            continue
        cl.sort(key=lambda i: (-data["count"][i], i))
        if any(data["count"][a] == data["count"][b] for a, b in zip(cl, cl[1:])):
            trace.add("count_tie")
        vec, nk, best = subcluster_single(cl, data, k, p, trace, mul_add)
        base = n + len(new_keys)
        new_keys += nk
        good += [0] * len(nk)
        data["tq"] += [np.float32(1.0)] * len(nk)  # KMerStat(0, 1.0, NULL)
        data["keys"] += nk
        st["newkmers"] += len(nk)
        st["tncls"] += 1
        bic.append(best)
        nsub = 0
        for v in vec:
            if not v:
                continue
            v = [base + x[1] if isinstance(x, tuple) else x for x in v]
            nsub += 1
            g, cnt, _ = decide_center(data["tq"][v[0]], [data["tq"][x] for x in v[1:]], p)
            good[v[0]] = g
            if len(v) == 1:
                st["tcsingl"] += 1
                st["gcsingl"] += cnt
            else:
                st["tcls"] += 1
                st["gcls"] += cnt
            st["tkmers"] += len(v)
            cb = bases(data["keys"][v[0]], k)
            for x in v[1:]:
                for i, b in enumerate(bases(data["keys"][x], k)):
                    errs[4 * cb[i] + b] += 1
            out_members += v
            out_sizes.append(len(v))
        per_cluster.append(nsub)
    return dict(good=np.array(good, dtype=np.uint8), members=np.array(out_members, dtype=np.uint64),
                sizes=np.array(out_sizes, dtype=np.uint64), per_cluster=np.array(per_cluster, dtype=np.uint64),
                new_keys=np.array(new_keys, dtype=np.uint64), bic=np.array(bic, dtype=np.float64),
                errs=np.array(errs, dtype=np.uint64),
                stats=np.array([st[x] for x in "gsingl tsingl tcsingl gcsingl tcls gcls tkmers tncls newkmers".split()],
                               dtype=np.uint64), trace=trace)


def fused(a, b, c):
    """a * b + c with one rounding: what a contracted `loglik += count * logL` computes on the device"""
    from fractions import Fraction
    if math.isinf(a) or math.isinf(b) or math.isinf(c):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))
