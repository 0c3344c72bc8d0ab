"""Sequential restatement of DistanceEstimation for a paired-end library (pure Python, test infrastructure): the chain
of estimate_distance (projects/spades/distance_estimation.cpp:137-154) up to and including the weight filter, over
gmapper_restated.Graph and the raw points of pairinfo_restated (ascending (e1, e2, gap, weight)).
  - estimate_distance: the library parameters (library_params).
  - DistanceEstimator::ProcessEdge (common/paired_info/distance_estimation.cpp:152-174): per first edge the stored second
    edges of GetHalf, i.e. the canonical pairs, which are the only ones the raw index of f17 stores.
  - GraphDistanceFinder::FillGraphDistancesLengths (:17-45) with the bounds of pair_info_bounds.hpp:16-27: one bounded
    Dijkstra (gmapper_restated.dijkstra) from EdgeEnd(e1), then per second edge PathProcessor::Traversal
    (assembly_graph/paths/path_processor.hpp:56-181) from EdgeStart(e2) with DistancesLengthsCallback (:380-402).
    `traversal` is the literal search.  `walk_lengths` is the order-free form: the walk-count recurrence
        B[t][0] = 1 at t = EdgeStart(e2);  B[v][l] = sum over edges v -> w of B[w][l - len(e)],  kept while dist(v) + l <= U
    whose sum is the number of calls Go makes when no limit fires, and whose support at EdgeEnd(e1) from min_len on is
    the length set.  No limit can fire below 500 calls (VERTEX_USAGE_ENABLE_THRESHOLD; MAX_CALL_CNT is 3000) when the
    Dijkstra stayed below its vertex limit, so there the two agree whatever the order of the incoming edges.
    Declared deviation: where the order matters, ties in (distance, coverage) go by this engine's edge numbers
    (g.incoming order, stable sort), since the reference's edge ids are not reproducible here.
  - DistanceEstimator::EstimateEdgePairDistances (:97-150), AbstractDistanceEstimator::ClusterResult (:51-67).
  - AddToResult / PairedIndex::Merge (paired_info_buffer.hpp:63-68, 103-133; paired_info.hpp:282-299): a pair that is its
    own conjugate (e1 == conj e2) has its clusters inserted twice into the thread's buffer and that buffer's histogram
    merged twice into the result: four times the weight.  The thread's buffer is a PairedInfoBuffer, whose points are raw
    (RawPointTraits, paired_info.hpp:711-712): AddMany slices the half-span that ClusterResult computed off every cluster
    and Merge restores it as 0 (index_point.hpp:228-229), so every cluster of the result has half-span 0
    (tests/golden/graph_ref/ records it so; the earlier reading kept ClusterResult's value).
  - PairInfoFilter with PairInfoWeightChecker (pair_info_filters.hpp:42-56, 241-261): a point stays iff
    math::ge(weight, threshold).
  - PairedBuffer::BinWrite of the clustered index (paired_info_buffer.hpp:197-210): PointT (index_point.hpp:218-259) does
    not override RawPointT::BinWrite (:195-197), which writes sizeof(RawPointT) = 8 bytes: the float gap = d - length(e1)
    (PointTraits::Shrink, :296-299) and the float weight; the variance is not written.
Weights are kept in integer half-units (an exact tie gives half a weight to each side); the reference sums floats, which
is the same number while a sum stays below 2^23.  Distances are integers, exact as floats below 2^21, where math::eq's
4 ULPs are less than 1."""
import math
import struct

from tests import gmapper_restated as G
from tests import pairinfo_restated as P

MAX_CALL_CNT, MAX_DIJKSTRA_VERTICES = G.MAX_CALL_CNT, G.MAX_DIJKSTRA_VERTICES
VERTEX_USAGE_ENABLE_THRESHOLD, MAX_VERTEX_USAGE = G.VERTEX_USAGE_ENABLE_THRESHOLD, G.MAX_VERTEX_USAGE


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def ge(a, b):
    """math::ge on doubles: not (a < b and more than 4 ULPs apart)"""
    return not G.gr(b, a)


class Params:
    def __init__(self, insert_size, read_length, delta, linkage_distance=0, max_distance=0, filter_threshold=2.0):
        self.insert_size, self.read_length, self.delta = insert_size, read_length, delta
        self.linkage_distance, self.max_distance, self.filter_threshold = linkage_distance, max_distance, filter_threshold

    @property
    def gap(self):
        return self.insert_size - 2 * self.read_length  # int(insert_size - 2 * read_length)


def library_params(mean, deviation, read_length, linkage_distance_coeff=0.0, max_distance_coeff=2.0, threshold=2.0):
    """estimate_distance: math::round is floor(t + 0.5 + 1e-10) (math/xmath.h:324-330)"""
    return Params(int(math.floor(mean + 0.5 + 1e-10)), read_length, int(deviation), int(linkage_distance_coeff * deviation),
                  int(max_distance_coeff * deviation), threshold)


def upper_bound(k, insert_size, delta):
    """PairInfoPathLengthUpperBound; None where the reference's VERIFY fails"""
    answer = insert_size + delta - k - 2
    return answer if answer > 0 else None


def lower_bound(k, l1, l2, gap, delta):
    return max(0, gap + k + 2 - l1 - l2 - delta)


def _sorted_incoming(g, dist, v):
    inc = [e for e in g.incoming(v) if g.start(e) in dist]
    inc.sort(key=lambda e: (dist[g.start(e)], -g.coverage(e)))  # stable: the declared tie rule
    return inc


def traversal(g, dist, start_v, end_v, min_len, max_len):
    """Traversal(...).Go() with DistancesLengthsCallback: (ascending distinct lengths, calls made)"""
    if end_v not in dist or dist[end_v] > max_len:
        return [], 0
    found, cnt = set(), {end_v: 1}
    st = {"len": 0, "calls": 0}

    def enter(v):
        """the head of Go(v): None when the call limit is reached, else the incoming edges to try"""
        st["calls"] += 1
        if st["calls"] >= MAX_CALL_CNT:
            return None
        if v == start_v and st["len"] >= min_len:
            found.add(st["len"])
        return iter(_sorted_incoming(g, dist, v))

    it = enter(end_v)
    stack = [(end_v, it, 0)] if it is not None else []
    while stack:
        v, it, came = stack[-1]
        for e in it:
            s = g.start(e)
            if dist[s] + g.length(e) + st["len"] > max_len:
                continue
            if st["calls"] >= VERTEX_USAGE_ENABLE_THRESHOLD and cnt.get(s, 0) >= MAX_VERTEX_USAGE:
                continue
            st["len"] += g.length(e)
            cnt[s] = cnt.get(s, 0) + 1
            it2 = enter(s)
            if it2 is None:  # the limit unwinds every frame
                return sorted(found), st["calls"]
            stack.append((s, it2, g.length(e)))
            break
        else:
            stack.pop()
            if stack:
                cnt[v] -= 1
                st["len"] -= came
    return sorted(found), st["calls"]


def walk_lengths(g, dist, start_v, end_v, min_len, max_len, cap=VERTEX_USAGE_ENABLE_THRESHOLD):
    """the recurrence of the header by increasing l: (lengths, sum of B); the sum stops counting at `cap`, where the
    lengths are None: the search is no longer order-free there"""
    if end_v not in dist or dist[end_v] > max_len:
        return [], 0
    B = {0: {end_v: 1}}
    calls, found = 0, []
    for l in range(max_len + 1):
        for v, c in sorted(B.pop(l, {}).items()):
            calls += c
            if calls >= cap:
                return None, calls
            if v == start_v and l >= min_len:
                found.append(l)
            for e in g.incoming(v):
                s = g.start(e)
                if s in dist and dist[s] + g.length(e) + l <= max_len:
                    row = B.setdefault(l + g.length(e), {})
                    row[s] = row.get(s, 0) + c
    return found, calls


def estimate_edge_pair(g, e1, e2, hist, raw_forward, max_distance):
    """EstimateEdgePairDistances: hist = [(d, weight in half-units)] ascending; [(length, weight in half-units)]"""
    first_len, second_len = g.length(e1), g.length(e2)
    min_d, max_d = hist[0][0], hist[-1][0]
    forward = [x for x in raw_forward if min_d - max_distance <= x <= max_d + max_distance]
    if not forward:
        return []
    cur, weights = 0, [0] * len(forward)
    for d, w in hist:
        if 2 * d + second_len < first_len:
            continue
        while cur + 1 < len(forward) and forward[cur + 1] < d:
            cur += 1
        if cur + 1 < len(forward) and forward[cur + 1] - d < d - forward[cur]:
            cur += 1
            if abs(forward[cur] - d) <= max_distance:
                weights[cur] += w
        elif cur + 1 < len(forward) and forward[cur + 1] - d == d - forward[cur]:
            assert w % 2 == 0
            if abs(forward[cur] - d) <= max_distance:
                weights[cur] += w // 2
            cur += 1
            if abs(forward[cur] - d) <= max_distance:
                weights[cur] += w // 2
        elif abs(forward[cur] - d) <= max_distance:
            weights[cur] += w
    return list(zip(forward, weights))


def cluster_result(estimated, linkage_distance):
    """ClusterResult: [(centre float, weight in half-units, half-span float)]"""
    out, i = [], 0
    while i < len(estimated):
        left, weight = i, estimated[i][1]
        while i + 1 < len(estimated) and estimated[i + 1][0] - estimated[i][0] <= linkage_distance:
            i += 1
            weight += estimated[i][1]
        out.append((f32((estimated[left][0] + estimated[i][0]) * 0.5), weight,
                    f32((estimated[i][0] - estimated[left][0]) * 0.5)))
        i += 1
    return out


class Clustering:
    """the clustered index of one library: records [(e1, e2, centre, half-span = 0, weight in half-units)] ascending, and
    per pair what its search met: calls[(e1, e2)] (the literal search's, or the recurrence's sum) and ball[e1]"""

    def __init__(self, g, points, p, lengths="search", keep_unfiltered=False):
        self.g, self.p = g, p
        self.U = upper_bound(g.k, p.insert_size, p.delta)
        if self.U is None:
            raise ValueError("insert_size + delta - k - 2 <= 0")
        self.records, self.calls, self.ball, self.lengths = [], {}, {}, {}
        by_pair = {}
        for e1, e2, gap, w in points:
            by_pair.setdefault(e1, {}).setdefault(e2, []).append((gap, w))
        for e1 in sorted(by_pair):
            dist = G.dijkstra(g, g.end[e1], self.U, MAX_DIJKSTRA_VERTICES)
            self.ball[e1] = len(dist)
            for e2 in sorted(by_pair[e1]):
                min_len = lower_bound(g.k, g.length(e1), g.length(e2), p.gap, p.delta)
                f = traversal if lengths == "search" else walk_lengths
                found, calls = f(g, dist, g.end[e1], g.start(e2), min_len, self.U)
                self.calls[(e1, e2)] = calls
                if found is None:
                    continue
                raw = sorted([x + g.length(e1) for x in found] + ([0] if e1 == e2 else []))
                self.lengths[(e1, e2)] = raw
                hist = [(gap + g.length(e1), 2 * w) for gap, w in sorted(by_pair[e1][e2])]
                est = estimate_edge_pair(g, e1, e2, hist, raw, p.max_distance)
                times = 4 if e1 == g.conj[e2] else 1
                for centre, weight, _ in cluster_result(est, p.linkage_distance):
                    if keep_unfiltered or ge(weight * times / 2.0, p.filter_threshold):
                        self.records.append((e1, e2, centre, f32(0.0), weight * times))  # AddToResult drops the half-span

    def order_free(self, e1, e2):
        return self.calls[(e1, e2)] < VERTEX_USAGE_ENABLE_THRESHOLD and self.ball[e1] < MAX_DIJKSTRA_VERTICES - 1

    def hard_pairs(self, ball_cap, u_cap):
        """the pairs a device with these capacities leaves to the host"""
        return sorted(pr for pr in self.calls
                      if not self.order_free(*pr) or self.ball[pr[0]] > ball_cap or self.U > u_cap)

    def file_bytes(self):
        """<prefix>.<i>.clustered.prd: BinWrite with ids edge + 1, points (float gap, float weight)"""
        return P.prd_bytes([(e1, e2, f32(c - f32(self.g.length(e1))), f32(w / 2.0)) for e1, e2, c, _, w in self.records])


def canonical_points(g, points):
    """what bbk_pairinfo_import leaves of host points: every pair under the smaller of itself and its conjugate (the gap is
    the same under both), ascending, equal (e1, e2, gap) summed.  Weights are stored weights: nothing is doubled"""
    store = {}
    for e1, e2, gap, w in points:
        key = min((e1, e2), (g.conj[e2], g.conj[e1])) + (gap,)
        store[key] = store.get(key, 0) + w
    return [key + (w,) for key, w in sorted(store.items())]
