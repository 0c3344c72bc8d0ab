"""Sequential restatement of spades-gmapper for contig libraries (pure Python, test infrastructure).

Literal form, contig by contig as the reference runs it (projects/gmapper/main.cpp:156-247):
  - GFAReader::to_graph (io/graph/gfa_reader.cpp:54-148): segment i is edge 2i and its conjugate 2i+1 (a palindromic
    segment is the one self-conjugate edge 2i); these numbers order as the reference's edge ids.  Per segment a vertex
    pair is created as the end of 2i (vertex 4i, conjugate 4i+1) and, unless self-conjugate, one as the end of 2i+1
    (4i+2, 4i+3): creation order, so they order as the reference's vertex ids.  Links are applied one arc at a time
    with ConstructionHelper::LinkEdges (construction_helper.hpp:95-99), which MOVES the start of e2 onto the end of e1.
    The arcs are the gfa library's (ext/src/gfa1/gfa.c): one per L line, plus the complement w' -> v' of every L line
    whose complement is not in the file (gfa_fix_symm), sorted by source (segment, orientation), file order kept within
    a source.  KC:i: is the raw coverage of both strands.
  - AbstractSequenceMapper::MapRead (modules/alignment/sequence_mapper.hpp:68-98): the contig is cut at every N and each
    piece mapped with BasicSequenceMapper::MapSequence (:288-404), initial ranges shifted by the piece's start.
  - GappedPathExtractor (modules/alignment/long_read_mapper.cpp:201-326): DeleteSameEdges, FilterBadMappings,
    FindReadPathWithGaps with MappingPathFixer::TryCloseGap (sequence_mapper.hpp:204-235), i.e. a bounded Dijkstra
    (dijkstra_algorithm.hpp) and PathProcessor's backward DFS (assembly_graph/paths/path_processor.hpp), first path wins.
  - PathStorage::AddPath / SaveAllPaths (modules/alignment/long_read_storage.hpp:66-265) and GFAPathWriter
    (bidirectional_path_output.hpp:70-107) after GFAWriter::WriteSegmentsAndLinks (io/graph/gfa_writer.cpp).
Position-local form, the rule the GPU kernel applies (csrc/edgeprof.hip: k_gm_paths): each position starts a range or
continues its predecessor's from the two positions alone."""
import heapq
import struct

from tests.helpers import rc
from tests.unitig_profile_restated import parse_gfa

LENGTH_BOUND = 70
MIN_MAPPED_LENGTH, MIN_MAPPED_RATIO = 100, 0.3
MAX_CALL_CNT, MAX_DIJKSTRA_VERTICES = 3000, 3000
VERTEX_USAGE_ENABLE_THRESHOLD, MAX_VERTEX_USAGE = 500, 5
_ACGT = set("ACGT")


def parse_kc(text):
    """KC:i: of every S line (0 without one), as the gfa library reads an int32 tag"""
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "S":
            v = 0
            for t in f[3:]:
                if t.startswith("KC:i:"):
                    v = int(t[5:]) & 0xFFFFFFFF
                    break
            out.append(v)
    return out


def gfa_arcs(links):
    """[(v, w)] over oriented segments x = 2 * segment + (x is '-'), in the order to_graph links them"""
    arcs = [((a << 1) | (oa == "-"), (b << 1) | (ob == "-")) for a, oa, b, ob in links]
    order = sorted(range(len(arcs)), key=lambda j: arcs[j][0])
    by_src = {}
    for j in order:
        by_src.setdefault(arcs[j][0], []).append(j)
    comp = [False] * len(arcs)
    extra = []
    for j in order:  # gfa_fix_symm
        if comp[j]:
            continue
        v, w = arcs[j]
        for i in by_src.get(w ^ 1, []):
            if not comp[i] and arcs[i][1] == v ^ 1:
                comp[i] = True
                break
        else:
            extra.append((w ^ 1, v ^ 1))
    return sorted(arcs + extra, key=lambda a: a[0])


def fmt_float(x):
    """std::ostream << float(x)"""
    return "%g" % struct.unpack("f", struct.pack("f", x))[0]


def gr(a, b):
    """math::gr: a > b and more than 4 ULPs apart (common/math/xmath.h)"""
    def biased(x):
        u = struct.unpack("<Q", struct.pack("<d", x))[0]
        return ((~u + 1) & ((1 << 64) - 1)) if u >> 63 else u | (1 << 63)
    return abs(biased(a) - biased(b)) > 4 and a > b


class Graph:
    def __init__(self, k, names, seqs, links, kc=None):
        self.k, self.names, self.links = k, list(names), list(links)
        self.kc = list(kc) if kc is not None else [0] * len(seqs)
        self.seq, self.conj = {}, {}
        for i, q in enumerate(seqs):
            e = 2 * i
            self.seq[e] = q
            if q == rc(q):
                self.conj[e] = e
            else:
                self.seq[e + 1] = rc(q)
                self.conj[e], self.conj[e + 1] = e + 1, e
        self.end = {}
        for i in range(len(seqs)):
            self.end[2 * i] = 4 * i  # LinkIncomingEdge: e ends at v, conj(e) leaves conj(v) = v ^ 1
            if self.conj[2 * i] != 2 * i:
                self.end[2 * i + 1] = 4 * i + 2
        for v, w in gfa_arcs(links):
            self.link_edges(self.oriented(v), self.oriented(w))
        # OutgoingEdges(v): the edges that start at v, sorted by id (AddOutgoingEdge, graph_core.hpp:193)
        self.out = {}
        for e in sorted(self.seq):
            self.out.setdefault(self.start(e), []).append(e)
        self.index = {}
        for e, q in self.seq.items():
            for p in range(len(q) - k):
                self.index[q[p:p + k + 1]] = (e, p)

    def oriented(self, x):
        e = 2 * (x >> 1)
        return e if self.conj[e] == e else e + (x & 1)

    def start(self, e):
        return self.end[self.conj[e]] ^ 1

    def link_edges(self, e1, e2):
        """LinkEdges: e2 (and with it the end of conj(e2)) moves to the end of e1"""
        self.end[self.conj[e2]] = self.end[e1] ^ 1

    def length(self, e):
        return len(self.seq[e]) - self.k

    def coverage(self, e):
        return self.kc[e // 2] / self.length(e)

    def outgoing(self, v):
        return self.out.get(v, [])

    def incoming(self, v):
        """IncomingEdges(v): the conjugates of OutgoingEdges(conj v), in that order"""
        return [self.conj[e] for e in self.outgoing(v ^ 1)]

    def canonical(self, e):
        return min(e, self.conj[e])

    def orient(self, e, delim=""):
        """CanonicalEdgeHelper::EdgeOrientationString with the segment names (MapNamingF)"""
        return self.names[self.canonical(e) // 2] + delim + ("+" if e == self.canonical(e) else "-")

    def loop1(self, e):
        """TryThread re-enters a one-(k+1)-mer edge at its own end: e is among OutgoingEdges(EdgeEnd(e))"""
        return self.length(e) == 1 and e in self.outgoing(self.end[e])

    def index_loop1(self, e):
        """the index's kEpLoop1: a one-(k+1)-mer homopolymer segment with an L line from itself to itself"""
        s = e // 2
        return (self.length(e) == 1 and len(set(self.seq[e])) == 1 and
                any(a == b == s and oa == ob for a, oa, b, ob in self.links))

    @classmethod
    def from_gfa(cls, text, k):
        names, seqs, links = parse_gfa(text)
        return cls(k, names, seqs, links, parse_kc(text))


def map_sequence(g, s):
    """BasicSequenceMapper::MapSequence: [(edge, [initial start, initial end, mapped start, mapped end])]"""
    k_ = g.k + 1
    passed, ranges = [], []
    if len(s) < k_:
        return []

    def find_kmer(kmer, pos):
        hit = g.index.get(kmer)
        if hit is None:
            return False
        e, off = hit
        if not passed or passed[-1] != e or pos != ranges[-1][1] or off + 1 < ranges[-1][3]:
            passed.append(e)
            ranges.append([pos, pos + 1, off, off + 1])
        else:
            ranges[-1][1] = pos + 1
            ranges[-1][3] = off + 1
        return True

    def try_thread(kmer, pos):
        last = passed[-1]
        end = ranges[-1][3]
        if end < g.length(last):
            if g.seq[last][end + k_ - 1] == kmer[k_ - 1]:
                ranges[-1][1] += 1
                ranges[-1][3] += 1
                return True
        else:
            for e in g.outgoing(g.end[last]):
                if g.seq[e][k_ - 1] == kmer[k_ - 1]:
                    passed.append(e)
                    ranges.append([pos, pos + 1, 0, 1])
                    return True
        return False

    def process_kmer(kmer, pos, tt):
        if tt:
            if not try_thread(kmer, pos):
                find_kmer(kmer, pos)
                return False
            return True
        return find_kmer(kmer, pos)

    tt = process_kmer(s[:k_], 0, False)
    for i in range(k_, len(s)):
        tt = process_kmer(s[i - k_ + 1:i + 1], i - k_ + 1, tt)
    return list(zip(passed, ranges))


def map_sequence_local(g, s):
    """the kernel's rule: a found position starts a range unless its predecessor is found on the same oriented edge at an
    offset below it, or at the same offset of an edge without the index's loop flag"""
    out, prev = [], None
    for p in range(len(s) - g.k):
        hit = g.index.get(s[p:p + g.k + 1])
        if hit is not None:
            e, off = hit
            if prev is not None and prev[0] == e and (off > prev[1] or (off == prev[1] and not g.index_loop1(e))):
                out[-1][1][1], out[-1][1][3] = p + 1, off + 1
            else:
                out.append((e, [p, p + 1, off, off + 1]))
        prev = hit
    return out


def pieces(contig):
    """MapRead's cut at every N: [(start, piece)]; a character other than ACGTN is refused (the reference aborts)"""
    s = contig.upper()
    bad = set(s) - _ACGT - {"N"}
    if bad:
        raise ValueError("character %r is not a nucleotide" % sorted(bad)[0])
    out, start = [], 0
    for i, c in enumerate(s + "N"):
        if c == "N":
            if i > start:
                out.append((start, s[start:i]))
            start = i + 1
    return out


def map_read(g, contig, mapper=None):
    """MapRead: the mapping paths of the pieces joined, initial ranges shifted by the piece's start"""
    mapper = mapper or map_sequence
    out = []
    for st, piece in pieces(contig):
        for e, r in mapper(g, piece):
            out.append((e, [r[0] + st, r[1] + st, r[2], r[3]]))
    return out


def dijkstra(g, v1, bound=LENGTH_BOUND, vertex_limit=MAX_DIJKSTRA_VERTICES):
    """DijkstraHelper::CreateBoundedDijkstra(g, bound, vertex_limit).Run(v1): vertex -> distance (DistanceCounted)"""
    dist, heap, n = {}, [(0, v1, -1, -1)], 0
    while heap:
        d, v, _, _ = heapq.heappop(heap)
        if v in dist:
            continue
        dist[v] = d
        n += 1
        if n > vertex_limit or not (n < vertex_limit and d <= bound):
            continue
        for e in g.outgoing(v):
            w = g.end[e]
            if w not in dist and d + g.length(e) <= bound:
                heapq.heappush(heap, (d + g.length(e), w, v, e))
    return dist


def close_gap(g, v1, v2, bound=LENGTH_BOUND):
    """MappingPathFixer::TryCloseGap: the first path ProcessPaths(g, 0, bound, v1, v2) finds, or []"""
    if v1 == v2:
        return []
    dist = dijkstra(g, v1, bound)
    if v2 not in dist or dist[v2] > bound:
        return []
    found, rev, cnt = [], [], {v2: 1}
    st = {"len": 0, "calls": 0}

    def go(v):
        st["calls"] += 1
        if st["calls"] >= MAX_CALL_CNT:
            return True
        if v == v1:
            found.append(rev[::-1])
        inc = [e for e in g.incoming(v) if g.start(e) in dist]
        inc.sort(key=lambda e: (dist[g.start(e)], -g.coverage(e)))  # stable, as libstdc++'s insertion sort of <= 16
        for e in inc:
            s = g.start(e)
            if dist[s] + g.length(e) + st["len"] > bound:
                continue
            if st["calls"] >= VERTEX_USAGE_ENABLE_THRESHOLD and cnt.get(s, 0) >= MAX_VERTEX_USAGE:
                continue
            st["len"] += g.length(e)
            rev.append(e)
            cnt[s] = cnt.get(s, 0) + 1
            stop = go(s)
            cnt[s] -= 1
            rev.pop()
            st["len"] -= g.length(e)
            if stop:
                return True
        return False

    go(v2)
    return found[0] if found else []


def extract_paths(g, mp):
    """GappedPathExtractor: the edge paths of one read's mapping path"""
    if not mp:
        return []
    corrected = []
    for e, _ in mp:  # DeleteSameEdges
        if not corrected or corrected[-1] != e:
            corrected.append(e)
    filtered, i = [], 0
    for e in corrected:  # FilterBadMappings over CountMappedEdgeSize
        while mp[i][0] != e:
            i += 1
        j = i
        while j < len(mp) and mp[j][0] == e:
            j += 1
        size = sum(r[1] - r[0] for _, r in mp[i:j])
        i = j
        if size > MIN_MAPPED_LENGTH or gr(size / g.length(e), MIN_MAPPED_RATIO):
            filtered.append(e)
    if not filtered:
        return []
    paths, cur = [], [filtered[0]]
    for prev, nxt in zip(filtered, filtered[1:]):  # FindReadPathWithGaps
        left, right = g.end[prev], g.start(nxt)
        if left != right:
            closure = close_gap(g, left, right)
            if closure:
                cur += closure
            else:
                paths.append(cur)
                cur = []
        cur.append(nxt)
    paths.append(cur)
    return paths


class PathStorage:
    def __init__(self):
        self.index = {}

    def add_path(self, p, w=1):
        if p:
            d = self.index.setdefault(p[0], {})
            d[tuple(p)] = d.get(tuple(p), 0) + w

    def save_all_paths(self):
        return [(list(p), self.index[f][p]) for f in sorted(self.index) for p in sorted(self.index[f])]


def write_gfa(g, paths):
    """GFAPathWriter: WriteSegmentsAndLinks, then one P line per contiguous stretch of every path"""
    out = []
    for i, name in enumerate(g.names):
        e = 2 * i
        out.append("S\t%s\t%s\tDP:f:%s\tKC:i:%d\n" % (name, g.seq[e], fmt_float(g.coverage(e)), g.kc[i]))
    verts = set(g.end.values())
    for v in sorted(verts | {x ^ 1 for x in verts}):
        if v & 1:
            continue
        for a in g.incoming(v):
            for b in g.outgoing(v):
                out.append("L\t%s\t%s\t%dM\n" % (g.orient(a, "\t"), g.orient(b, "\t"), g.k))
    for idx, (p, w) in enumerate(paths, 1):
        name = "PATH_%d_length_%d_weigth_%d" % (idx, len(p), w)
        seg, cur = 1, []
        for a, b in zip(p, p[1:]):
            cur.append(g.orient(a))
            if g.end[a] != g.start(b):
                out.append("P\t%s_%d\t%s\t*\tZ:W:%d\n" % (name, seg, ",".join(cur), w))
                seg, cur = seg + 1, []
        cur.append(g.orient(p[-1]))
        out.append("P\t%s_%d\t%s\t*\tZ:W:%d\n" % (name, seg, ",".join(cur), w))
    return "".join(out)


def gmapper(g, contigs, mapper=None):
    """the output file of one contig library (untrusted-contigs / path-extend-contigs)"""
    st = PathStorage()
    for c in contigs:
        for p in extract_paths(g, map_read(g, c, mapper)):
            st.add_path(p)
    return write_gfa(g, st.save_all_paths())
