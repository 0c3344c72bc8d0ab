"""Sequential restatement of unitig-coverage (pure Python, test infrastructure).

Literal form, read by read as the reference runs it:
  - the graph of a GFA (io/graph/gfa_reader.cpp): segment i is edge 2i on its forward strand and edge 2i+1 on the
    reverse one, a palindromic segment is one self-conjugate edge 2i; links join the end vertex of one edge to the start
    vertex of the next (and, by conjugation, the reverse pair);
  - BasicSequenceMapper::MapSequence with FindKmer / TryThread / ProcessKmer (modules/alignment/sequence_mapper.hpp:288-404)
    over the (k+1)-mers of every edge (k_ = k + 1);
  - EdgeProfileStorage::Fill / Save (projects/unitig_coverage/profile_storage.hpp:71-93, profile_storage.cpp:44-52) over
    reads that went through LongestValid (io/reads/longest_valid_wrapper.hpp:15-52), each followed by its reverse
    complement (io::EasyStream, io/reads/io_helper.cpp:19-32).
Position-local form, the rule the GPU kernel applies (csrc/edgeprof.hip): one pass over the forward read, delta_i from
positions i-1 and i only, added to the segment; twice for a self-conjugate segment."""
from tests.helpers import rc

_NUCL = set("ACGTacgt")


def longest_valid(s):
    """LongestValidCoords: the first longest run of nucleotides (empty when there is none)"""
    best_len, best_pos, pos = 0, None, None
    for i in range(len(s) + 1):
        if i < len(s) and s[i] in _NUCL:
            if pos is None:
                pos = i
        else:
            if pos is not None and i - pos > best_len:
                best_len, best_pos = i - pos, pos
            pos = None
    return "" if best_len == 0 else s[best_pos:best_pos + best_len].upper()


def parse_gfa(text):
    """(names, sequences, links [(a, '+'|'-', b, '+'|'-')] by segment index) of the S and L lines"""
    names, seqs, raw = [], [], []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "S":
            names.append(f[1])
            seqs.append(f[2].upper())
        elif f[0] == "L":
            raw.append((f[1], f[2], f[3], f[4]))
    idx = {n: i for i, n in enumerate(names)}
    return names, seqs, [(idx[a], oa, idx[b], ob) for a, oa, b, ob in raw]


class Graph:
    def __init__(self, k, names, seqs, links):
        self.k, self.names = k, list(names)
        self.seq, self.conj = {}, {}
        for i, q in enumerate(seqs):
            e = 2 * i
            self.seq[e] = q
            if q == rc(q):
                self.conj[e] = e
            else:
                self.seq[e + 1] = rc(q)
                self.conj[e], self.conj[e + 1] = e + 1, e
        # vertices: ('s', e) start of e, ('e', e) end of e; the start of conj(e) is the conjugate of the end of e, so a
        # link x -> y joins end(x) with start(y) and end(conj y) with start(conj x)
        parent = {}

        def find(v):
            parent.setdefault(v, v)
            while parent[v] != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v

        def union(a, b):
            parent[find(a)] = find(b)

        def oriented(i, o):
            e = 2 * i
            return e if o == "+" or self.conj[e] == e else e + 1

        for a, oa, b, ob in links:
            x, y = oriented(a, oa), oriented(b, ob)
            union(("e", x), ("s", y))
            union(("e", self.conj[y]), ("s", self.conj[x]))
        self._out = {}
        for e in self.seq:
            self._out.setdefault(find(("s", e)), []).append(e)
        self._find = find
        # EdgeIndex: every (k+1)-mer of every edge -> (edge, offset)
        self.index = {}
        for e, q in self.seq.items():
            for p in range(len(q) - k):
                self.index[q[p:p + k + 1]] = (e, p)

    def length(self, e):
        return len(self.seq[e]) - self.k

    def outgoing_of_end(self, e):
        """OutgoingEdges(EdgeEnd(e))"""
        return self._out.get(self._find(("e", e)), [])

    @classmethod
    def from_gfa(cls, text, k):
        return cls(k, *parse_gfa(text))


def map_sequence(g, s):
    """BasicSequenceMapper::MapSequence (optimization_on, an empty KmerMapper): [(edge, mapped_range.size())]"""
    k_ = g.k + 1
    passed, ranges = [], []  # ranges: [initial start, initial end, mapped start, mapped end]
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
            for e in g.outgoing_of_end(last):
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
    return [(e, r[3] - r[2]) for e, r in zip(passed, ranges)]


def fill_literal(g, samples):
    """EdgeProfileStorage::Fill: raw[edge][sample] over every read and its reverse complement"""
    raw = {e: [0] * len(samples) for e in g.seq}
    for si, reads in enumerate(samples):
        for r in reads:
            s = longest_valid(r)
            for x in (s, rc(s)):
                for e, size in map_sequence(g, x):
                    raw[e][si] += size
    return raw


def segment_raw(g, raw):
    """[segments][samples]: what Save prints for each S line before the division (the canonical edge 2i)"""
    return [raw[2 * i] for i in range(len(g.names))]


def save(g, raw):
    """EdgeProfileStorage::Save text: name, then raw / length per sample as std::ostream prints a double (%g)"""
    out = []
    for i, name in enumerate(g.names):
        e = 2 * i
        out.append(name + "\t" + "".join("%g\t" % (v / g.length(e)) for v in raw[e]) + "\n")
    return "".join(out)


def loop1(g, e):
    """a one-(k+1)-mer homopolymer edge linked to itself"""
    q = g.seq[e]
    return g.length(e) == 1 and len(set(q)) == 1 and e in g.outgoing_of_end(e)


def fill_position_local(g, samples):
    """the kernel's rule: [segments][samples] from one pass over each forward read"""
    out = [[0] * len(samples) for _ in g.names]
    for si, reads in enumerate(samples):
        for r in reads:
            s = longest_valid(r)
            prev = None
            for p in range(len(s) - g.k):
                hit = g.index.get(s[p:p + g.k + 1])
                if hit is not None:
                    e, off = hit
                    if prev is not None and prev[0] == e and off >= prev[1]:
                        d = off - prev[1] if off > prev[1] else (1 if loop1(g, e) else 0)
                    else:
                        d = 1
                    out[e // 2][si] += d * (2 if g.conj[e] == e else 1)
                prev = hit
    return out
