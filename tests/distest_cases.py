"""Inputs of the distance-estimation tests (pure Python): crafted graphs with true k-overlaps, so that the engine's GFA
reader accepts what the restatement reads, the hand-derived cases, and the shapes that sit on the edges of the device path
(group sizes, capacities, the order-free boundary, the Dijkstra's vertex limit)."""
import random

from tests import distest_restated as D
from tests import gmapper_restated as G
from tests.helpers import rc

K = 21
# the device's capacities (csrc/distest.hip: kDeBallCap, kDeUCap), stated here and not read from the engine
BALL_CAP, U_CAP = 512, 2047


class Builder:
    """vertices are random k-mers, an edge u -> v of `length` (k+1)-mers is kmer(u) + bases + kmer(v); a vertex is an id,
    ~id its conjugate.  length >= k + 2, so every junction is a k-overlap by construction and the base after kmer(u) and
    the base before kmer(v) are free: they are made to differ among the edges that share the vertex, as in a de Bruijn
    graph (the edge index wants every (k+1)-mer once), which allows four edges out of a vertex and four into it.  The L
    lines link every edge that ends at a vertex to every edge that starts there."""

    def __init__(self, k=K, seed=1):
        self.k, self.rng = k, random.Random(seed)
        self.kmers, self.segs, self.used = [], [], {}

    def _rand(self, n):
        return "".join(self.rng.choice("ACGT") for _ in range(n))

    def vertex(self):
        self.kmers.append(self._rand(self.k))
        return len(self.kmers) - 1

    def kmer(self, v):
        return rc(self.kmers[~v]) if v < 0 else self.kmers[v]

    def free(self, v):
        """edges that may still start at v (an edge that ends at ~v counts: its conjugate starts at v)"""
        return 4 - len(self.used.get(v, ""))

    def _take(self, v):
        """a base no edge out of v follows kmer(v) with yet"""
        left = [c for c in "ACGT" if c not in self.used.get(v, "")]
        assert left, "a vertex has four edges out and four in at most"
        self.used[v] = self.used.get(v, "") + left[0]
        return left[0]

    def edge(self, u, v, length, kc=None):
        """the segment's number; its forward edge is 2 * number"""
        assert length >= self.k + 2
        first, last = self._take(u), rc(self._take(~v))
        self.segs.append((u, v, self.kmer(u) + first + self._rand(length - self.k - 2) + last + self.kmer(v),
                          kc if kc is not None else length * (3 + len(self.segs) % 5)))
        return len(self.segs) - 1

    def palindrome(self, u, length):
        """a self-conjugate segment from u to ~u (length - k even)"""
        assert length >= self.k + 2 and (length - self.k) % 2 == 0
        x = self._take(u) + self._rand((length - self.k) // 2 - 1)
        seq = self.kmer(u) + x + rc(x) + rc(self.kmer(u))
        assert seq == rc(seq)
        self.segs.append((u, ~u, seq, 4 * length))
        return len(self.segs) - 1

    def gfa(self):
        out = ["S\t%d\t%s\tKC:i:%d\n" % (3 + 2 * i, q, kc) for i, (_, _, q, kc) in enumerate(self.segs)]
        ends, starts = {}, {}  # vertex -> oriented segments
        for i, (u, v, q, _) in enumerate(self.segs):
            starts.setdefault(u, []).append((i, "+"))
            ends.setdefault(v, []).append((i, "+"))
            if q != rc(q):
                starts.setdefault(~v, []).append((i, "-"))
                ends.setdefault(~u, []).append((i, "-"))
        seen = set()
        for v in sorted(ends):
            for a, oa in ends[v]:
                for b, ob in starts.get(v, []):
                    if (a, oa, b, ob) not in seen:
                        seen.add((a, oa, b, ob))
                        out.append("L\t%d\t%s\t%d\t%s\t%dM\n" % (3 + 2 * a, oa, 3 + 2 * b, ob, self.k))
        return "".join(out)

    def graph(self):
        return G.Graph.from_gfa(self.gfa(), self.k)


# insert_size 400, read length 100, deviation 40: U = 400 + 40 - 21 - 2 = 417, gap 200,
# min_len = max(0, 200 + 23 - l1 - l2 - 40) = max(0, 183 - l1 - l2)
def params(linkage=0, max_distance=80, threshold=2.0, insert_size=400, delta=40):
    return D.Params(insert_size, 100, delta, linkage, max_distance, threshold)


def single_path():
    """A(100) -> M(50) -> B(100)"""
    b = Builder(seed=11)
    v = [b.vertex() for _ in range(4)]
    A, M, B = b.edge(v[0], v[1], 100), b.edge(v[1], v[2], 50), b.edge(v[2], v[3], 100)
    return b, (2 * A, 2 * M, 2 * B)


def bubble():
    """A(100) -> {M1(30), M2(60), M3(230)} -> B(100): the distances 130, 160 and 330"""
    b = Builder(seed=12)
    v = [b.vertex() for _ in range(4)]
    A = b.edge(v[0], v[1], 100)
    arms = [b.edge(v[1], v[2], n) for n in (30, 60, 230)]
    B = b.edge(v[2], v[3], 100)
    return b, (2 * A, [2 * x for x in arms], 2 * B)


def cycle_between():
    """A(100) -> v, C(40): v -> v, v -> B(100)"""
    b = Builder(seed=13)
    v = [b.vertex() for _ in range(3)]
    A, C, B = b.edge(v[0], v[1], 100), b.edge(v[1], v[1], 40), b.edge(v[1], v[2], 100)
    return b, (2 * A, 2 * C, 2 * B)


def cycle_through():
    """A(100): u -> v, R(70): v -> u"""
    b = Builder(seed=14)
    u, v = b.vertex(), b.vertex()
    A, R = b.edge(u, v, 100), b.edge(v, u, 70)
    return b, (2 * A, 2 * R)


def no_path():
    """A(100) and B(100) in two components"""
    b = Builder(seed=15)
    v = [b.vertex() for _ in range(4)]
    A, B = b.edge(v[0], v[1], 100), b.edge(v[2], v[3], 100)
    return b, (2 * A, 2 * B)


def hairpin():
    """A(100): w -> u, P(41) palindromic: u -> ~u, so A -> P -> conj A; and Q(60): u -> x next to it"""
    b = Builder(seed=16)
    w, u, x = b.vertex(), b.vertex(), b.vertex()
    A, Pl, Q = b.edge(w, u, 100), b.palindrome(u, 41), b.edge(u, x, 60)
    return b, (2 * A, 2 * Pl, 2 * Q)


def tree(n_edges, edge_len=23, seed=17):
    """A(100) into the root of a 4-ary tree of n_edges edges of edge_len, filled level by level: with U >= 5 * edge_len
    the ball of A holds the root and one vertex per edge (n_edges <= 1364), and every tree edge is a second edge of A at
    the distance 100 + edge_len * its depth.  (A, [tree edges], [their depths])"""
    b = Builder(seed=seed)
    root = b.vertex()
    A = b.edge(b.vertex(), root, 100)
    level, edges, depths, depth = [root], [], [], 0
    while len(edges) < n_edges:
        nxt = []
        for v in level:
            for _ in range(4):
                if len(edges) < n_edges:
                    w = b.vertex()
                    edges.append(2 * b.edge(v, w, edge_len))
                    depths.append(depth)
                    nxt.append(w)
        level, depth = nxt, depth + 1
    return b, (2 * A, edges, depths)


def paths(n):
    """n single paths A_i(100) -> M_i(30) -> B_i(100): n first edges with one second edge each"""
    b = Builder(seed=18 + n)
    firsts, seconds = [], []
    for _ in range(n):
        v = [b.vertex() for _ in range(4)]
        firsts.append(2 * b.edge(v[0], v[1], 100))
        b.edge(v[1], v[2], 30)
        seconds.append(2 * b.edge(v[2], v[3], 100))
    return b, (firsts, seconds)


def random_graph(seed, n_vertices=24, n_edges=60):
    """a junction-rich multigraph with cycles, conjugate links and a few palindromes, edges of 23 .. 70"""
    b = Builder(seed=seed)
    rng = random.Random(seed)
    vs = [b.vertex() for _ in range(n_vertices)]
    for i in range(n_edges):
        while True:  # a vertex takes four edges a side
            u, v = rng.choice(vs), rng.choice(vs)
            if i % 7 == 3:
                v = ~v
            if b.free(u) if i % 11 == 5 else b.free(u) and b.free(~v) and (u != ~v or b.free(u) > 1):
                break
        if i % 11 == 5:
            b.palindrome(u, 23 + 2 * rng.randint(0, 20))
        else:
            b.edge(u, v, rng.randint(23, 70))
    return b


def random_points(g, seed, n_pairs=120):
    """points of random edge pairs, gaps around the insert geometry, as bbk_pairinfo_import leaves them"""
    rng = random.Random(seed)
    edges = sorted(g.seq)
    pts = []
    for _ in range(n_pairs):
        e1, e2 = rng.choice(edges), rng.choice(edges)
        for _ in range(rng.randint(1, 5)):
            pts.append((e1, e2, rng.randint(-60, 330), rng.randint(1, 6)))
    return D.canonical_points(g, pts)


def pair_points(pairs, distance, seed=3):
    """a few points per (e1, e2) around the graph distance between them; every e1 is 100 long"""
    rng = random.Random(seed)
    return [(e1, e2, d - 100 + rng.randint(-9, 9), rng.randint(1, 4))
            for (e1, e2), d in zip(pairs, distance) for _ in range(rng.randint(1, 3))]


def bubble_chain(n_bubbles, lead, tail):
    """A(100) -> `lead` edges of 23 -> n bubbles of arms (23, 24), each followed by an edge of 23 -> `tail` edges of 23
    -> B(100).  The backward search calls Go once per walk: once at every vertex of the tail, 2^j times at each of the
    two inner vertices of the j-th bubble from the end, 2^n times at every vertex of the lead"""
    b = Builder(seed=40 + n_bubbles)
    v = b.vertex()
    A = b.edge(b.vertex(), v, 100)
    for _ in range(lead):
        w = b.vertex()
        b.edge(v, w, 23)
        v = w
    for _ in range(n_bubbles):
        w, x = b.vertex(), b.vertex()
        b.edge(v, w, 23, kc=23 * 7)
        b.edge(v, w, 24, kc=24 * 7)  # equal coverage: the tie rule decides the order
        b.edge(w, x, 23)
        v = x
    for _ in range(tail):
        w = b.vertex()
        b.edge(v, w, 23)
        v = w
    B = b.edge(v, b.vertex(), 100)
    return b, (2 * A, 2 * B)


# the chain on either side of the order-free boundary: 5 bubbles and 12 lead edges, 499 calls with 21 tail edges and 500
# with 22 (tests/test_distest_restated.py holds both against the restatement's count)
BOUNDARY = {499: (5, 12, 21), 500: (5, 12, 22)}


def boundary_params():
    """U = 1200 + 40 - 23 = 1217 covers the longest walk of either chain, 5 * 47 + 34 * 23 + 5 = 1022"""
    return params(insert_size=1200)


def one_mer_chain(n):
    """n one-(k+1)-mer edges in a row between A(100) and B(100)"""
    b = Builder(seed=50)
    s = b._rand(n + K + 2 * (100 + K))
    segs = [s[:100 + K]] + [s[100 + i:100 + i + K + 1] for i in range(n)] + [s[100 + n:100 + n + 100 + K]]
    gfa = "".join("S\t%d\t%s\tKC:i:%d\n" % (3 + 2 * i, q, 5 * (len(q) - K)) for i, q in enumerate(segs))
    gfa += "".join("L\t%d\t+\t%d\t+\t%dM\n" % (3 + 2 * i, 5 + 2 * i, K) for i in range(len(segs) - 1))
    return gfa, (0, 2 * (len(segs) - 1))
