"""Inputs for the subclustering tests (tests/test_subcluster_restated.py on the CPU, tests/test_gpu_subcluster.py on the
GPU): clusters of k-mers with counts, total_qual and quality sums, as plain arrays.  A case is a dict:

    k, keys (ascending ints), count (u32), tq (float32), quals (n x k sums), qual_words (n x ceil(6k / 64) u64),
    members / sizes (the Hamming clusters in the documented order: ascending inside, clusters by smallest member)

Nothing here depends on the engine.  The clusters need not be components of the Hamming graph: the subclustering takes
whatever clusters it is given.
"""
import numpy as np

from tests import subcluster_restated as R


def make_case(k, items, clusters):
    """items: [(key, count, tq, quals)]; clusters: lists of positions in items; items no cluster names become
    singletons"""
    assert len({it[0] for it in items}) == len(items), "k-mers must be distinct"
    order = sorted(range(len(items)), key=lambda i: items[i][0])
    pos = {old: new for new, old in enumerate(order)}
    named = {i for cl in clusters for i in cl}
    cls = [sorted(pos[i] for i in cl) for cl in clusters] + [[pos[i]] for i in range(len(items)) if i not in named]
    cls.sort(key=lambda cl: cl[0])
    its = [items[i] for i in order]
    quals = np.array([it[3] for it in its], dtype=np.uint8).reshape(len(its), k)
    return dict(k=k, keys=[int(it[0]) for it in its], count=np.array([it[1] for it in its], dtype=np.uint32),
                tq=np.array([it[2] for it in its], dtype=np.float32), quals=quals,
                qual_words=np.array([R.pack_quals(q) for q in quals], dtype=np.uint64).reshape(len(its), (6 * k + 63) // 64),
                members=np.array([i for cl in cls for i in cl], dtype=np.uint64),
                sizes=np.array([len(cl) for cl in cls], dtype=np.uint64))


def restate(case, params=None, mul_add=None):
    return R.process(case["keys"], case["k"], case["count"], case["tq"], case["qual_words"], case["members"],
                     case["sizes"], params, mul_add)


def sub(key, pos, delta):
    """the k-mer with base `pos` advanced by delta (1..3)"""
    b = (key >> (2 * pos)) & 3
    return (key & ~(3 << (2 * pos))) | (((b + delta) & 3) << (2 * pos))


def _rand_key(rng, k):
    return int(rng.integers(0, 4, k, dtype=np.uint64).dot(1 << (2 * np.arange(k, dtype=np.uint64)).astype(object)))


def random_cluster(rng, k, size, used, n_centers=None, top=None):
    """`size` distinct k-mers around 1 .. 3 centers one or two substitutions apart; high counts, saturated sums and a tiny
    total_qual for the centers, low counts and poor qualities around them, with ties"""
    n_centers = int(rng.integers(1, 4)) if n_centers is None else n_centers
    n_centers = min(n_centers, size)
    items = []
    base = _rand_key(rng, k)
    centers = []
    while len(centers) < n_centers:
        c = base
        for _ in range(int(rng.integers(0, 3)) if centers else 0):
            c = sub(c, int(rng.integers(0, k)), int(rng.integers(1, 4)))
        if c not in used:
            used.add(c)
            centers.append(c)
    for c in centers:
        cnt = int(rng.integers(15, 200)) if top is None else top
        if rng.random() < 0.25 and top is None:
            cnt = int(rng.integers(1, 12))
        q = np.minimum(63, rng.integers(30, 64, k) + (20 if cnt > 20 else 0))
        items.append((c, cnt, np.float32(10.0 ** -rng.uniform(2, 8)), q))
    while len(items) < size:
        c = centers[int(rng.integers(0, len(centers)))]
        x = sub(c, int(rng.integers(0, k)), int(rng.integers(1, 4)))
        if rng.random() < 0.3:
            x = sub(x, int(rng.integers(0, k)), int(rng.integers(1, 4)))
        if x in used:
            continue
        used.add(x)
        cnt = int(rng.integers(1, 4))
        items.append((x, cnt, np.float32(rng.uniform(0.001, 0.9)), rng.integers(0, 25, k)))
    return items


def random_case(k, seed, n_clusters, max_size):
    rng = np.random.default_rng(seed)
    used, items, clusters = set(), [], []
    for _ in range(n_clusters):
        size = int(rng.integers(1, max_size + 1))
        cl = random_cluster(rng, k, size, used)
        clusters.append(list(range(len(items), len(items) + len(cl))))
        items += cl
    return make_case(k, items, clusters)


def sized_case(k, seed, sizes=(64, 65, 256, 257)):
    """one cluster of each size, one to three members of high count and good quality each (maxcls <= 4)"""
    rng = np.random.default_rng(seed)
    used, items, clusters = set(), [], []
    for j, size in enumerate(sizes):
        cl = random_cluster(rng, k, size, used, n_centers=1 + j % 3, top=100 + j)
        clusters.append(list(range(len(items), len(items) + len(cl))))
        items += cl
    return make_case(k, items, clusters)


def _hi(k):
    return [40] * k


def chain_case(k):
    """c+e1, c+e1+e2, c+e2, c+e2+e3, c+e3 with counts 10, 1, 10, 1, 10: the consensus c is no member and not in the set"""
    rng = np.random.default_rng(7 * k)
    c = _rand_key(rng, k)
    p1, p2, p3 = 1, k // 2, k - 2
    e1, e2, e3 = (lambda x: sub(x, p1, 1)), (lambda x: sub(x, p2, 2)), (lambda x: sub(x, p3, 3))
    ks = [e1(c), e2(e1(c)), e2(c), e3(e2(c)), e3(c)]
    items = [(x, cnt, np.float32(0.3), [2] * k) for x, cnt in zip(ks, (10, 1, 10, 1, 10))]
    return make_case(k, items, [list(range(5))])


def threshold_case(k):
    """singletons and pairs around thresholds that floats hold exactly: singleton 0.75, correct 0.5, nonsingleton 0.875"""
    rng = np.random.default_rng(11 * k)
    params = dict(singleton_threshold=0.75, nonsingleton_threshold=0.875, correct_threshold=0.5, correct_use_threshold=1)
    f = np.float32
    up, down = (lambda x: np.nextafter(f(x), f(2))), (lambda x: np.nextafter(f(x), f(-1)))
    # 1 - tq against 0.75 and 0.5.  For T = 0.25 and 0.5: T puts the float difference at the threshold; T - 2^-24 puts it
    # one float above; the float above T puts it below (or, rounded to even, at it); the float below T (T - 2^-26,
    # T - 2^-25) has a double difference above the threshold and a float difference that rounds to the threshold
    e = f(2.0 ** -24)
    tqs = [f(0.25), f(0.25) - e, up(0.25), down(0.25), f(0.5), f(0.5) - e, up(0.5), down(0.5), f(0.0), f(1.0)]
    used, items, clusters = set(), [], []
    for t in tqs:
        x = _rand_key(rng, k)
        assert x not in used
        used.add(x)
        items.append((x, 5, t, rng.integers(0, 64, k)))
    # pairs: the center's quality good (tq 0.125), the member's total_qual decides 1 - tq against 0.875
    for mt in (f(0.125), down(0.125), up(0.125)):
        for ct in (f(0.125), f(0.25), f(0.4), f(0.5)):
            c = _rand_key(rng, k)
            x = sub(c, int(rng.integers(0, k)), 1)
            assert c not in used and x not in used
            used.update((c, x))
            clusters.append([len(items), len(items) + 1])
            items.append((c, 50, ct, _hi(k)))
            items.append((x, 1, mt, [3] * k))
    return make_case(k, items, clusters), params


def denormal_case(k):
    """subclusters whose cluster_quality is a product with a denormal float total_qual in it"""
    rng = np.random.default_rng(13 * k)
    used, items, clusters = set(), [], []
    for tiny in (np.float32(1e-45), np.float32(7e-42), np.float32(1.1754942e-38)):
        c = _rand_key(rng, k)
        xs = [sub(c, (3 * j + 1) % k, 1 + j % 3) for j in range(4)]
        assert c not in used and not used.intersection(xs)
        used.update([c] + xs)
        clusters.append(list(range(len(items), len(items) + 5)))
        items.append((c, 80, np.float32(1e-4), _hi(k)))
        for j, x in enumerate(xs):
            items.append((x, 1 + j % 2, tiny if j == 1 else np.float32(0.3 + 0.1 * j), [4] * k))
    return make_case(k, items, clusters)


def tie_case(k):
    """equal counts everywhere: the order of the members is decided by the index"""
    rng = np.random.default_rng(17 * k)
    used, items, clusters = set(), [], []
    for cnt in (1, 7, 30):
        c = _rand_key(rng, k)
        xs = [c] + [sub(c, (5 * j + 2) % k, 1 + j % 3) for j in range(5)]
        assert not used.intersection(xs)
        used.update(xs)
        clusters.append(list(range(len(items), len(items) + len(xs))))
        for x in xs:
            items.append((x, cnt, np.float32(rng.uniform(1e-4, 0.5)), rng.integers(10, 50, k)))
    return make_case(k, items, clusters)


def past_maxcls_case(k):
    """two well-separated groups of good quality but counts of at most 10: maxcls is 1 and the BIC still improves at
    l = 2"""
    rng = np.random.default_rng(19 * k)
    a = _rand_key(rng, k)
    b = a
    for p in range(0, k, 2):
        b = sub(b, p, 1 + p % 3)
    items = []
    for c in (a, b):
        items.append((c, 10, np.float32(1e-5), [60] * k))
        for j in range(3):
            items.append((sub(c, 2 * j + 1, 1 + j), 8, np.float32(1e-3), [60] * k))
    return make_case(k, items, [list(range(len(items)))])


def sparse_cluster(k, seed, pad_to=None):
    """one cluster of 4 .. 10 k-mers that differ at two to four positions only, most quality sums 2 (where a match and a
    mismatch weigh the same, so that assignments tie and go to the lower center), counts from a few values.  pad_to: the
    same cluster at a larger k, the added positions the same base everywhere with the sum 2"""
    rng = np.random.default_rng(seed)
    c = _rand_key(rng, k)
    size = int(rng.integers(4, 11))
    ks = set()
    npos = int(rng.integers(2, 5))
    poss = rng.choice(k, npos, replace=False)
    while len(ks) < size:
        x = c
        for p in poss:
            if rng.random() < 0.5:
                x = sub(x, int(p), int(rng.integers(1, 3)))
        ks.add(x)
        if len(ks) >= 3 ** npos - 1:
            break
    items = []
    for x in ks:
        q = rng.choice([2, 2, 2, 40], k)
        items.append((x, int(rng.choice([1, 2, 2, 3, 3, 12, 12, 30])), np.float32(rng.uniform(0, 1)), q))
    if pad_to:
        items = [(x, cnt, t, list(q) + [2] * (pad_to - k)) for x, cnt, t, q in items]
        k = pad_to
    return make_case(k, items, [list(range(len(items)))])


def small_cluster(k, seed):
    """one cluster of 4 .. 7 k-mers one or two substitutions from a k-mer that is mostly a member too"""
    rng = np.random.default_rng(seed)
    c = _rand_key(rng, k)
    size = int(rng.integers(4, 8))
    ks = {c} if rng.random() < 0.8 else set()
    while len(ks) < size:
        x = sub(c, int(rng.integers(0, k)), int(rng.integers(1, 4)))
        if rng.random() < 0.3:
            x = sub(x, int(rng.integers(0, k)), int(rng.integers(1, 4)))
        ks.add(x)
    items = []
    for x in ks:
        q = rng.choice([2, 2, 40, 63], k)
        items.append((x, int(rng.integers(1, 30)), np.float32(rng.uniform(0, 1)), q))
    return make_case(k, items, [list(range(len(items)))])


# Generator arguments whose restatement takes the named branches (found by search, asserted by the CPU test)
SEARCHED = {
    21: dict(center_without_members=(random_case, (0, 40, 12), {"center_without_members"}),
             one_member_subcluster=(random_case, (1, 40, 12), {"one_member_subcluster"}),
             maxcls_stop=(random_case, (2, 40, 12), {"maxcls_stop", "l_reached_block_size"}),
             listed_twice=(small_cluster, (9637,), {"consensus_found_in_set"}),
             duplicate_center=(sparse_cluster, (228426,), {"duplicate_center_merged"})),
    32: dict(center_without_members=(random_case, (0, 40, 12), {"center_without_members"}),
             one_member_subcluster=(random_case, (1, 40, 12), {"one_member_subcluster"}),
             maxcls_stop=(random_case, (2, 40, 12), {"maxcls_stop", "l_reached_block_size"}),
             listed_twice=(small_cluster, (4760,), {"consensus_found_in_set"}),
             empty_list=(small_cluster, (33022,), {"empty_list_skipped"}),
             duplicate_center=(lambda k, seed: sparse_cluster(21, seed, pad_to=k), (228426,), {"duplicate_center_merged"})),
}


def crafted(k):
    """name -> (case, params or None, the branches the case was built for)"""
    tc, tp = threshold_case(k)
    out = {
        "new_kmer": (chain_case(k), None, {"new_kmer"}),
        "count_ties": (tie_case(k), None, {"count_tie"}),
        "threshold_equality": (tc, tp, set()),
        "denormal_total_qual": (denormal_case(k), None, set()),
        "past_maxcls": (past_maxcls_case(k), None, {"improves_past_maxcls"}),
    }
    for name, (gen, args, want) in SEARCHED.get(k, {}).items():
        out[name] = (gen(k, *args), None, set(want))
    return out
