"""What the emulated and the GPU tests of `from_msa --unaligned --progressive --device-tree` share: mprg_prog_tree called directly
through the C ABI on hand-built tables (with nw = 65 536 for every leaf, s = 65 536 - D reaches any D in 0 .. 65 536), against the
spec's plain-Python statements (prog_ref.upgma, collapse_ref.upgma; up to 20 leaves) and the host's tree (star_align.prog_tree,
which the existing tests pin to them); whole MSAs with the flag on against the flag-off run and the references; what moves between
host and device.  Every reference is computed once per process."""
import functools
import hashlib

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import collapse_common as cc
from tests import collapse_ref as cr
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import star_trace as tr

POISON = 0x5C
GUARD = 64                                 # poisoned bytes in front of and behind the merges
NW = 1 << 16
BLANK = int(np.full(4, POISON, np.uint8).view(np.int32)[0])
EDGE_M = (63, 64, 65, 255, 256, 257, 511, 512, 513, 520)      # the wavefront, the workgroup's 256 threads, TR_LDS_M = 512 records
WEIGHTED_EDGE_M = (65, 257, 513)


def nested(merges):
    """A merge list as prog_ref.upgma's nested pairs."""
    tree = {}
    for u, v in merges:
        tree[u] = (tree.get(u, u), tree.pop(v, v))
    assert len(tree) == 1
    return next(iter(tree.values()))


class Locus:
    """m records of which `leaf` are non-empty, D between them (symmetric int64; only the leaves' entries mean anything), w: how
    many times each record counts (read for the leaves only)."""

    def __init__(self, D, leaf, w):
        self.D, self.leaf, self.w = np.asarray(D, np.int64), np.asarray(leaf, bool), np.asarray(w, np.int64)
        self.m, self.leaves = len(self.leaf), np.nonzero(self.leaf)[0].tolist()

    def plain(self, weighted):
        """The plain statement's tree, as nested pairs (O(m^4): small loci only)."""
        if weighted:
            return cr.upgma(self.D.tolist(), self.leaves, self.w.tolist())
        return pr.upgma(self.D.tolist(), self.leaves)

    def host(self, weighted):
        return sa.prog_tree(self.D, self.leaves, self.w[self.leaves] if weighted else None)


def random_locus(rng, n_leaves, top, empties=(), w_top=9):
    """n_leaves leaves with D drawn from 0 .. top (top None: all 65 536) and weights from 1 .. w_top; empties: the records (by
    index in the finished locus) that are empty."""
    m = n_leaves + len(empties)
    leaf = np.ones(m, bool)
    leaf[list(empties)] = False
    D = np.full((m, m), NW, np.int64) if top is None else rng.integers(0, top + 1, (m, m))
    D = np.triu(D, 1)
    D = D + D.T
    w = rng.integers(1, w_top + 1, m)
    w[~leaf] = 0
    return Locus(D, leaf, w)


@functools.lru_cache(maxsize=None)
def small_loci():
    """2 to 20 leaves, D from {0 .. 3}, {0 .. 65 536} and all equal, empty records in front, between and behind; then the two hand
    cases of test_tree_ties_resolve_by_key."""
    rng = np.random.default_rng(5)
    out = []
    for n in (2, 3, 4, 5, 9, 14, 20):
        for top in (3, NW, None):
            m = n + 3 + n // 5
            mid = rng.choice(np.arange(2, m - 1), 1 + n // 5, replace=False).tolist()
            out.append(random_locus(rng, n, top, [0] + mid + [m - 1]))
    for seqs in (["ACGTAC", "TTTTTT", "ACGTAC", "TTTTTT"], ["ACG", "ACGT", "AC", "ACGTA"]):
        out.append(Locus(pr.distances(seqs)[0], [True] * 4, [1] * 4))
    return out


@functools.lru_cache(maxsize=None)
def small_spec(weighted):
    return [l.plain(weighted) for l in small_loci()]


@functools.lru_cache(maxsize=None)
def edge_loci():
    """Per m of EDGE_M a locus of tie-heavy D (small integers) and one of spread D; two empty records each."""
    rng = np.random.default_rng(6)
    return [random_locus(rng, m - 2, top, [1, m - 2], w_top=7) for m in EDGE_M for top in (max(3, m // 4), NW)]


@functools.lru_cache(maxsize=None)
def edge_spec(weighted):
    return [l.host(weighted) if not weighted or l.m in WEIGHTED_EDGE_M else None for l in edge_loci()]


# ---- the call
def tables(loci, weighted):
    """mprg_prog_tree's host-side tables for these loci: what is not a leaf pair's s, a leaf's nw or a leaf's weight is garbage.
    (ws_alloc: the words the workspace buffer really has, whatever a refusal case then states as ws_words.)"""
    m = np.array([l.m for l in loci], np.int64)
    first, toff = sa.exclusive_sum(m), sa.exclusive_sum(m * m)
    n_merges = np.array([max(len(l.leaves) - 1, 0) for l in loci], np.int64)
    words = sa.prog_tree_words(m)
    shared = np.full(int((m * m).sum()), 0xFFFFFFFF, np.uint32)
    for l, o in zip(loci, toff.tolist()):
        t = shared[o:o + l.m * l.m].reshape(l.m, l.m)
        pair = np.triu(np.outer(l.leaf, l.leaf), 1)
        t[pair] = (NW - l.D)[pair]
    leaf = np.concatenate([l.leaf for l in loci])
    return dict(shared=shared, nw=np.where(leaf, NW, -7).astype(np.int64), seqs=np.stack([np.zeros(len(leaf), np.int64), leaf * 9], 1),
                loci=np.stack([first, m, toff, sa.exclusive_sum(words), 2 * sa.exclusive_sum(n_merges)], 1).astype(np.int64),
                weights=np.concatenate([l.w for l in loci]).astype(np.int32) if weighted else None, n_merges=n_merges,
                shared_words=len(shared), ws_words=int(words.sum()), ws_alloc=int(words.sum()), merges_words=2 * int(n_merges.sum()))


def call(be, t):
    """(status words, per locus its merges as written: BLANK where nothing was); the guard bytes around the merges are checked."""
    d_shared, d_nw, d_seqs, d_loci = be.upload(t["shared"]), be.upload(t["nw"]), be.upload(t["seqs"]), be.upload(t["loci"])
    d_weights = None if t["weights"] is None else be.upload(t["weights"])
    n_loci, n_words = len(t["loci"]), 2 * int(t["n_merges"].sum())
    d_ws, d_merges, d_status = be.empty(8 * t["ws_alloc"]), be.full(4 * n_words + 2 * GUARD, POISON), be.full(4 * n_loci, POISON)
    be.call("mprg_prog_tree", be.ptr(d_shared), t["shared_words"], be.ptr(d_nw), be.ptr(d_seqs), len(t["nw"]), be.ptr(d_loci), n_loci,
            0 if d_weights is None else be.ptr(d_weights), be.ptr(d_ws), t["ws_words"], be.ptr(d_merges) + GUARD, t["merges_words"],
            be.ptr(d_status), be.stream)
    raw = be.download(d_merges, np.uint8, 4 * n_words + 2 * GUARD)
    assert (raw[:GUARD] == POISON).all() and (raw[GUARD + 4 * n_words:] == POISON).all()
    flat = raw[GUARD:GUARD + 4 * n_words].view(np.int32)
    off = 2 * sa.exclusive_sum(t["n_merges"])
    got = [[tuple(p) for p in flat[o:o + 2 * n].reshape(-1, 2).tolist()] for o, n in zip(off.tolist(), t["n_merges"].tolist())]
    return be.download(d_status, np.int32, n_loci).tolist(), got


def trees(be, loci, weighted):
    status, got = call(be, tables(loci, weighted))
    assert status == [0] * len(loci)
    return got


# ---- 1. small trees against the plain statement
def check_small(be):
    loci = small_loci()
    assert {len(l.leaves) for l in loci} == {2, 3, 4, 5, 9, 14, 20} and all(not l.leaf[0] and not l.leaf[-1] and not l.leaf[1:-1].all() for l in loci[:-2])
    for weighted in (False, True):
        got = trees(be, loci, weighted)
        for l, g, want in zip(loci, got, small_spec(weighted)):
            assert nested(g) == want, (l.m, weighted)
            assert g == l.host(weighted), (l.m, weighted)     # ... and merge by merge what the host's tree lists
    assert nested(got[-2]) == ((0, 2), (1, 3)) and nested(got[-1]) == (((0, 1), 2), 3)
    one = Locus(np.zeros((3, 3), np.int64), [False, True, False], [0, 1, 0])                 # L < 2: nothing written
    assert call(be, tables([one, loci[3], Locus(np.zeros((2, 2), np.int64), [False, False], [0, 0])], False)) == ([0, 0, 0], [[], loci[3].host(False), []])


# ---- 2. the edges of the kernel's own structure against prog_tree
def check_edges(be, weighted=False):
    loci, spec = edge_loci(), edge_spec(weighted)
    pick = [k for k, s in enumerate(spec) if s is not None]
    assert {loci[k].m for k in pick} == set(WEIGHTED_EDGE_M if weighted else EDGE_M)
    got = trees(be, [loci[k] for k in pick], weighted)                  # loci of different m in one launch
    for k, g in zip(pick, got):
        assert g == spec[k], (loci[k].m, weighted)
    return pick, got


def check_edges_in_groups(be):
    """The same loci, one launch per group of a small budget: the same merges."""
    loci, spec = edge_loci(), edge_spec(False)
    need = sa.prog_tree_bytes(np.array([l.m for l in loci], np.int64))
    groups = list(pa.budget_groups(need, int(need.max()) + int(need[2])))
    assert 5 < len(groups) < len(loci) and any(hi - lo > 1 for lo, hi in groups)
    for lo, hi in groups:
        assert trees(be, loci[lo:hi], False) == spec[lo:hi], (lo, hi)


def check_prog_trees(be):
    """star_align.prog_trees (distances and trees, both on the device) on sequences: the host's tree from prog_shared's tables,
    with the default budget, with a budget that forces groups, and weighted."""
    loci = pc.msa_loci()
    codes = [sa.locus_codes(str(k), pc.records(l)) for k, l in enumerate(loci)]
    rng = np.random.default_rng(9)
    weights = [rng.integers(1, 6, len(c)) for c in codes]
    want = {True: [], False: []}
    for cs, (shared, nw), w in zip(codes, sa.prog_shared(be, codes), weights):
        lv = [a for a, c in enumerate(cs) if len(c)]
        for weighted in (False, True):
            want[weighted].append(sa.prog_tree(sa.prog_distance_matrix(shared, nw), lv, w[lv] if weighted else None) if len(lv) > 1 else [])
    assert max(len(t) for t in want[False]) >= 17 and any(a != b for a, b in zip(want[False], want[True]))
    assert sa.prog_trees(be, codes) == want[False]
    assert sa.prog_trees(be, codes, budget_bytes=sa.prog_tree_bytes(20)) == want[False]
    assert sa.prog_trees(be, codes, weights) == want[True]


# ---- 3. exactness beyond float64
def _represent(rng, c, p, mean):
    """D[0 .. 3] in 0 .. 65 536 with sum c[i] D[i] = p exactly (D[0], D[1] drawn around `mean`, D[2], D[3] solved), or None."""
    g = int(np.gcd(c[2], c[3]))
    c2, c3 = c[2] // g, c[3] // g
    for _ in range(4000):
        d0, d1 = (int(x) for x in rng.integers(mean - 8000, mean + 8000, 2))
        rest = p - c[0] * d0 - c[1] * d1
        if rest < 0 or rest % g:
            continue
        r = rest // g
        d2 = r * pow(c2, -1, c3) % c3 if c3 > 1 else 0
        while d2 <= NW:
            d3, rem = divmod(r - c2 * d2, c3)
            if rem == 0 and 0 <= d3 <= NW:
                return [d0, d1, d2, d3]
            d2 += c3
    return None


@functools.lru_cache(maxsize=None)
def exact_loci():
    """Eight leaves of weights 300 .. 512 (sum <= 4 096): leaves 2 q, 2 q + 1 merge first (D = 1 .. 4), which leaves the clusters A, B,
    C, E of keys 0, 2, 4, 6.  The sums p1 between A and B and p2 between C and E are solved for, with q1 = |A| |B| and q2 = |C| |E|, so
    that p1 q2 - p2 q1 = gcd(q1, q2): the smallest difference there is, in cross products above 2^53.  Kept when p1 / q1 and p2 / q2
    are the same float64: the spec merges (4, 6), the smaller average, where a comparison of rounded quotients keeps the first pair
    in key order, (0, 2).  Every other D is 65 000 or more."""
    out = []
    rng = np.random.default_rng(1)
    while len(out) < 3:
        w = [int(x) for x in rng.integers(300, 513, 8)]
        if sum(w) > sa.PROG_MAX_LEAVES:
            continue
        q1, q2 = (w[0] + w[1]) * (w[2] + w[3]), (w[4] + w[5]) * (w[6] + w[7])
        g = int(np.gcd(q1, q2))
        a1, a2 = q1 // g, q2 // g
        if a1 == 1:
            continue
        mean = int(rng.integers(38000, 48000))
        p1 = pow(a2, -1, a1)                                             # p1 a2 = 1 (mod a1)
        p1 += (mean * q1 - p1) // a1 * a1
        p2 = (p1 * a2 - 1) // a1
        assert p1 * q2 - p2 * q1 == g
        if p1 / q1 != p2 / q2 or p2 * q1 <= 1 << 53:
            continue
        dab = _represent(rng, [w[a] * w[b] for a in (0, 1) for b in (2, 3)], p1, mean)
        dce = _represent(rng, [w[a] * w[b] for a in (4, 5) for b in (6, 7)], p2, mean)
        if dab is None or dce is None:
            continue
        D = rng.integers(65000, NW + 1, (8, 8))
        for q in range(4):
            D[2 * q, 2 * q + 1] = q + 1
        D[0, 2], D[0, 3], D[1, 2], D[1, 3] = dab
        D[4, 6], D[4, 7], D[5, 6], D[5, 7] = dce
        D = np.triu(D, 1)
        assert p1 == sum(w[a] * w[b] * int(D[a, b]) for a in (0, 1) for b in (2, 3))
        assert p2 == sum(w[a] * w[b] * int(D[a, b]) for a in (4, 5) for b in (6, 7))
        out.append(Locus(D + D.T, [True] * 8, w))
    return out


def check_exact(be):
    loci = exact_loci()
    got = trees(be, loci, True)
    for l, g in zip(loci, got):
        assert nested(g) == l.plain(True) and g[:5] == [(0, 1), (2, 3), (4, 5), (6, 7), (4, 6)], l.w
        assert g == l.host(True)


# ---- 4. the limit and the refusals
def check_refusals(be):
    rng = np.random.default_rng(8)
    a, c = random_locus(rng, 5, 3, [2]), random_locus(rng, 6, NW, [0, 3])
    b = random_locus(rng, 4, 100, [1])
    b.w[b.leaf] = [1024, 1024, 1024, 1025]                                   # a weight sum of 4 097
    loci = [a, b, c]
    blank = [(BLANK, BLANK)] * 3
    want_a, want_c = a.host(True), c.host(True)
    assert call(be, tables(loci, True)) == ([0, 1, 0], [want_a, blank, want_c])
    b.w[b.leaf] = [1024, 1024, 1024, 1024]                                   # ... and 4 096 is built
    want_b = b.host(True)
    assert nested(want_b) == b.plain(True)
    assert call(be, tables(loci, True)) == ([0, 0, 0], [want_a, want_b, want_c])

    def tripped(code, **change):
        t = tables(loci, True)
        for key, value in change.items():
            if key in ("toff", "woff", "moff", "first", "m"):
                t["loci"][1, ("first", "m", "toff", "woff", "moff").index(key)] = value(t) if callable(value) else value
            else:
                t[key] = value(t) if callable(value) else value
        assert call(be, t) == ([0, code, 0], [want_a, blank, want_c]), change
    tripped(1, toff=lambda t: t["shared_words"] - b.m * b.m + 1)             # the table ends one word outside shared_words
    tripped(1, toff=-1)
    tripped(1, moff=lambda t: t["merges_words"] - 6 + 1)                     # the merges end one element outside merges_words
    tripped(1, moff=-2)
    tripped(1, first=lambda t: len(t["nw"]) - b.m + 1)                       # the sequences end outside n_seqs
    tripped(1, m=0)
    tripped(3, woff=lambda t: t["ws_words"] - sa.prog_tree_words(b.m) + 1)   # the workspace one word short
    tripped(3, woff=-1)
    leaf = int(sum(l.m for l in loci[:1])) + b.leaves[2]
    for low in (0, -3):
        def weights(t, low=low):
            t["weights"][leaf] = low
            return t["weights"]
        tripped(1, weights=weights)                                          # a leaf's weight below 1
    # the last locus's table one word outside: the others are built
    t = tables(loci, True)
    t["shared_words"] -= 1
    assert call(be, t) == ([0, 0, 1], [want_a, want_b, [(BLANK, BLANK)] * 5])
    t = tables(loci, True)
    t["ws_words"] -= 1
    assert call(be, t) == ([0, 0, 3], [want_a, want_b, [(BLANK, BLANK)] * 5])


# ---- 5. whole MSAs
def fasta(msas):
    return [sa.msa_fasta(m) for m in msas]


def check_msas(be, **kw):
    """prog_common.check_msas with the flag on (prog_ref's rows and progression), and the flag-off run byte for byte."""
    pc.check_msas(be, device_tree=True, **kw)
    recs = [pc.records(l) for l in pc.msa_loci()]
    timings, on_info, off_info = {}, [], []
    on = sa.star_msas(be, recs, progressive=True, device_tree=True, timings=timings, progression=on_info, **kw)
    off = sa.star_msas(be, recs, progressive=True, progression=off_info, **kw)
    assert fasta(on) == fasta(off) and on_info == off_info
    assert timings["tree_device_loci"] == sum(1 for n, _, _ in on_info if n >= 3) > 20 and 0 < timings["tree_plan_s"] < timings["tree_s"]


def check_compositions(be):
    """adjust_direction, band and refine with the flag on: the reference compositions of prog_common and the flag-off bytes."""
    recs = [pc.records(l) for l in pc.flipped_loci()]
    spec = pc.flipped_spec()
    msas = sa.star_msas(be, recs, progressive=True, adjust_direction=True, device_tree=True)
    assert [(m.descriptions, m.rows_as_strings()) for m in msas] == [(t, rows) for t, rows, _ in spec]
    for band in (False, True):
        info = []
        msas = sa.star_msas(be, recs, progressive=True, adjust_direction=True, refine=2, refinement=info, band=band, device_tree=True)
        for m, got, (t, _, (rows, acc, trail)) in zip(msas, info, spec):
            assert m.descriptions == t and m.rows_as_strings() == rows and got == (acc, trail[0], trail[-1])
        assert fasta(msas) == fasta(sa.star_msas(be, recs, progressive=True, adjust_direction=True, refine=2, band=band))


def check_collapse(be):
    """collapse_common's loci with collapse: collapse_ref's rows (and the band and refine runs of its check) with the weighted tree
    from the device, and the flag-off bytes."""
    cc.check_progressive(be, device_tree=True)
    recs = [pc.records(l) for l in cc.loci()]
    on_info, off_info, timings = [], [], {}
    on = sa.star_msas(be, recs, progressive=True, collapse=True, device_tree=True, progression=on_info, timings=timings)
    assert fasta(on) == fasta(sa.star_msas(be, recs, progressive=True, collapse=True, progression=off_info)) and on_info == off_info
    assert timings["tree_device_loci"] == sum(1 for n, _, _ in on_info if n >= 3) >= 4


# ---- 6. what moves between host and device
def check_trace(be):
    """With the flag on: one mprg_prog_tree call per mprg_prog_distances call, right behind it, and no uint32 table comes back;
    the MSAs are the golden run's.  With it off: the golden digest."""
    for name in ("progressive", "everything_small_budget"):
        wrapped = tr.TraceBackend(be)
        msas = sa.star_msas(wrapped, tr.loci(), **dict(tr.scenarios()[name], device_tree=True))
        calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
        at = [k for k, c in enumerate(calls) if c == "mprg_prog_distances"]
        assert len(at) >= (1 if name == "progressive" else 2) and calls.count("mprg_prog_tree") == len(at)
        assert all(calls[k + 1] == "mprg_prog_tree" for k in at)
        assert not any(line.startswith("download uint32") for line in wrapped.lines)
        assert hashlib.md5("".join(fasta(msas)).encode()).hexdigest() == tr.golden()[name]["msa_md5"]
    assert tr.run(be, "progressive")[1] == tr.golden()["progressive"]
