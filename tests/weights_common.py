"""The checks of `from_msa --unaligned --progressive --seq-weights` (make_prg_amd/from_msa/star_align.py "Sequence weights",
csrc/k_prog_weights.inc), for any backend: tests/test_weights_emulated.py runs them on the CPU emulation build,
tests/test_gpu_weights.py on the MI355X.  mprg_prog_leaf_weights called directly against tests/weights_ref.py's plain statement on
hand-written tables (the shapes around a wavefront and a workgroup, empty records, poisoned tables, guard words), its refusals,
whole MSAs against the statement, the compositions with the other flags, and what moves between host and device."""
import functools
import random
from types import SimpleNamespace
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import collapse_common as cc
from tests import large_common as lc
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import star_ref as sr
from tests import star_trace as tr
from tests import strand_ref as st
from tests import weights_ref as wr

SCALE = sa.PROG_SCALE
TOP = 1 << 20                                  # PROG_MAX_RECORDS: the largest multiplicity sum
POISON8, POISON32, POISON64, BLANK, BLANK64 = 0x5C, 0xEEEEEEEE, -7, 0x5C5C5C5C, 0x5C5C5C5C5C5C5C5C
GUARD = 64                                     # guard bytes in front of and behind heights, raw, q and the workspace
CHANGED = [2, 3, 6, 8, 10, 12, 14, 15]         # the loci of prog_ref.table_loci() whose bytes the weights change (the issue's list)


# ---- 1. the kernel against the plain statement
class Locus(NamedTuple):
    """A locus of the kernel's tables: m records of which `leaf` (ascending) are leaves; s (m x m, the part above the diagonal
    between leaves is read), nw (m); mult per record, or None; the merges."""
    m: int
    leaf: List[int]
    s: np.ndarray
    nw: np.ndarray
    mult: Optional[np.ndarray]
    merges: List[Tuple[int, int]]

    def D(self) -> np.ndarray:
        s = np.triu(self.s, 1)
        s = s + s.T
        mn = np.minimum(self.nw[:, None], self.nw[None, :])
        D = np.where(mn > 0, SCALE - (SCALE * s) // np.maximum(mn, 1), SCALE).astype(np.int64)
        np.fill_diagonal(D, 0)
        return D


def random_merges(rng, leaf):
    """A valid merge list over the leaves that is nobody's UPGMA: two live keys picked at random."""
    live, out = list(leaf), []
    while len(live) > 1:
        u, v = sorted(rng.sample(live, 2))
        out.append((u, v))
        live.remove(v)
    return out


def make_locus(rng, L, spare=0, mult=None, merges="upgma", spread=1.0) -> Locus:
    """L leaves among m = L + spare records (the others empty, at random places), in a few families so that the tree has long and
    short edges; nw between 20 and 400, s up to the smaller nw.  merges: "upgma" (star_align.prog_tree's on D), "random", or a
    list."""
    m = L + spare
    leaf = sorted(rng.sample(range(m), L))
    nw = np.array([rng.randint(20, 400) for _ in range(m)], np.int64)
    fam = np.array([rng.randrange(1 + L // 5) for _ in range(m)])
    close = np.array([[rng.random() * (0.95 if fam[a] == fam[b] else 0.3 * spread) for b in range(m)] for a in range(m)])
    s = np.triu((close * np.minimum(nw[:, None], nw[None, :])).astype(np.int64), 1)
    w = None if mult is None else np.array([rng.randint(1, mult) for _ in range(m)], np.int64)
    l = Locus(m, leaf, s, nw, w, [])
    if merges == "upgma":
        merges = sa.prog_tree(l.D(), leaf, None if w is None else w[leaf]) if L >= 2 else []
    elif merges == "random":
        merges = random_merges(rng, leaf)
    return l._replace(merges=[(int(u), int(v)) for u, v in merges])


def expected(l: Locus):
    """(heights, raw per record, q per record) by the plain statement."""
    D = l.D()
    h, raw, q = wr.leaf_weights(D.tolist(), l.leaf, l.merges, None if l.mult is None else l.mult.tolist())
    raw_r, q_r = np.zeros(l.m, np.int64), np.zeros(l.m, np.int64)
    for a in l.leaf:
        raw_r[a], q_r[a] = raw[a], q[a]
    return np.array(h, np.int64), raw_r, q_r


def expected_np(l: Locus):
    """expected() with the sums in NumPy, for a locus too large for the plain loops (checked against them on the small ones)."""
    D = l.D()
    w = np.ones(l.m, np.int64) if l.mult is None else l.mult
    WD = D * np.outer(w, w)
    members, size, node, par, lpar, h = {a: [a] for a in l.leaf}, {a: int(w[a]) for a in l.leaf}, {}, {}, {}, []
    below = []
    for t, (u, v) in enumerate(l.merges):
        h.append(int(WD[np.ix_(members[u], members[v])].sum()) // (size[u] * size[v]))
        for key in (u, v):
            if key in node:
                par[node[key]] = t
            else:
                lpar[key] = t
        members[u] += members.pop(v)
        size[u] += size.pop(v)
        node[u] = t
        below.append(size[u])
    raw = np.zeros(l.m, np.int64)
    for a in l.leaf:
        c, lo, n, t = 0, 0, int(w[a]), lpar.get(a)
        while t is not None:
            c += (wr.UNIT * max(h[t] - lo, 0) * int(w[a])) // n
            lo, n, t = h[t], below[t], par.get(t)
        raw[a] = c
    top = int(raw.max()) if len(l.leaf) else 0
    q = np.zeros(l.m, np.int64)
    q[l.leaf] = 1 if top == 0 else 1 + ((wr.UNIT - 1) * raw[l.leaf]) // top
    return np.array(h, np.int64), raw, q


class Launch:
    """The tables of one mprg_prog_leaf_weights launch over loci.  `shared` is poisoned wherever the kernel must not read: the
    diagonal, the part below it, the rows and columns of records that are no leaves, three words between two tables and two in
    front of the first; nw and the multiplicities of records that are no leaves are poison too (a negative number: read, it would
    refuse the locus); a spare record stands in front of the first locus and behind the last."""

    def __init__(self, loci: List[Locus], weighted: Optional[bool] = None):
        self.loci = loci
        n = len(loci)
        weighted = any(l.mult is not None for l in loci) if weighted is None else weighted
        m = np.array([l.m for l in loci], np.int64)
        self.first = 1 + sa.exclusive_sum(m)
        self.n_seqs = int(m.sum()) + 2
        self.toff = 2 + sa.exclusive_sum(m * m + 3)
        self.shared_words = int((m * m + 3).sum()) + 2
        self.n_merges = np.array([len(l.merges) for l in loci], np.int64)
        self.moff = 2 * sa.exclusive_sum(self.n_merges)
        self.merges_words = 2 * int(self.n_merges.sum())
        self.ws_words = sa.prog_weights_words(m)
        self.woff = sa.exclusive_sum(self.ws_words)
        self.ws_total = int(self.ws_words.sum())
        self.shared = np.full(self.shared_words, POISON32, np.uint32)
        self.nw = np.full(self.n_seqs, POISON64, np.int64)
        self.seqs = np.zeros((self.n_seqs, 2), np.int64)
        self.weights = np.full(self.n_seqs, -5, np.int32) if weighted else None
        self.merges = np.zeros(max(self.merges_words, 1), np.int32)
        for k, l in enumerate(loci):
            f, t = int(self.first[k]), int(self.toff[k])
            tab = np.full((l.m, l.m), POISON32, np.uint32)
            idx = np.array(l.leaf, np.int64)
            iu = np.triu_indices(len(idx), 1)
            tab[idx[iu[0]], idx[iu[1]]] = l.s[idx[iu[0]], idx[iu[1]]]
            self.shared[t:t + l.m * l.m] = tab.reshape(-1)
            self.nw[f + np.array(l.leaf, np.int64)] = l.nw[l.leaf]
            self.seqs[f + np.array(l.leaf, np.int64), 1] = 5
            if weighted:
                self.weights[f + np.array(l.leaf, np.int64)] = 1 if l.mult is None else l.mult[l.leaf]
            self.merges[self.moff[k]:self.moff[k] + 2 * len(l.merges)] = np.array(l.merges, np.int32).reshape(-1)
        self.table = np.stack([self.first, m, self.toff, self.woff, self.moff], 1).astype(np.int64)

    def expected(self, want, skip=()):
        """(heights, raw, q) as the launch leaves buffers that were BLANK, BLANK64, BLANK: want[k] per locus, `skip` not written."""
        heights = np.full(self.merges_words // 2, BLANK, np.int32)
        raw, q = np.full(self.n_seqs, BLANK64, np.int64), np.full(self.n_seqs, BLANK, np.int32)
        for k, l in enumerate(self.loci):
            if k in skip:
                continue
            f, o = int(self.first[k]), int(self.moff[k]) // 2
            heights[o:o + len(l.merges)] = want[k][0]
            raw[f:f + l.m], q[f:f + l.m] = want[k][1], want[k][2]
        return heights, raw, q


def call(be, la: Launch, table=None, **over):
    """The launch on the backend, a table or a size replaced: (status words, heights, raw, q afterwards).  Guard bytes around
    heights, raw, q and the workspace are checked."""
    table = la.table if table is None else table
    d_shared, d_nw, d_seqs, d_table = be.upload(la.shared), be.upload(over.get("nw", la.nw)), be.upload(la.seqs), be.upload(table)
    weights = over.get("weights", la.weights)
    d_weights = None if weights is None else be.upload(weights)
    d_merges = be.upload(over.get("merges", la.merges))
    sizes = dict(heights=4 * (la.merges_words // 2), raw=8 * la.n_seqs, q=4 * la.n_seqs, ws=8 * la.ws_total)
    bufs = {k: be.full(n + 2 * GUARD, POISON8) for k, n in sizes.items()}
    d_status = be.upload(np.full(len(table), BLANK, np.int32))
    be.call("mprg_prog_leaf_weights", be.ptr(d_shared), over.get("shared_words", la.shared_words), be.ptr(d_nw), be.ptr(d_seqs),
            over.get("n_seqs", la.n_seqs), be.ptr(d_table), len(table), 0 if d_weights is None else be.ptr(d_weights),
            be.ptr(bufs["ws"]) + GUARD, over.get("ws_words", la.ws_total), be.ptr(d_merges), over.get("merges_words", la.merges_words),
            be.ptr(bufs["heights"]) + GUARD, be.ptr(bufs["raw"]) + GUARD, be.ptr(bufs["q"]) + GUARD, be.ptr(d_status), be.stream)
    out = {}
    for k, n in sizes.items():
        got = be.download(bufs[k], np.uint8, n + 2 * GUARD)
        assert (got[:GUARD] == POISON8).all() and (got[GUARD + n:] == POISON8).all(), k
        out[k] = got[GUARD:GUARD + n]
    return (be.download(d_status, np.int32, len(table)).tolist(), out["heights"].view(np.int32), out["raw"].view(np.int64),
            out["q"].view(np.int32))


def same(got, want, what=""):
    for name, g, w in zip(("heights", "raw", "q"), got[1:], want):
        bad = np.nonzero(g != w)[0]
        assert not len(bad), (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


def caterpillar_and_balanced():
    rng = random.Random(2)
    return [make_locus(rng, 4, merges=[(0, 1), (0, 2), (0, 3)]), make_locus(rng, 4, merges=[(0, 1), (2, 3), (0, 2)])]


@functools.lru_cache(maxsize=None)
def kernel_loci():
    """L = 1, 2, 3, the two shapes of 4, 5, 63, 64, 65 (a wavefront's rows), 257 (past a workgroup's threads in the leaf walk, 129
    row pairs); empty records between the leaves; UPGMA's merges and random valid ones (heights that fall: the clamp); with and
    without multiplicities.  No state of the kernel lives in LDS, so no m is a threshold there."""
    rng = random.Random(11)
    out = [make_locus(rng, 1, spare=2), make_locus(rng, 2), make_locus(rng, 2, spare=3, mult=9), make_locus(rng, 3, spare=1)]
    out += caterpillar_and_balanced()
    out += [make_locus(rng, 5, spare=4, mult=7, merges="random"), make_locus(rng, 63, spare=2), make_locus(rng, 64, mult=5),
            make_locus(rng, 65, spare=9, merges="random"), make_locus(rng, 257, spare=3, mult=12), make_locus(rng, 0, spare=2),
            make_locus(rng, 40, spare=40, mult=3, merges="random")]
    return out


@functools.lru_cache(maxsize=None)
def kernel_expected():
    return [expected(l) for l in kernel_loci()]


def falls(l: Locus, heights) -> bool:
    """A node of the locus's tree lies below one of its children: the clamp is needed."""
    node = {}
    for t, (u, v) in enumerate(l.merges):
        if any(key in node and heights[node[key]] > heights[t] for key in (u, v)):
            return True
        node[u] = t
    return False


def check_kernel(be):
    """Several loci of different m in one launch, unweighted and weighted ones side by side; then the unweighted ones with a null
    weights pointer.  Heights that fall occur, and the NumPy statement used for large loci agrees with the plain one."""
    loci, want = kernel_loci(), kernel_expected()
    assert any(falls(l, w[0]) for l, w in zip(loci, want))
    assert any(l.m > len(l.leaf) for l in loci) and any(l.leaf != list(range(len(l.leaf))) for l in loci)
    for l, w in zip(loci, want):
        for a, b in zip(expected_np(l), w):
            assert (a == b).all()
        h, raw, q = sa.leaf_weights(l.D(), l.leaf, l.merges, None if l.mult is None else l.mult[l.leaf])
        assert h == w[0].tolist() and raw == w[1][l.leaf].tolist() and q == w[2][l.leaf].tolist()
    la = Launch(loci)
    got = call(be, la)
    assert got[0] == [0] * len(loci)
    same(got, la.expected(want))
    plain = [k for k, l in enumerate(loci) if l.mult is None]
    la = Launch([loci[k] for k in plain], weighted=False)
    got = call(be, la)
    assert got[0] == [0] * len(plain)
    same(got, la.expected([want[k] for k in plain]), "null weights")


def check_extremes(be):
    """All D = 0: M = 0, every q = 1.  All D = 65 536: every height 65 536, every q = 256.  A caterpillar of equal distances."""
    rng = random.Random(3)
    zero = make_locus(rng, 9, spare=2, merges="random")
    zero = zero._replace(s=np.triu(np.minimum(zero.nw[:, None], zero.nw[None, :]), 1))
    far = make_locus(rng, 9, spare=2, merges="random")
    far = far._replace(s=np.zeros_like(far.s))
    none = make_locus(rng, 6, mult=4, merges="random")
    none = none._replace(nw=np.zeros_like(none.nw), s=np.zeros_like(none.s))          # nw = 0: D = 65 536 by the rule for m = 0
    loci = [zero, far, none]
    want = [expected(l) for l in loci]
    assert not want[0][0].any() and set(want[0][2][zero.leaf].tolist()) == {1}
    assert set(want[1][0].tolist()) == {SCALE} and set(want[1][2][far.leaf].tolist()) == {256}
    assert set(want[2][0].tolist()) == {SCALE}
    la = Launch(loci)
    got = call(be, la)
    assert got[0] == [0, 0, 0]
    same(got, la.expected(want))


def check_heavy(be):
    """One leaf of 2^20 - 3 beside three of 1: N_t passes 2^32 and comes close to 2^54; and two leaves of 2^19 each at D = 65 536,
    whose N_t is 2^54 exactly."""
    rng = random.Random(4)
    l = make_locus(rng, 4, spare=1, merges="random", spread=0.2)
    w = np.ones(l.m, np.int64)
    w[l.leaf[1]] = TOP - 3
    l = l._replace(mult=w)
    two = make_locus(rng, 2)
    two = two._replace(s=np.zeros_like(two.s), mult=np.full(2, TOP // 2, np.int64))
    loci = [l, two]
    want = [expected(x) for x in loci]
    D = l.D()
    sums = [int(w[a]) * int(w[b]) * int(D[a, b]) for a in l.leaf for b in l.leaf if a < b]
    assert max(sums) > 1 << 32 and int(w[l.leaf].sum()) == TOP and want[1][0].tolist() == [SCALE]
    la = Launch(loci)
    got = call(be, la)
    assert got[0] == [0, 0]
    same(got, la.expected(want))


def check_most_leaves(be):
    """4 096 leaves, the most the kernel takes, in two families of 1 024 and 3 072 (a cheap table: one distance inside a family,
    one between them), random merges inside each family, then the two joined."""
    L, cut = sa.PROG_MAX_LEAVES, 1024
    rng = random.Random(5)
    nw = np.full(L, 64, np.int64)
    fam = np.arange(L) >= cut
    s = np.triu(np.where(fam[:, None] == fam[None, :], 48, 8).astype(np.int64), 1)
    merges = random_merges(rng, list(range(cut))) + random_merges(rng, list(range(cut, L))) + [(0, cut)]
    l = Locus(L, list(range(L)), s, nw, None, merges)
    want = expected_np(l)
    assert len(set(want[2].tolist())) == 2 and want[2].max() == 256 and want[0][-1] == SCALE - SCALE * 8 // 64
    la = Launch([l], weighted=False)
    got = call(be, la)
    assert got[0] == [0]
    same(got, la.expected([want]))


# ---- 2. the refusals
def check_refusals(be):
    """One locus of three bad, in every way the header names, one at a time: MPRG_PG_BAD_ITEM or MPRG_PG_NO_SPACE for it and nothing
    of heights, raw and q written for it; the other two are what they are alone."""
    rng = random.Random(6)
    loci = [make_locus(rng, 6, spare=1, mult=3), make_locus(rng, 9, spare=2, mult=4), make_locus(rng, 5, mult=2)]
    want = [expected(l) for l in loci]
    la = Launch(loci)
    ok = call(be, la)
    assert ok[0] == [0, 0, 0]
    same(ok, la.expected(want))
    skipped = la.expected(want, skip=(1,))
    first, m, toff, woff, moff = la.table[1].tolist()
    leaf = loci[1].leaf

    def refused(code=1, **change):
        table, kw = la.table.copy(), {}
        for key, value in change.items():
            if key in ("first", "m", "toff", "woff", "moff"):
                table[1, ("first", "m", "toff", "woff", "moff").index(key)] = value
            else:
                kw[key] = value
        got = call(be, la, table=table, **kw)
        assert got[0] == [0, code, 0], (change, got[0])
        same(got, skipped, change)

    # mprg_prog_tree's range clauses
    refused(first=-1)
    refused(first=la.n_seqs - m + 1)
    refused(m=0)
    refused(m=1 << 31)
    refused(toff=-1)
    refused(toff=la.shared_words - m * m + 1)
    refused(moff=-2)
    refused(moff=la.merges_words + 2)
    refused(moff=la.merges_words - 2 * (len(leaf) - 1) + 2)             # fewer than L - 1 merges in range
    refused(moff=moff + 1)                                              # an odd offset: heights would not be at moff / 2
    # the multiplicities
    for value in (0, -1):
        w = la.weights.copy()
        w[first + leaf[2]] = value
        refused(weights=w)
    w = la.weights.copy()
    w[first + leaf[0]] = TOP + 1 - int(loci[1].mult[leaf[1:]].sum())
    refused(weights=w)                                                  # a sum of 2^20 + 1
    # the tables: an s above min(nw) > 0, an nw below 0
    nw = la.nw.copy()
    nw[first + leaf[3]] = -1
    refused(nw=nw)
    a, b = leaf[1], leaf[4]
    over = Launch([loci[0], loci[1]._replace(s=loci[1].s + np.where((np.arange(m)[:, None] == a) & (np.arange(m)[None, :] == b), 1000, 0)), loci[2]])
    got = call(be, over)
    assert got[0] == [0, 1, 0]
    same(got, skipped, "s above min(nw)")
    # a merge list that is no tree over the leaves
    at = int(moff)
    for change in ("dead key", "no leaf", "u >= v", "u == v", "v out of range", "u negative"):
        mg = la.merges.copy()
        pairs = mg[at:at + 2 * (len(leaf) - 1)].reshape(-1, 2)            # (a view)
        if change == "dead key":
            pairs[-1] = pairs[0]                                         # the first merge's V again: merged into U long ago
        elif change == "no leaf":
            pairs[0] = sorted((leaf[0], next(x for x in range(m) if x not in leaf)))
        elif change == "u >= v":
            pairs[0] = pairs[0][::-1]
        elif change == "u == v":
            pairs[0, 1] = pairs[0, 0]
        elif change == "v out of range":
            pairs[0] = (leaf[0], m)
        else:
            pairs[0] = (-1, leaf[0])
        refused(merges=mg)
    # the workspace
    refused(code=3, woff=-1)
    refused(code=3, woff=la.ws_total - sa.prog_weights_words(m) + 1)
    got = call(be, la, ws_words=la.ws_total - 1)                        # the last locus's need one word outside: the others are written
    assert got[0] == [0, 0, 3]
    same(got, la.expected(want, skip=(2,)), "ws_words")
    # more than 4 096 leaves
    L = sa.PROG_MAX_LEAVES + 1
    many = SimpleNamespace(shared=np.zeros(L * L, np.uint32), nw=np.full(L + 2, 9, np.int64), seqs=np.full((L + 2, 2), 5, np.int64),
                           n_seqs=L + 2, shared_words=L * L, merges=np.zeros(2 * L, np.int32), merges_words=2 * L, ws_total=6 * L,
                           weights=None, table=np.array([[1, L, 0, 0, 0]], np.int64))
    got = call(be, many)
    assert got[0] == [1] and (got[1] == BLANK).all() and (got[2] == BLANK64).all() and (got[3] == BLANK).all()


# ---- 3. whole MSAs
def fasta(msas):
    return [sa.msa_fasta(m) for m in msas]


def table_loci():
    return pr.table_loci()


def small_loci():
    """A 3-record locus of sequences shorter than 6 nt (no 6-mer: every D = 65 536, equal q), a 2-leaf locus, a locus of one
    record, and two leaves beside an empty record."""
    return [["ACGTA", "ACTA", "AGTA"], ["ACGTACGTTGACCA", "ACGTTCGTTGACA"], ["ACGTACGT"], ["ACGTACGTAA", "", "ACGTTCGTA"]]


def msa_loci():
    return table_loci() + rr.special_loci() + small_loci()


@functools.lru_cache(maxsize=None)
def msa_spec():
    return [wr.progressive(l) for l in msa_loci()]


def check_msas(be, **kw):
    """Rows equal the statement; exactly the issue's eight table loci differ from --progressive; the small loci keep their
    --progressive bytes; the counters."""
    loci, timings = msa_loci(), {}
    recs = [pc.records(l) for l in loci]
    msas = sa.star_msas(be, recs, progressive=True, seq_weights=True, timings=timings, **kw)
    for l, m, (rows, q, _, _, _) in zip(loci, msas, msa_spec()):
        assert m.rows_as_strings() == rows, l
        assert m.descriptions == [t for t, _ in pc.records(l)]
        cc.invariants(l, rows, equal_rows=False)
    # --progressive's bytes: prog_ref's rows, which tests/prog_common.py pins the flag-off run to (check_flag_off runs it once more)
    differ = [k for k, (l, m) in enumerate(zip(loci, msas)) if m.rows_as_strings() != pr.progressive_rows(l)]
    assert [k for k in differ if k < 18] == CHANGED, differ
    n = len(loci) - len(small_loci())
    assert not [k for k in differ if k >= n]
    assert len(set(msa_spec()[n][1].values())) == 1                     # the 3-record locus: equal q
    weighted = [spec[1] for l, spec in zip(loci, msa_spec()) if sum(1 for s in l if sr.normalise(s)) >= 3]
    assert timings["seq_weight_loci"] == len(weighted) and timings["seq_weight_s"] > 0
    assert timings["seq_weight_min_q"] == min(min(q.values()) for q in weighted)
    qs = [v for spec in msa_spec()[:18] for v in spec[1].values()]
    assert (min(qs), max(qs)) == (132, 256)                             # (the issue's prototype on these loci)
    return fasta(msas)


def check_same_bytes(be):
    """band, device_tree and a small budget with several groups and chunks: the statement's rows again."""
    pick = CHANGED[:5] + [0, 5] + list(range(18, len(msa_loci())))
    want = [msa_spec()[k][0] for k in pick]
    recs = [pc.records(msa_loci()[k]) for k in pick]
    for kw in (dict(band=True), dict(band=True, device_tree=True),
               dict(budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14, device_tree=True),
               dict(budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)):
        msas = sa.star_msas(be, recs, progressive=True, seq_weights=True, **kw)
        assert [m.rows_as_strings() for m in msas] == want, kw


def check_flag_off(be):
    """Flag off: today's bytes and today's recorded trace."""
    loci = [table_loci()[k] for k in CHANGED[:3]]
    recs = [pc.records(l) for l in loci]
    assert [m.rows_as_strings() for m in sa.star_msas(be, recs, progressive=True, seq_weights=False)] == [pr.progressive_rows(l) for l in loci]
    assert tr.run(be, "progressive")[1] == tr.golden()["progressive"]


def check_scaling(be):
    """Multiplying every q of a locus by a constant changes no plane and no score: a merge of rows weighted q gives the ops and the
    score of the rows weighted 3 q, through _prog_pairs as the rounds call it."""
    rng = random.Random(8)
    X, Y = pr.random_profiles(rng, 3, 40), pr.random_profiles(rng, 5, 55)
    text = np.concatenate([pc.codes(X).reshape(-1), pc.codes(Y).reshape(-1)])
    bufs = [(be.upload(text), len(text))]
    Xt, Yt = np.array([[0, 0, 3, 40]], np.int64), np.array([[0, 120, 5, 55]], np.int64)
    qx, qy = np.array([7, 200, 31], np.int64), np.array([256, 1, 90, 17, 133], np.int64)
    got = []
    for k in (1, 3):
        d_ops, ops_bytes, _, count, score = sa._prog_pairs(be, sa._bufs_table(be, bufs), 1, Xt, Yt, weights=([k * qx], [k * qy]))
        got.append((be.download(d_ops, np.uint8, ops_bytes)[:int(count[0])].tobytes(), int(score[0])))
    assert got[0] == got[1]
    ops, score = pr.align_profiles_np([r for r, n in zip(X, qx) for _ in range(n)], [r for r, n in zip(Y, qy) for _ in range(n)])
    assert got[0] == (ops[::-1].encode(), score)


def oversampled_loci():
    """Ten near-copies of one sequence and two outliers (the issue's over-sampled locus), and a second such locus."""
    out = []
    for seed in (1, 2):
        rng = random.Random(seed)
        root = "".join(rng.choice("ACGT") for _ in range(120))
        far = sr.mutate(rng, root, 0.15, 0.05)
        l = [sr.mutate(rng, root, 0.01, 0.0) for _ in range(10)] + [sr.mutate(rng, far, 0.03, 0.01) for _ in range(2)]
        rng.shuffle(l)
        out.append(l)
    return out


def check_oversampled(be):
    """The crowd gets less than the outliers: the largest q belongs to a record that is no near-copy."""
    loci = oversampled_loci()
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, seq_weights=True, device_tree=True)
    for l, m in zip(loci, msas):
        rows, q = wr.progressive(l)[:2]
        assert m.rows_as_strings() == rows
        order = sorted(q, key=q.get)
        assert max(q[a] for a in order[:10]) < min(q[a] for a in order[10:]) and q[order[-1]] == 256


def check_collapse(be):
    """collapse_common's loci: the statement on the weighted meaning, equal rows for equal sequences; a class of copies gets less
    than its multiplicity's share; a locus without copies the bytes it gets without collapse."""
    loci = cc.loci()
    for device_tree in (False, True):
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, collapse=True, seq_weights=True, device_tree=device_tree)
        plain = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, seq_weights=True)
        for l, m, p in zip(loci, msas, plain):
            rows = wr.progressive(l, collapse=True)[0]
            assert m.rows_as_strings() == rows, l
            cc.invariants(l, rows)
            if cc.n_classes(l)[0] == cc.n_classes(l)[1]:
                assert sa.msa_fasta(m) == sa.msa_fasta(p)
    shares = 0
    for l in loci:
        _, _, q, w, _, _, _, _ = wr.locus(l, collapse=True)
        heavy = [a for a in q if w[a] > 1]
        if len(q) >= 3 and heavy and len(set(q.values())) > 1:
            a = max(heavy, key=lambda x: w[x])
            shares += q[a] * sum(w[b] for b in q) < w[a] * sum(q.values())     # q's share of the class below its multiplicity's
    assert shares >= 2


def check_large_loci(be):
    """large_loci: 4 097 records over ten alleles: the statement's rows, on the host's tree and on the device's."""
    l = lc.loci()[0]
    rows = wr.progressive(l, collapse=True)[0]
    for device_tree in (True, False):
        wrapped = tr.TraceBackend(be)
        m, = sa.star_msas(wrapped, [pc.records(l)], progressive=True, collapse=True, large_loci=True, seq_weights=True, device_tree=device_tree)
        assert m.rows_as_strings() == rows
        cc.invariants(l, rows)
        calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
        assert ("mprg_prog_tree_wide" in calls) == device_tree and calls.count("mprg_prog_leaf_weights") == 1


def check_adjust_direction(be):
    """strand_ref's orientation, then the statement on the oriented sequences."""
    loci = pc.flipped_loci()[:8]
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, adjust_direction=True, seq_weights=True, device_tree=True)
    for l, m in zip(loci, msas):
        rev, _, ori = st.oriented(l)
        assert m.descriptions == st.titles(pc.records(l), rev) and m.rows_as_strings() == wr.progressive(ori)[0], l


def stage_loci():
    return [table_loci()[k] for k in (5, 6, 13)]


def check_retree_and_refine_tree(be):
    """retree=1 and refine_tree=1 against the statement: a rebuild runs with the q of the rebuilt tree on D', a step's realignment
    with the q of the tree that built the accepted MSA; acceptance by S with multiplicities.  refine afterwards, unweighted."""
    loci = stage_loci()
    recs = [pc.records(l) for l in loci]
    seen = set()
    for kw in (dict(retree=1), dict(refine_tree=1, device_tree=True), dict(retree=1, refine_tree=1, refine=2, band=True),
               dict(retree=1, collapse=True, device_tree=True)):
        info, tree, leave = [], [], []
        msas = sa.star_msas(be, recs, progressive=True, seq_weights=True, retreeing=info, tree_refinement=tree, refinement=leave, **kw)
        for k, (l, m) in enumerate(zip(loci, msas)):
            rows, _, want, want_tree, want_leave = wr.progressive(l, collapse=kw.get("collapse", False), retree=kw.get("retree", 0),
                                                                  refine_tree=kw.get("refine_tree", 0), refine=kw.get("refine", 0))
            assert m.rows_as_strings() == rows, (kw, k)
            assert (not kw.get("retree") or info[k] == want) and (not kw.get("refine_tree") or tree[k] == want_tree), (kw, k)
            assert not kw.get("refine") or leave[k] == want_leave, (kw, k)
            seen.update(("retree", i[1] > 0) for i in info[k:k + 1] if i)
            seen.update(("tree", t[1] > 0) for t in tree[k:k + 1] if t)
    assert ("retree", True) in seen and ("tree", True) in seen, seen


# ---- 4. what moves
def check_trace(be):
    """With the flag on, beside the flag-off run: the same calls plus one mprg_prog_leaf_weights per tree group (and, on the host's
    tree, the distances launched again); downloaded in addition are the launch's status words and q, nothing else."""
    recs = [pc.records(l) for l in table_loci()[4:10]]
    n_seqs = sum(len(r) for r in recs)
    for device_tree in (True, False):
        off, on = tr.TraceBackend(be), tr.TraceBackend(be)
        sa.star_msas(off, recs, progressive=True, device_tree=device_tree)
        sa.star_msas(on, recs, progressive=True, device_tree=device_tree, seq_weights=True)
        count = lambda b, name: sum(line.split()[1] == name for line in b.lines if line.startswith("call "))
        assert count(on, "mprg_prog_leaf_weights") == 1 and count(off, "mprg_prog_leaf_weights") == 0
        assert count(on, "mprg_prog_distances") == count(off, "mprg_prog_distances") + (0 if device_tree else 1)
        for name in ("mprg_prog_tree", "mprg_align_profile_pairs", "mprg_prog_rows"):
            assert count(on, name) == count(off, name)
        assert count(on, "mprg_prog_columns_weighted") == count(off, "mprg_prog_columns") > 0
        # (the MSAs' text, uint8, has another size where the weights change a width)
        downloads = lambda b: sorted(line for line in b.lines if line.startswith("download ") and "uint8" not in line)
        extra = downloads(on)
        for line in downloads(off):
            extra.remove(line)
        want = [f"download int32 {len(recs)}", f"download int32 {n_seqs}"] + ([] if device_tree else [f"download int32 {n_seqs}"])
        assert sorted(extra) == sorted(want), extra                     # (the host's tree: the second distances launch's status words)


# ---- 5. parameters and the command line
def check_parameters(be):
    import pytest
    recs = [pc.records(pr.clade_locus(42, 8))]
    with pytest.raises(ValueError):
        sa.star_msas(be, recs, seq_weights=True)
    assert sa.prog_weights_words(7) == 42


def cli_loci():
    return [pr.clade_locus(k, 8, L=(60, 90)) for k in range(6)]


def log_line():
    qs = [v for l in cli_loci() for v in wr.progressive(l)[1].values()]
    return "--seq-weights: 6 loci weighted, smallest weight %d" % min(qs)


def write_inputs(src):
    """Six small loci as unaligned FASTA files under src: per file name the MSA text --progressive --seq-weights writes."""
    want = {}
    for k, l in enumerate(cli_loci()):
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(l)]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"gene{k}.fa"] = wr.fasta(recs)
    return want
