"""The checks of `from_msa --unaligned --progressive --retree` (make_prg_amd/from_msa/star_align.py "Retree",
csrc/k_prog_retree.inc), for any backend: tests/test_retree_emulated.py runs them on the CPU emulation build,
tests/test_gpu_retree.py on the MI355X.  mprg_prog_identities called directly against tests/retree_ref.py's plain statement (the
shapes around the row block and the LDS column tile, odd offsets, two buffers, permuted leaves, poisoned tables), its refusals,
the tables through the tree entry points, whole MSAs against the statement, the compositions, and what moves."""
import functools

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import collapse_common as cc
from tests import large_common as lc
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import retree_ref as rt
from tests import star_ref as sr
from tests import star_trace as tr
from tests import strand_ref as st
from tests import treerefine_ref as tf

B = sa.PI_BLOCK_ROWS
TILE = 2048                                    # PI_TILE of csrc/k_prog_retree.inc: the columns of the kernel's LDS tile
LETTERS = "ACGT-RYKMSWN"
POISON32, POISON64 = 0xEEEEEEEE, -7
ROWS = (1, 2, B - 1, B, B + 1, 2 * B + 1, 65)
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
OFFSETS = (0, 1, 2, 3, 13)


def ascii_rows(t):
    return ["".join(LETTERS[c] for c in row) for row in t]


# ---- 1. the kernel against the plain statement
def text(rng, R, W):
    """An R x W text over all twelve codes, rows related enough to match often.  R + W even: whole columns of '-', of N and of one
    base; R + W odd: one row all '-' and, from three rows on, one row all N (nw' = 0)."""
    base = rng.integers(0, 4, W)
    t = np.where(rng.random((R, W)) < 0.6, base[None, :], rng.integers(0, 12, (R, W))).astype(np.uint8)
    if (R + W) % 2 == 0 and W >= 3:
        t[:, 0], t[:, W // 2], t[:, W - 1] = 4, 11, 2
    if (R + W) % 2 and R >= 2:
        t[1] = 4
        t[2 % R] = 11
    return t


class Launch:
    """The tables of one mprg_prog_identities launch over texts laid out in buffers, and what the plain statement expects of it.
    `shared` has two guard words in front of the tables and two behind shared_words, `nw` one in front and one behind n_seqs."""

    def __init__(self, rng, texts, n_bufs=2):
        n = len(texts)
        self.texts = texts
        self.bufs = [[] for _ in range(n_bufs)]
        used = [0] * n_bufs
        self.items = np.zeros((n, sa.PI_ITEM_FIELDS), np.int64)
        self.leaf, loff, first, toff = [], 0, 1, 2
        for k, t in enumerate(texts):
            R, W = t.shape
            b = k % n_bufs
            off = -(-used[b] // 64) * 64 + OFFSETS[(k // n_bufs) % len(OFFSETS)]
            self.bufs[b].append((off, t))
            used[b] = off + t.size
            m = R + 1 + k % 3                                            # records without a row: their entries stay what they were
            self.leaf.append(rng.permutation(m)[:R].astype(np.int32))   # rows not in index order: the min / max placement
            self.items[k] = [b, off, R, W, loff, first, m, toff]
            loff, first, toff = loff + R, first + m, toff + m * m
        self.buf_bytes = used
        self.leaf_words, self.n_seqs, self.shared_words = loff, first, toff
        blocks = -(-self.items[:, 2] // B)
        self.work = np.stack([np.repeat(np.arange(n), blocks), np.concatenate([np.arange(x) for x in blocks])], 1).astype(np.int32)

    def buffers(self):
        out = []
        for parts, size in zip(self.bufs, self.buf_bytes):
            a = np.zeros(size + 64, np.uint8)                           # (A between and behind the texts: a cell read outside a text would match)
            for off, t in parts:
                a[off:off + t.size] = t.reshape(-1)
            out.append(a)
        return out

    def expected(self, skip=()):
        """(shared, nw) as the launch leaves them, the items `skip` not written."""
        shared, nw = np.full(self.shared_words + 2, POISON32, np.uint32), np.full(self.n_seqs + 1, POISON64, np.int64)
        for k, t in enumerate(self.texts):
            if k in skip:
                continue
            _, _, R, _, _, first, m, toff = self.items[k].tolist()
            s, cells = rt.identities(ascii_rows(t))
            lf = self.leaf[k]
            for r in range(R):
                nw[first + lf[r]] = cells[r]
                for q in range(r + 1, R):
                    a, b = sorted((int(lf[r]), int(lf[q])))
                    shared[toff + a * m + b] = s[r][q]
        return shared, nw


def call(be, la: Launch, items=None, work=None, leaf=None, **over):
    """The launch on the backend, a table or a size replaced: (status words, shared, nw afterwards)."""
    bufs = [be.upload(a) for a in la.buffers()]
    sizes = over.get("buf_bytes", la.buf_bytes)
    d_bufs = be.upload(np.array([[be.ptr(b), n] for b, n in zip(bufs, sizes)], np.int64))
    items = la.items if items is None else items
    work = la.work if work is None else work
    flat = np.concatenate(la.leaf) if leaf is None else leaf
    d_items, d_work, d_leaf = be.upload(items), be.upload(work), be.upload(flat.astype(np.int32))
    d_shared = be.upload(np.full(la.shared_words + 2, POISON32, np.uint32))
    d_nw = be.upload(np.full(la.n_seqs + 1, POISON64, np.int64))
    d_status = be.upload(np.full(len(work), 0x5C5C5C5C, np.int32))
    be.call("mprg_prog_identities", be.ptr(d_bufs), len(bufs), be.ptr(d_items), over.get("n_items", len(items)), be.ptr(d_work), len(work),
            be.ptr(d_leaf), over.get("leaf_words", la.leaf_words), be.ptr(d_shared), over.get("shared_words", la.shared_words), be.ptr(d_nw),
            over.get("n_seqs", la.n_seqs), be.ptr(d_status), be.stream)
    return (be.download(d_status, np.int32, len(work)).tolist(), be.download(d_shared, np.uint32, la.shared_words + 2),
            be.download(d_nw, np.int64, la.n_seqs + 1))


@functools.lru_cache(maxsize=None)
def kernel_launch():
    """Every R of ROWS at every W of WIDTHS, one launch: items of different R and W side by side, in two buffers, at the offsets
    0, 1, 2, 3 and 13 behind a 64-byte boundary."""
    rng = np.random.default_rng(5)
    texts = [text(rng, R, W) for W in WIDTHS for R in ROWS]
    la = Launch(rng, texts)
    return la, la.expected()


def check_kernel(be):
    la, (shared, nw) = kernel_launch()
    assert {int(o) % 64 for o in la.items[:, 1]} == set(OFFSETS) and set(la.items[:, 0].tolist()) == {0, 1}
    assert sum((t == 4).all(1).any() and (t == 11).all(1).any() for t in la.texts) > 20
    assert sum((t == 4).all(0).any() and (t == 11).all(0).any() and (t == 2).all(0).any() for t in la.texts) > 20
    status, got_shared, got_nw = call(be, la)
    assert status == [0] * len(la.work)
    bad = np.nonzero(got_nw != nw)[0]
    assert not len(bad), (bad[:5], got_nw[bad[:5]], nw[bad[:5]])
    bad = np.nonzero(got_shared != shared)[0]
    assert not len(bad), (bad[:5], got_shared[bad[:5]], shared[bad[:5]], la.items[np.searchsorted(la.items[:, 7], bad[0], "right") - 1])
    # what is written: the leaf pairs' b > a entries and the leaves' nw, nothing else, the guard words included
    assert (shared[:2] == POISON32).all() and (shared[-2:] == POISON32).all() and nw[0] == nw[-1] == POISON64
    assert 0 < (shared != POISON32).sum() < len(shared) and 0 < (nw != POISON64).sum() < len(nw)
    # the helper gives the same numbers, every record a row
    for t, (s, cells) in zip(la.texts[::9], sa.prog_identities(be, la.texts[::9])):
        want_s, want_cells = rt.identities(ascii_rows(t))
        assert cells.tolist() == want_cells and np.triu(s, 1).tolist() == np.triu(np.array(want_s).reshape(len(t), len(t)), 1).tolist()
        assert not np.tril(s).any()


# ---- 2. the refusals
def check_refusals(be):
    """One item of three bad, in every way the header names: its work items get MPRG_PG_BAD_ITEM and nothing else is written for it;
    the other two are what they are alone."""
    rng = np.random.default_rng(6)
    la = Launch(rng, [text(rng, 5, 40), text(rng, 2 * B + 3, 37), text(rng, 3, 70)], n_bufs=1)
    of_b = (la.work[:, 0] == 1).astype(int).tolist()
    assert sum(of_b) == 3
    ok = call(be, la)
    want = la.expected()
    assert ok[0] == [0] * len(la.work) and (ok[1] == want[0]).all() and (ok[2] == want[1]).all()
    skipped = la.expected(skip=(1,))

    def refused(status=None, expect=skipped, **change):
        items, kw = la.items.copy(), {}
        for key, value in change.items():
            if key in ("buf", "off", "R", "W", "loff", "first", "m", "toff"):
                items[1, ("buf", "off", "R", "W", "loff", "first", "m", "toff").index(key)] = value
            else:
                kw[key] = value
        got = call(be, la, items=items, **kw)
        assert got[0] == (of_b if status is None else status), change
        assert (got[1] == expect[0]).all() and (got[2] == expect[1]).all(), change

    _, off, R, W, loff, first, m, toff = la.items[1].tolist()
    # the text one byte outside its buffer (it is the buffer's last but one: put behind everything else), a negative offset
    refused(off=la.buf_bytes[0] - R * W + 1)
    refused(off=-1)
    refused(buf=1)
    refused(buf=-1)
    refused(R=0)
    refused(W=0)
    refused(loff=la.leaf_words - R + 1)                                  # the leaf entries one word outside leaf_words
    refused(loff=-1)
    refused(first=la.n_seqs - m + 1)                                    # first + m one past n_seqs
    refused(first=-1)
    refused(toff=la.shared_words - m * m + 1)                            # the table one word outside shared_words
    refused(toff=-1)
    for value in (m, -1):                                                # a leaf index of m and of -1, in the item's last block
        leaf = np.concatenate(la.leaf)
        leaf[loff + R - 1] = value
        refused(leaf=leaf)
    # an item index and a block index out of range: those work items alone
    for column, value in ((0, 3), (0, -1), (1, 3), (1, -1)):
        work = la.work.copy()
        k = int(np.nonzero(work[:, 0] == 0)[0][0])
        work[k, column] = value
        status, shared, nw = call(be, la, work=work)
        assert status == [int(i == k) for i in range(len(work))], (column, value)
        only = la.expected(skip=(0,))
        assert (shared == only[0]).all() and (nw == only[1]).all()     # (item 0 has one block)
    # the last item's table one word outside: the others are written
    got = call(be, la, shared_words=la.shared_words - 1)
    last = la.expected(skip=(2,))
    assert got[0] == [int(i == 2) for i in la.work[:, 0]] and (got[1] == last[0]).all() and (got[2] == last[1]).all()


# ---- 3. the tables feed the tree unchanged
def tree_loci():
    return [l for l in pc.msa_loci() if sum(1 for s in l if sr.normalise(s)) >= 3]


def check_trees(be):
    """D' of prog_common's progressive MSAs: through prog_distance_matrix and prog_tree it is retree_ref's tree; _retree_trees gives
    that tree from the device and from the host, unweighted, weighted, and with weights above 4 096 (mprg_prog_tree_wide)."""
    loci = tree_loci()
    rows = [pr.progressive_rows(l) for l in loci]
    leaves = [[a for a, s in enumerate(l) if sr.normalise(s)] for l in loci]
    texts = [pc.codes([r[a] for a in lv]) for r, lv in zip(rows, leaves)]
    got = sa.prog_identities(be, texts, leaves, [len(l) for l in loci])
    rng = np.random.default_rng(9)
    heavy = [rng.integers(1, 6, len(l)) for l in loci]
    wide = [w * 1500 for w in heavy]
    assert all(w[lv].sum() > sa.PROG_MAX_LEAVES for w, lv in zip(wide, leaves))
    want = {}
    for k, (l, r, lv, (s, nw)) in enumerate(zip(loci, rows, leaves, got)):
        D = rt.distances(lv, [r[a] for a in lv])
        Dm = sa.prog_distance_matrix(s, nw)
        assert all(Dm[a, b] == D[a][b] for a in lv for b in lv), l
        for name, w in (("plain", None), ("heavy", heavy[k]), ("wide", wide[k])):
            want[name, k] = tf.merge_order(D, lv, None if w is None else w.tolist())[0]
            assert sa.prog_tree(Dm, lv, None if w is None else w[lv]) == want[name, k], (name, l)
    # the stage's own path: the texts in a buffer behind the chunk's codes, the rows in leaf order
    chunk = sa._pack(be, [sa.locus_codes(str(k), pc.records(l)) for k, l in enumerate(loci)])
    off = sa.exclusive_sum(np.array([t.size for t in texts], np.int64))
    flat = np.concatenate([t.reshape(-1) for t in texts])
    bufs = [(chunk.d_codes, chunk.codes_bytes), (be.upload(flat), len(flat))]
    where = {k: (1, int(off[k]), *t.shape) for k, t in enumerate(texts)}
    order = [np.array(lv, np.int64) for lv in leaves]
    sel = np.arange(len(loci))
    for name, ws in (("plain", None), ("heavy", heavy), ("wide", wide)):
        weights = None if ws is None else np.concatenate(ws).astype(np.int64)
        for device_tree in (True, False):
            wrapped = tr.TraceBackend(be)
            merges = sa._retree_trees(wrapped, chunk, sel, where, order, bufs, weights, 1 << 16, device_tree)
            assert [merges[k] for k in range(len(loci))] == [want[name, k] for k in range(len(loci))], (name, device_tree)
            calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
            assert calls.count("mprg_prog_identities") >= 2                     # (the budget makes several groups)
            if device_tree:
                assert calls.count("mprg_prog_tree_wide" if name == "wide" else "mprg_prog_tree") == calls.count("mprg_prog_identities")
                assert not any(line.startswith("download uint32") for line in wrapped.lines)
            else:
                assert set(calls) == {"mprg_prog_identities"}


# ---- 4. whole MSAs
def fasta(msas):
    return [sa.msa_fasta(m) for m in msas]


def msa_loci():
    return pr.table_loci() + [pr.clade_locus(42, 8)]


@functools.lru_cache(maxsize=None)
def msa_spec(rebuilds=2):
    return [rt.progressive(l, rebuilds) for l in msa_loci()]


def check_counts():
    """What the issue's table promises of these loci under two rebuilds: every branch of the rule occurs."""
    info = [i for _, i, _, _, _ in msa_spec()]
    assert any(i[:3] == (2, 2, None) for i in info), "no locus accepts twice"
    assert any(i[2] == "refused" for i in info) and any(i[:3] == (2, 1, "same") for i in info) and any(i[:3] == (1, 0, "same") for i in info)
    assert sum(1 for i in info[:18] if i[1]) == 12 and info[-1][:3] == (1, 0, "same")


def invariants(l, rows):
    cc.invariants(l, rows, equal_rows=False)


def check_msas(be, **kw):
    """Rows, retreeing and progression equal the statement; the spec's promises on the result."""
    check_counts()
    loci, info, prog, timings = msa_loci(), [], [], {}
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, retree=2, retreeing=info, progression=prog, timings=timings, **kw)
    off = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, **kw)
    for l, m, plain, got, got_prog, (rows, want, want_prog, _, _) in zip(loci, msas, off, info, prog, msa_spec()):
        assert m.rows_as_strings() == rows, l
        assert got == want and got_prog == want_prog, (got, want, got_prog, want_prog)
        assert m.descriptions == [t for t, _ in pc.records(l)]
        invariants(l, rows)
        assert got[4] >= got[3] and (got[4] > got[3]) == (got[1] > 0)
        if not got[1]:
            assert sa.msa_fasta(m) == sa.msa_fasta(plain)                       # nothing accepted: the --progressive bytes
        else:
            assert sa.msa_fasta(m) != sa.msa_fasta(plain)
    assert timings["retree_loci"] == len(loci) and timings["retree_accepted"] == sum(i[1] for i in info) and timings["retree_s"] > 0
    assert timings["retree_same_tree"] == sum(i[2] == "same" for i in info) and timings["retree_refused"] == sum(i[2] == "refused" for i in info)
    assert timings["retree_rebuilds"] == timings["retree_accepted"] + timings["retree_refused"] and timings["retree_over_bound"] == 0
    return fasta(msas), info


def check_one_rebuild(be):
    """N = 1: the statement's rows; an accepted locus has reason None."""
    loci = msa_loci()[4:8]
    info = []
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, retree=1, retreeing=info)
    for l, m, got in zip(loci, msas, info):
        rows, want = rt.progressive(l, 1)[:2]
        assert m.rows_as_strings() == rows and got == want
    assert any(i[:3] == (1, 1, None) for i in info)


# ---- 5. the compositions
def check_same_bytes(be):
    """band, device_tree and a small budget with several groups and chunks: the statement's rows again, the same tuples."""
    want = [rows for rows, _, _, _, _ in msa_spec()]
    base = [i for _, i, _, _, _ in msa_spec()]
    for kw in (dict(band=True), dict(device_tree=True), dict(band=True, device_tree=True),
               dict(budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14, device_tree=True),
               dict(budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)):
        info = []
        msas = sa.star_msas(be, [pc.records(l) for l in msa_loci()], progressive=True, retree=2, retreeing=info, **kw)
        assert [m.rows_as_strings() for m in msas] == want and info == base, kw


def check_adjust_direction(be):
    """strand_ref's orientation, then the statement on the oriented sequences."""
    loci = pc.flipped_loci()[:8]
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, adjust_direction=True, retree=2, device_tree=True)
    for l, m in zip(loci, msas):
        rev, _, ori = st.oriented(l)
        assert m.descriptions == st.titles(pc.records(l), rev) and m.rows_as_strings() == rt.progressive(ori, 2)[0], l


def check_collapse(be):
    """collapse_common's loci: the statement on the weighted meaning, equal rows for equal sequences, a locus without copies the
    bytes it gets without collapse."""
    loci = cc.loci()
    for device_tree in (False, True):
        info = []
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, collapse=True, retree=2, retreeing=info, device_tree=device_tree)
        plain = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, retree=2)
        for l, m, p, got in zip(loci, msas, plain, info):
            rows, want = rt.progressive(l, 2, collapse=True)[:2]
            assert m.rows_as_strings() == rows and got == want, l
            cc.invariants(l, rows)
            if cc.n_classes(l)[0] == cc.n_classes(l)[1]:
                assert sa.msa_fasta(m) == sa.msa_fasta(p)
        assert any(cc.n_classes(l)[0] == cc.n_classes(l)[1] for l in loci) and any(i[1] for i in info)


def check_large_loci(be):
    """large_loci: a locus of 4 097 records over ten alleles goes through the stage like any other (its tree by mprg_prog_tree_wide
    with device_tree); with a small max_leaves the loci above it keep the star bytes and get None."""
    l = lc.loci()[0]
    rows, want = rt.progressive(l, 2, collapse=True)[:2]
    for device_tree in (True, False):
        info = []
        wrapped = tr.TraceBackend(be)
        m, = sa.star_msas(wrapped, [pc.records(l)], progressive=True, collapse=True, large_loci=True, retree=2, retreeing=info, device_tree=device_tree)
        assert m.rows_as_strings() == rows and info == [want]
        cc.invariants(l, rows)
        calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
        assert ("mprg_prog_tree_wide" in calls) == device_tree and "mprg_prog_identities" in calls
    loci = cc.loci()
    kw = dict(progressive=True, collapse=True, large_loci=True, max_leaves=6)
    info, prog = [], []
    msas = sa.star_msas(be, [pc.records(x) for x in loci], retree=2, retreeing=info, progression=prog, **kw)
    star = sa.star_msas(be, [pc.records(x) for x in loci], **kw)
    assert any(p[2] for p in prog) and not all(p[2] for p in prog)
    for x, m, s, got, p in zip(loci, msas, star, info, prog):
        if p[2]:
            assert got is None and sa.msa_fasta(m) == sa.msa_fasta(s)
        else:
            assert (m.rows_as_strings(), got) == rt.progressive(x, 2, collapse=True)[:2]


def check_refine_after(be):
    """refine_tree=1 and refine=2 behind it: the statement followed by treerefine_ref on the accepted tree and refine_ref."""
    loci = msa_loci()[4:7] + [msa_loci()[13]]
    for kw in (dict(refine_tree=1), dict(refine=2), dict(refine_tree=1, refine=2, band=True, device_tree=True)):
        info, tree, leave = [], [], []
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, retree=2, retreeing=info, tree_refinement=tree, refinement=leave, **kw)
        for k, (l, m) in enumerate(zip(loci, msas)):
            rows, want, _, want_tree, want_leave = rt.progressive(l, 2, refine_tree=kw.get("refine_tree", 0), refine=kw.get("refine", 0))
            assert m.rows_as_strings() == rows and info[k] == want, (kw, l)
            assert (not tree or tree[k] == want_tree) and (not leave or leave[k] == want_leave), (kw, l)
        assert any(i[1] for i in info)


def check_limit(be, columns=520):
    """The spec's Limit on the rebuilds, with the stage's limit function replaced by "fewer than `columns` columns in all" (the real
    one needs merges of 10^6 columns): a locus with such a merge in a rebuild stops with "limit" and the MSA it had, in the middle
    of rounds that go on for the others; every other locus is the statement's."""
    loci, info = msa_loci(), []
    real = sa._tree_step_fits
    sa._tree_step_fits = lambda WX, WY, budget_words: WX + WY < columns
    try:
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, retree=2, retreeing=info, device_tree=True)
    finally:
        sa._tree_step_fits = real
    kinds = set()
    for l, m, got, (rows, want, _, _, _) in zip(loci, msas, info, msa_spec()):
        if got[2] == "limit":
            assert got[0] == got[1] + 1 and got[:2] <= want[:2] and m.rows_as_strings() == rt.progressive(l, got[1])[0], l
        else:
            assert got == want and m.rows_as_strings() == rows, l
        kinds.add((got[2], got[1]))
    assert ("limit", 0) in kinds and len({k for k in kinds if k[0] != "limit" and k[1]}) >= 1, kinds


# ---- 6. what moves
def check_trace(be):
    """With device_tree no uint32 table and no text comes back during the stage; an iteration in which every locus stops "same"
    aligns nothing; with the flag off the golden scenarios' call lists are what they were."""
    loci = msa_loci()
    wrapped = tr.TraceBackend(be)
    sa.star_msas(wrapped, [pc.records(l) for l in loci], progressive=True, retree=2, device_tree=True)
    calls = [k for k, line in enumerate(wrapped.lines) if line.startswith("call mprg_prog_identities")]
    last_objective = max(k for k, line in enumerate(wrapped.lines) if line.startswith("call mprg_tree_objective"))
    stage = wrapped.lines[calls[0]:last_objective + 3]             # (behind the call: its status words and S)
    assert len(calls) == 2 and not any(line.startswith(("download uint32", "download uint8")) for line in stage)
    assert sum(line.startswith("download int64") for line in stage) == 2      # S of the rebuilds, 8 bytes a locus
    same = [pr.clade_locus(42, 8)]
    assert rt.progressive(same[0], 2)[1][:3] == (1, 0, "same")
    for device_tree in (True, False):
        plain, wrapped = tr.TraceBackend(be), tr.TraceBackend(be)
        sa.star_msas(plain, [pc.records(l) for l in same], progressive=True, device_tree=device_tree)
        sa.star_msas(wrapped, [pc.records(l) for l in same], progressive=True, retree=2, device_tree=device_tree)
        count = lambda b, name: sum(line.startswith("call " + name) for line in b.lines)
        assert count(wrapped, "mprg_align_profile_pairs") == count(plain, "mprg_align_profile_pairs") > 0
        assert count(wrapped, "mprg_prog_identities") == 1 and count(wrapped, "mprg_tree_objective") == 1
    assert tr.run(be, "progressive")[1] == tr.golden()["progressive"]


# ---- 7. parameters
def check_parameters(be):
    import pytest
    recs = [pc.records(pr.clade_locus(42, 8))]
    for kw in (dict(retree=1), dict(retree=0, progressive=True), dict(retree=sa.RETREE_MAX + 1, progressive=True), dict(retree=True, progressive=True)):
        with pytest.raises(ValueError):
            sa.star_msas(be, recs, **kw)
    assert fasta(sa.star_msas(be, recs, progressive=True, retree=sa.RETREE_MAX)) == fasta(sa.star_msas(be, recs, progressive=True))


def cli_loci():
    return [pr.clade_locus(k, 8, L=(60, 90)) for k in range(6)]


def cli_counts():
    """(loci rebuilt, accepted, same tree, refused) of the command-line test's six loci under two rebuilds, by the statement."""
    info = [rt.progressive(l, 2)[1] for l in cli_loci()]
    same, refused = (sum(i[2] == why for i in info) for why in ("same", "refused"))
    accepted = sum(i[1] for i in info)
    return accepted + refused, accepted, same, refused


def log_line():
    return "--retree 2: %d loci rebuilt, %d accepted, %d same tree, %d refused" % cli_counts()


def check_cli_counts(be):
    """The counters the command line logs are the statement's counts, on the loci of the command-line test."""
    timings = {}
    msas = sa.star_msas(be, [pc.records(l) for l in cli_loci()], progressive=True, retree=2, timings=timings)
    assert [m.rows_as_strings() for m in msas] == [rt.progressive(l, 2)[0] for l in cli_loci()]
    assert tuple(timings[k] for k in ("retree_rebuilds", "retree_accepted", "retree_same_tree", "retree_refused")) == cli_counts()
    assert cli_counts()[0] > 0


def write_inputs(src):
    """Six small loci as unaligned FASTA files under src: per file name the MSA text --progressive --retree 2 writes."""
    want = {}
    for k, l in enumerate(cli_loci()):
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(l)]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"gene{k}.fa"] = rt.fasta(recs, 2)
    return want
