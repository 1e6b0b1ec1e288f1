"""What the emulated and the GPU tests of `from_msa --unaligned --progressive --refine-tree` share: mprg_tree_split and
mprg_tree_objective called directly through the C ABI (against NumPy, mprg_refine_counts and the plain-Python objective; every
status code with nothing else written), and whole MSAs against the spec's plain-Python statement (tests/treerefine_ref.py, computed
once per process): alone, under --band, --device-tree and a small budget, with --collapse-identical, above the cap, composed with
--adjust-direction and --refine, and with the flag off."""
import functools

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import collapse_common as cc
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import refine_common as rc
from tests import refine_ref as rr
from tests import star_ref as sr
from tests import strand_ref as st
from tests import treerefine_ref as tr

POISON = 0x5C
GAP = 4
SHAPES = [(R, W) for R in (2, 3, 7) for W in (1, 255, 256, 257, 600)] + [(257, 257), (257, 600)]   # the widths: around the 256-column tile
KINDS = ("first", "last", "tile", "alternating", "all")
SMALL_BUDGET = dict(budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)   # prog_common.check_msas' small run


# ---- mprg_tree_split
@functools.lru_cache(maxsize=None)
def split_cases():
    """(text, side bytes, kind) for every kind of KINDS at every shape of SHAPES (a text of one column: once, as it is): Y's rows all
    '-' in the first column, in the last, over the whole second 256-column tile (texts below 512 columns: the columns from 100 on),
    Y and X all '-' in alternating columns, a Y that keeps every column.  The sides are dealt at random with a row each at least;
    two rows are one row each."""
    rng = np.random.default_rng(41)
    out = []
    for k, (R, W) in enumerate(SHAPES):
        for q, what in enumerate(KINDS if W > 1 else ("all",)):
            t = rng.integers(0, 12, (R, W)).astype(np.uint8)
            t[rng.random((R, W)) < 0.3] = GAP
            side = (rng.random(R) < 0.5).astype(np.uint8)
            side[0], side[R - 1] = (k + q) % 2, 1 - (k + q) % 2
            y, x = np.nonzero(side == 0)[0], np.nonzero(side == 1)[0]
            t[y[0], W // 2] = t[x[0], W // 2] = 1                    # (both sides keep a column, whatever the kind blanks)
            if W == 1:
                pass
            elif what == "first":
                t[y, 0] = GAP
            elif what == "last":
                t[y, W - 1] = GAP
            elif what == "tile":
                t[np.ix_(y, np.arange(256, 512) if W >= 512 else np.arange(100, W))] = GAP
                t[y[0], W - 1] = 2                                   # (a kept column behind the blank ones)
            elif what == "alternating":
                t[np.ix_(y, np.arange(0, W, 2))] = GAP
                t[np.ix_(x, np.arange(1, W, 2))] = GAP
                t[y[0], 1], t[x[0], 0] = 2, 3
            else:
                rows = t[y]
                rows[rows == GAP] = 0
                t[y] = rows
            out.append((t, side, what))
    return out


def check_split_cases():
    """The cases are what their kinds say, by the NumPy statement: 'first' and 'last' drop Y's column 0 and W - 1 at widths above
    256 too; a 'tile' text of 512 columns or more has a whole 256-column tile without a kept column of Y and a kept column of Y in
    the tile behind it; 'alternating' keeps every other column; 'all' keeps all."""
    cases = split_cases()
    assert {(t.shape, w) for t, _, w in cases} == {(s, w) for s in SHAPES for w in (KINDS if s[1] > 1 else ("all",))}
    empty_tiles = 0
    for t, side, what in cases:
        R, W = t.shape
        keep = (t[side == 0] != GAP).any(0)
        assert keep.any() and (t[side == 1] != GAP).any(0).any() and 1 <= (side == 0).sum() < R
        if W == 1:
            continue
        if what == "first":
            assert not keep[0]
        elif what == "last":
            assert not keep[W - 1]
        elif what == "tile" and W >= 512:
            assert not keep[256:512].any() and keep[:256].any() and keep[512:].any()
            empty_tiles += 1
        elif what == "tile":
            assert not keep[100:W - 1].any() and keep[W - 1]
        elif what == "alternating":
            assert not keep[0::2].any() and not (t[side == 1] != GAP).any(0)[3::2].any()
        elif what == "all":
            assert keep.all()
    assert empty_tiles == 4 and sum(1 for t, _, w in cases if w in ("first", "last") and t.shape[1] > 256) >= 16


def split_ref(t, side):
    """(Y's text, X's text) in NumPy."""
    return tuple(t[side == s][:, (t[side == s] != GAP).any(0)] for s in (0, 1))


def _split(be, texts, sides, items=None, sides_bytes=None, n_cols=None, n_tiles=None, out_bytes=None, text_bytes=None, pad=64, work=None):
    """mprg_tree_split on these texts, with the tables sa.tree_split makes unless `items` replaces them: (status words, widths,
    the output buffer with `pad` bytes behind it, the item table).  Output, widths and status start as POISON."""
    n = len(texts)
    text = np.concatenate([t.reshape(-1) for t in texts])
    R, W = np.array([t.shape[0] for t in texts], np.int64), np.array([t.shape[1] for t in texts], np.int64)
    tiles = -(-W // 256) + 1
    need = int((R * W).sum())
    if items is None:
        items = np.stack([np.zeros(n, np.int64), sa.exclusive_sum(R * W), R, W, sa.exclusive_sum(R), sa.exclusive_sum(R * W), sa.exclusive_sum(W),
                          sa.exclusive_sum(tiles)], 1)
    items = np.array(items, np.int64)
    work = sa._tile_work(W) if work is None else np.array(work, np.int32).reshape(-1, 2)
    flat = np.concatenate(sides).astype(np.uint8)
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text) if text_bytes is None else text_bytes]], np.int64))
    d_items, d_work, d_sides = be.upload(items), be.upload(work), be.upload(flat)
    d_flags, d_tiles = be.empty(int(W.sum())), be.empty(8 * int(tiles.sum()))
    d_out, d_widths, d_status = be.full(need + pad, POISON), be.full(16 * n, POISON), be.full(4 * n, POISON)
    be.call("mprg_tree_split", be.ptr(d_bufs), 1, be.ptr(d_items), n, be.ptr(d_work), len(work), be.ptr(d_sides),
            len(flat) if sides_bytes is None else sides_bytes, be.ptr(d_flags), int(W.sum()) if n_cols is None else n_cols, be.ptr(d_tiles),
            int(tiles.sum()) if n_tiles is None else n_tiles, be.ptr(d_out), need if out_bytes is None else out_bytes, be.ptr(d_widths),
            be.ptr(d_status), be.stream)
    return (be.download(d_status, np.int32, n).tolist(), be.download(d_widths, np.int64, 2 * n).reshape(-1, 2),
            be.download(d_out, np.uint8, need + pad), items)


def check_split(be):
    """Every case of split_cases in one call: both texts, their widths, and nothing written behind R_Y W_Y + R_X W_X bytes."""
    check_split_cases()
    cases = split_cases()
    status, widths, out, items = _split(be, [t for t, _, _ in cases], [s for _, s, _ in cases])
    assert status == [0] * len(cases)
    dropped = 0
    for (t, side, what), (wy, wx), it in zip(cases, widths.tolist(), items.tolist()):
        Y, X = split_ref(t, side)
        assert (wy, wx) == (Y.shape[1], X.shape[1]), (t.shape, what)
        o, used = it[5], Y.size + X.size
        assert (out[o:o + Y.size] == Y.reshape(-1)).all() and (out[o + Y.size:o + used] == X.reshape(-1)).all(), (t.shape, what)
        assert (out[o + used:o + t.size] == POISON).all(), (t.shape, what)
        dropped += t.size - used
        if what == "all":
            assert wy == t.shape[1]
        if what == "tile" and t.shape[1] >= 512:
            assert wy <= t.shape[1] - 256
    assert dropped > 100_000 and (out[-64:] == POISON).all()
    # through the host's wrapper: the same texts
    texts = np.array([[0, it[1], it[2], it[3]] for it in items.tolist()], np.int64)
    text = np.concatenate([t.reshape(-1) for t, _, _ in cases])
    d_text = be.upload(text)
    d_out, _, ooff, w2 = sa.tree_split(be, be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64)), 1, texts, [s for _, s, _ in cases])
    got = be.download(d_out, np.uint8, len(text))
    assert (w2 == widths).all() and all((got[o:o + wy * (s == 0).sum() + wx * (s == 1).sum()] == out[o:o + wy * (s == 0).sum() + wx * (s == 1).sum()]).all()
                                        for o, (wy, wx), (_, s, _) in zip(ooff.tolist(), widths.tolist(), cases))


def check_split_statuses(be):
    """A refused item between two good ones: its status, no widths, no output; the good ones are what they are alone."""
    t = pc.codes(["AC-TA", "A-GTA", "--GT-", "AC---"])                # (either side drops one column: 16 of an item's 20 output bytes)
    side = np.array([0, 1, 1, 0], np.uint8)
    texts, sides = [t, t, t], [side, side, side]
    base = _split(be, texts, sides)
    assert base[0] == [0, 0, 0] and base[1].tolist() == [[4, 4]] * 3
    Y, X = split_ref(t, side)
    good = np.concatenate([Y.reshape(-1), X.reshape(-1)])
    blank = np.full(2, POISON, np.uint8).repeat(8).view(np.int64).tolist()

    def refused(code, field=None, value=None, sides2=None, **kw):
        items = base[3].copy()
        if field is not None:
            items[1, field] = value
        status, widths, out, _ = _split(be, texts, sides if sides2 is None else [side, sides2, side], items=items, **kw)
        assert status == [0, code, 0], (field, value, kw)
        assert widths.tolist() == [[4, 4], blank, [4, 4]], (field, value, kw)
        assert (out[:16] == good).all() and (out[40:56] == good).all() and (out[16:40] == POISON).all() and (out[56:] == POISON).all(), (field, value, kw)
    refused(1, 0, 1)                                                  # no such buffer
    refused(1, 0, -1)
    refused(1, 1, 41)                                                 # the text ends one byte outside
    refused(1, 1, -1)
    refused(1, 2, 1)                                                  # a single row has no two sides
    refused(1, 3, 0)
    refused(1, 4, 9)                                                  # the side bytes end outside
    refused(1, 4, -1)
    refused(1, 6, 11)                                                 # the flags end outside
    refused(1, 6, -1)
    refused(1, 7, 5)                                                  # the tile entries end outside
    refused(1, 7, -1)
    refused(1, sides2=np.array([0, 2, 1, 0], np.uint8))               # a side byte above 1
    refused(1, sides2=np.array([0, 0, 0, 0], np.uint8))               # a side without rows
    refused(1, sides2=np.array([1, 1, 1, 1], np.uint8))
    refused(3, 5, 45)                                                 # the output ends one byte outside
    refused(3, 5, -1)
    refused(3, 5, 61)
    # a side without a kept column: Y's only row is all '-'
    t2 = pc.codes(["-----", "A-GTA", "--GT-", "ACG--"])
    status, widths, out, _ = _split(be, [t, t2, t], [side, np.array([0, 1, 1, 1], np.uint8), side])
    assert status == [0, 1, 0] and widths.tolist() == [[4, 4], blank, [4, 4]] and (out[16:40] == POISON).all()
    # the buffers of the whole call one short: the last item is the one that does not fit
    for kw in (dict(text_bytes=59), dict(sides_bytes=11), dict(n_cols=14), dict(n_tiles=5)):
        status, widths, out, _ = _split(be, texts, sides, **kw)
        assert status == [0, 0, 1] and widths.tolist() == [[4, 4], [4, 4], blank] and (out[36:] == POISON).all(), kw
    # an empty work table: no counts to split from, every item refused
    status, widths, out, _ = _split(be, texts, sides, work=[])
    assert status == [1, 1, 1] and widths.tolist() == [blank] * 3 and (out == POISON).all()
    status, widths, out, _ = _split(be, texts, sides, out_bytes=47)
    assert status == [0, 0, 3] and widths.tolist() == [[4, 4], [4, 4], blank] and (out[36:] == POISON).all()


# ---- mprg_tree_objective
def _objective(be, texts, weights, empty, items=None, weights_words=None, work=None):
    """mprg_tree_objective on these texts (R x W matrices of cell codes): (status words, S per item)."""
    n = len(texts)
    text = np.concatenate([t.reshape(-1) for t in texts])
    R, W = np.array([t.shape[0] for t in texts], np.int64), np.array([t.shape[1] for t in texts], np.int64)
    if items is None:
        items = np.stack([np.zeros(n, np.int64), sa.exclusive_sum(R * W), R, W, sa.exclusive_sum(R), [int(np.sum(w)) for w in weights],
                          np.asarray(empty, np.int64)], 1)
    items = np.array(items, np.int64)
    work = sa._tile_work(W) if work is None else np.array(work, np.int32)
    flat = np.concatenate(weights).astype(np.int32)
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64))
    d_items, d_work, d_weights = be.upload(items), be.upload(work), be.upload(flat)
    d_sums, d_status = be.zeros(8 * n), be.full(4 * len(work), POISON)
    be.call("mprg_tree_objective", be.ptr(d_bufs), 1, be.ptr(d_items), n, be.ptr(d_work), len(work), be.ptr(d_weights),
            len(flat) if weights_words is None else weights_words, be.ptr(d_sums), be.ptr(d_status), be.stream)
    return be.download(d_status, np.int32, len(work)).tolist(), be.download(d_sums, np.int64, n).tolist(), items


def _ascii(t):
    return ["".join("ACGT-RYKMSWN"[c] for c in row) for row in t]


@functools.lru_cache(maxsize=None)
def objective_texts():
    """Texts over all twelve codes without an all-gap column: 1, 2, 3 and 7 rows at the widths around the tile; from three rows on
    the second row is all '-'."""
    rng = np.random.default_rng(43)
    out = []
    for R in (1, 2, 3, 7):
        for W in (1, 255, 256, 257, 600):
            t = pc.related_codes(rng, W, rng.integers(0, 4, W), R, W)
            if R >= 3:
                t[1] = GAP
                empty = (t == GAP).all(0)
                t[0, empty] = 2
            out.append(t)
    return out


def check_objective(be):
    texts = objective_texts()
    assert {t.shape for t in texts} == {(R, W) for R in (1, 2, 3, 7) for W in (1, 255, 256, 257, 600)}
    assert all(not (t == GAP).all(0).any() for t in texts) and sum(bool((t == GAP).all(1).any()) for t in texts) >= 10
    ones = [np.ones(len(t), np.int64) for t in texts]
    # weights 1, no empty record: mprg_refine_counts' S of the same MSA, and the plain-Python S
    status, plain, _ = _objective(be, texts, ones, np.zeros(len(texts)))
    assert not any(status)
    msas = [_ascii(t) for t in texts]
    d_text, nbytes, toff, R, W = rc.upload_msas(be, msas)
    assert plain == sa.refine_counts(be, d_text, nbytes, toff, R, W)[4].tolist() == [rr.objective(m) for m in msas]
    # weights 1 to 5, then two empty records as well: the expanded text's S (by this entry, and in plain Python)
    rng = np.random.default_rng(47)
    weights = [rng.integers(1, 6, len(t)) for t in texts]
    for E in (0, 2):
        status, got, _ = _objective(be, texts, weights, np.full(len(texts), E))
        expanded = [np.concatenate([np.repeat(t, w, axis=0), np.full((E, t.shape[1]), GAP, np.uint8)]) for t, w in zip(texts, weights)]
        status2, want, _ = _objective(be, expanded, [np.ones(len(t), np.int64) for t in expanded], np.zeros(len(texts)))
        assert not any(status) and not any(status2) and got == want
        assert got == [rr.objective(_ascii(t)) for t in expanded] == [tr.objective(m, w.tolist(), E) for m, w in zip(msas, weights)]
    assert len(set(plain)) > 15 and min(plain) < 0 < max(plain)
    # through the host's wrapper
    text = np.concatenate([t.reshape(-1) for t in texts])
    d_text = be.upload(text)
    tab = np.stack([np.zeros(len(texts), np.int64), sa.exclusive_sum([t.size for t in texts]), [len(t) for t in texts], [t.shape[1] for t in texts]], 1)
    assert sa.tree_objective(be, be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64)), 1, tab, weights, np.full(len(texts), 2)).tolist() == got


def check_objective_statuses(be):
    t = pc.codes(["ACGTA", "AC-TA", "ACGTN"])
    w = np.array([2, 1, 3])
    status, S, good = _objective(be, [t], [w], [1])
    assert status == [0] and S == [tr.objective(_ascii(t), w.tolist(), 1)]

    def refused(field=None, value=None, **kw):
        items = good.copy()
        if field is not None:
            items[0, field] = value
        assert _objective(be, [t], [kw.pop("w", w)], [1], items=items, **kw)[:2] == ([1], [0]), (field, value, kw)
    refused(0, 1)                                                    # no such buffer
    refused(1, 1)                                                    # the text ends one byte outside
    refused(1, -1)
    refused(2, 0)
    refused(3, 0)
    refused(4, 1)                                                    # the weights end outside
    refused(4, -1)
    refused(weights_words=2)
    refused(5, 5)                                                    # the stated sum is not the sum
    refused(5, 7)
    refused(w=np.array([2, 0, 4]))                                   # a weight below 1, the sum as stated
    refused(w=np.array([3, -1, 4]))
    refused(6, -1)
    refused(6, (1 << 20) - 5)                                        # sum + E above 2^20
    refused(work=[[1, 0]])
    refused(work=[[-1, 0]])
    refused(work=[[0, 1]])
    refused(work=[[0, -1]])
    items = good.copy()
    items[0, 6] = (1 << 20) - 6                                      # sum + E = 2^20: (sum + E)^2 W = 5 * 2^40 still fits
    assert _objective(be, [t], [w], [1], items=items)[:2] == ([0], [tr.objective(_ascii(t), w.tolist(), (1 << 20) - 6)])


# ---- whole MSAs
def msa_loci():
    return sr.edge_loci() + rr.special_loci() + pr.table_loci()


@functools.lru_cache(maxsize=None)
def msa_spec(passes):
    return [tr.progressive(l, passes) for l in msa_loci()]


def check_counts():
    """What the issue's table promises of the 18 table loci under two passes: 8 or more accept a step, one or more accept none."""
    table = msa_spec(2)[-18:]
    assert sum(1 for _, i in table if i[1]) >= 8 and sum(1 for _, i in table if not i[1]) >= 1
    assert any(i[0] == 0 for _, i in msa_spec(2)) and any(i[0] > 0 and i[1] == 0 for _, i in msa_spec(2))
    assert any(a[1] < b[1] for (_, a), (_, b) in zip(msa_spec(1), msa_spec(2)))          # a second pass that accepts a step


def invariants(l, rows, progressive_rows=None, info=None):
    cc.invariants(l, rows, equal_rows=False)
    if info is not None:
        assert info[4] >= info[3] and (info[4] > info[3]) == (info[1] > 0) and info[0] >= info[1] + info[2]
        if not info[1] and progressive_rows is not None:
            assert rows == progressive_rows


def check_msas(be, passes, **kw):
    """Rows and tuples equal the reference, exactly; the spec's promises on the result."""
    loci, info, timings = msa_loci(), [], {}
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, refine_tree=passes, tree_refinement=info, timings=timings, **kw)
    plain = pc.msa_spec()
    for k, (l, m, got, (rows, want)) in enumerate(zip(loci, msas, info, msa_spec(passes))):
        assert m.rows_as_strings() == rows, l
        assert got == want, l
        assert m.descriptions == [t for t, _ in pc.records(l)]
        if l in pc.msa_loci():
            invariants(l, rows, plain[pc.msa_loci().index(l)][0], got)
    assert timings["tree_refine_s"] > 0 and timings["tree_refine_steps"] == sum(i[0] for i in info)
    assert timings["tree_refine_accepted"] == sum(i[1] for i in info) > 0 and timings["tree_refine_skipped"] == 0
    assert timings["tree_refine_above_cap"] == 0 and timings["tree_refine_loci"] == sum(1 for i in info if i[0])
    return msas


def check_same_bytes(be, **kw):
    """Two passes under another flag: the reference's rows again."""
    msas = sa.star_msas(be, [pc.records(l) for l in msa_loci()], progressive=True, refine_tree=2, **kw)
    assert [m.rows_as_strings() for m in msas] == [rows for rows, _ in msa_spec(2)]


@functools.lru_cache(maxsize=None)
def collapse_spec():
    return [tr.progressive(l, 2, collapse=True) for l in cc.loci()]


def check_collapse(be, **kw):
    """collapse_common's loci: the reference on the expanded meaning, equal rows for equal sequences, a step accepted somewhere."""
    info = []
    msas = sa.star_msas(be, [pc.records(l) for l in cc.loci()], progressive=True, collapse=True, refine_tree=2, tree_refinement=info, **kw)
    for l, m, got, (rows, want) in zip(cc.loci(), msas, info, collapse_spec()):
        assert m.rows_as_strings() == rows and got == want, l
        cc.invariants(l, rows)
    assert any(i[1] for i in info) and any(i[0] and not i[1] for i in info)
    # a locus without duplicates: the bytes of the run without collapse
    assert collapse_spec()[-1] == tr.progressive(cc.loci()[-1], 2)


def check_cap(be):
    """With the cap at 8 leaves the 12-row and 18-row loci keep their progressive bytes and are reported; the others are refined."""
    loci, info, timings = msa_loci(), [], {}
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, refine_tree=2, tree_refinement=info, timings=timings,
                        tree_refine_max_leaves=8)
    above = 0
    for l, m, got, (rows, want) in zip(loci, msas, info, msa_spec(2)):
        if sum(1 for s in l if sr.normalise(s)) > 8:
            above += 1
            assert m.rows_as_strings() == pr.progressive_rows(l) and got == (0, 0, 0, want[3], want[3])
        else:
            assert m.rows_as_strings() == rows and got == want
    assert above == timings["tree_refine_above_cap"] == 18
    assert tr.progressive(loci[-1], 2, max_leaves=8) == (pr.progressive_rows(loci[-1]), info[-1])


def flipped_loci():
    return pc.flipped_loci() + rr.special_loci()


@functools.lru_cache(maxsize=None)
def flipped_spec():
    """Per locus (titles, the tree stage's tuple, refine_ref's (rows, rounds accepted, S trail)) of strand_ref -> treerefine_ref ->
    refine_ref."""
    out = []
    for l in flipped_loci():
        rev, _, ori = st.oriented(l)
        rows, info = tr.progressive(ori, 1)
        out.append((st.titles(pc.records(l), rev), info, rr.refine_rows(rows, 2)))
    return out


def check_compositions(be, **kw):
    recs = [pc.records(l) for l in flipped_loci()]
    tree, leave = [], []
    msas = sa.star_msas(be, recs, progressive=True, adjust_direction=True, refine_tree=1, tree_refinement=tree, refine=2, refinement=leave, **kw)
    for m, t, r, (titles, info, (rows, acc, trail)) in zip(msas, tree, leave, flipped_spec()):
        assert m.descriptions == titles and m.rows_as_strings() == rows
        assert t == info and r == (acc, trail[0], trail[-1])
        assert r[1] == t[4]                                          # the leave-one-out stage starts from the S the tree stage ended with
    assert any(t[1] for t in tree) and any(r[0] for r in leave) and sum(t.startswith(sa.REVERSED_PREFIX) for m in msas for t in m.descriptions) >= 20


class Calls:
    """A backend that notes the entry points called."""

    def __init__(self, be):
        self.be, self.names = be, []

    def __getattr__(self, key):
        return getattr(self.be, key)

    def call(self, name, *args, **kw):
        self.names.append(name)
        return self.be.call(name, *args, **kw)


def check_flag_off(be):
    """refine_tree=None: prog_ref's rows, neither new entry launched; with it on both are."""
    loci = pr.table_loci()[5:8] + rr.special_loci()
    for kw, used in ((dict(refine_tree=None), False), ({}, False), (dict(refine_tree=1), True)):
        wrapped = Calls(be)
        msas = sa.star_msas(wrapped, [pc.records(l) for l in loci], progressive=True, **kw)
        assert ("mprg_tree_split" in wrapped.names) == ("mprg_tree_objective" in wrapped.names) == used and "mprg_prog_rows" in wrapped.names
        if not used:
            assert [m.rows_as_strings() for m in msas] == [pr.progressive_rows(l) for l in loci]
