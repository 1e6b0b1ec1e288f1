"""What the emulated and the GPU tests of `from_msa --unaligned --progressive --position-gaps` share (the spec: star_align.py,
"Position gaps"; its plain-Python statement: tests/posgap_ref.py): the profile pairs of the DP check with their new reference, the
merges that open a run where 704 (R_X - g) is no multiple of R_X, the seventh plane, the banded entry, the widths entry, the two
passes, the closedness property, whole MSAs and their compositions, the four diverged loci of the finding, the status codes of the
new entries and the command line's inputs."""
import functools
import random
from collections import Counter

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from make_prg_amd.utils.synthetic import diverged_locus
from tests import collapse_ref as cr
from tests import compare_ref as cmp
from tests import posgap_ref as pg
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import progband_common as pbc
from tests import progband_ref as pbr
from tests import refine_ref as rr
from tests import star_ref as sr

W0 = pbc.W0


# ---- 2. the DP against the reference
def _gappy_first(rng, R, W):
    """random_profiles whose first column is mostly gaps (one residue among R rows where R > 1)."""
    rows = [list(r) for r in pr.random_profiles(rng, R, W, 0.2, amb=0.05)]
    for r in range(R):
        rows[r][0] = "-" if r else rows[r][0] if rows[r][0] != "-" else "A"
    return tuple("".join(r) for r in rows)


@functools.lru_cache(maxsize=None)
def dp_cases():
    """((X, Y), posgap_ref's (ops, score)): prog_common.dp_cases' pairs, then pairs whose first column on X's side, on Y's side and
    on both is one residue among gaps (the boundary uses Oc[0] and Ox[0]), across a strip and a ring block."""
    out = [(xy, pg.align_profiles_np(*xy)) for xy, _ in pc.dp_cases()]
    rng = random.Random(5)
    for k, (rx, wx, ry, wy) in enumerate(((3, 5, 7, 9), (7, 70, 3, 64), (2, 65, 7, 130), (7, 1, 3, 1), (3, 129, 2, 40), (7, 30, 7, 200))):
        X = _gappy_first(rng, rx, wx) if k % 3 != 1 else tuple(pr.random_profiles(rng, rx, wx, 0.2))
        Y = _gappy_first(rng, ry, wy) if k % 3 != 0 else tuple(pr.random_profiles(rng, ry, wy, 0.2))
        out.append(((X, Y), pg.align_profiles_np(X, Y)))
    return out


def check_dp(be, **kw):
    cases = dp_cases()
    fixed = [w for _, w in pc.dp_cases()]
    assert sum(a[1] != b for a, b in zip(cases, fixed)) >= 10            # the new opens change results, or nothing is tested
    Oc0 = [pg.opens(*xy)[0][0] for xy, _ in cases]
    Ox0 = [pg.opens(*xy)[1][0] for xy, _ in cases]
    assert sum(-704 < v < 0 for v in Oc0) >= 4 and sum(-704 < v < 0 for v in Ox0) >= 4
    got = sa.merge_profiles(be, [(pc.codes(x), pc.codes(y)) for (x, y), _ in cases], position_gaps=True, **kw)
    for ((x, y), want), (ops, score) in zip(cases, got):
        assert (ops.decode(), score) == want, (len(x), len(x[0]), len(y), len(y[0]))


def check_gap_free(be):
    """Neither side has a '-': Oc = Ox = -704, so ops and score are mprg_align_profile_pairs' (and prog_ref's); every leaf-leaf
    merge is such a pair."""
    rng = random.Random(6)
    cases = []
    for k, (wx, wy) in enumerate(((1, 1), (64, 65), (65, 128), (129, 127), (200, 300), (30, 3))):
        X = tuple(pr.random_profiles(rng, pc.ROWS[k % 4], wx, 0.0, amb=0.1))
        Y = tuple(pr.random_profiles(rng, pc.ROWS[(k + 1) % 4], wy, 0.0, amb=0.1))
        assert "-" not in "".join(X + Y)
        cases.append((X, Y))
    pairs = [(pc.codes(x), pc.codes(y)) for x, y in cases]
    got = sa.merge_profiles(be, pairs, position_gaps=True)
    assert got == sa.merge_profiles(be, pairs)
    assert [(o.decode(), s) for o, s in got] == [pr.align_profiles_np(x, y) for x, y in cases]


TALL_ROWS = (8, 255, 257, 4096)


@functools.lru_cache(maxsize=None)
def tall_cases():
    """prog_common.tall_dp_cases' related sides of 8, 255, 257 and 4 096 rows (on X's side), with posgap_ref's result."""
    picked = [xy for xy, _ in pc.tall_dp_cases()[:len(pc.TALL)] if xy[0].shape[0] in TALL_ROWS]
    assert {x.shape[0] for x, _ in picked} == set(TALL_ROWS)
    return [(xy, pg.align_profiles_np(*xy)) for xy in picked]


@functools.lru_cache(maxsize=None)
def divisor_cases():
    """Merges that open a run of I ops at an X column with 704 (R_X - g) not a multiple of R_X, for every R_X of
    prog_common.DIVISORS: X has a column of a residues among gaps (a = 1, R_X // 3, R_X - 1) beside an all-A column, Y is one all-A
    column (2 x 1 merges: the partial column first, so Ox[0] opens column 0, or second, so the cell opens it), or X has a partial
    column between two all-A columns against Y's two (3 x 2).  ((X, Y) as matrices of cell codes, posgap_ref's result)."""
    out = []
    Y1, Y2 = np.zeros((9, 1), np.uint8), np.zeros((9, 2), np.uint8)
    for R in pc.DIVISORS:
        for a in (1, R // 3, R - 1):
            assert (704 * a) % R, (R, a)
            part = np.concatenate([np.zeros(a, np.uint8), np.full(R - a, 4, np.uint8)]).reshape(R, 1)
            full = np.zeros((R, 1), np.uint8)
            for X, Y, ops in ((np.hstack([part, full]), Y1, "IM"), (np.hstack([full, part]), Y1, "MI"),
                              (np.hstack([full, part, full]), Y2, "MIM")):
                want = pg.align_profiles_np(X, Y)
                assert want[0] == ops and want[1] == 1280 * len(Y[0]) - (704 * a) // R - (640 * a) // R, (R, a, want)
                out.append(((X, Y), want))
    return out


def check_tall_and_divisors(be, **kw):
    cases = tall_cases() + divisor_cases()
    got = sa.merge_profiles(be, [xy for xy, _ in cases], position_gaps=True, **kw)
    for ((x, y), want), (ops, score) in zip(cases, got):
        assert (ops.decode(), score) == want, (x.shape, y.shape)


# ---- 2. the seventh plane
def _columns(be, mats, kinds, weights=None, posgap=True):
    """Every (text, kind) through mprg_prog_columns(_weighted)(_posgap): (the planes per item, nothing written behind them)."""
    off = sa.exclusive_sum([m.size for m in mats])
    text = np.concatenate([np.ascontiguousarray(m, np.uint8).reshape(-1) for m in mats])
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64))
    items, work, words = [], [], 0
    for kind in kinds:
        for k, (m, o) in enumerate(zip(mats, off.tolist())):
            work += [[len(items), tile] for tile in range(-(-m.shape[1] // 256))]
            items.append([0, o, *m.shape, kind, words] + ([0, 0] if weights is not None else []))
            words += (6 if kind == 0 else 7) * m.shape[1]
    items = np.array(items, np.int64)
    d_cols, d_status = be.full(4 * words + 64, 0x5C), be.full(4 * len(work), 0x5C)
    name = "mprg_prog_columns" + ("_weighted" if weights is not None else "") + ("_posgap" if posgap else "")
    d_work = be.upload(np.array(work, np.int32))
    if weights is None:
        d_items = be.upload(items)
        be.call(name, be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work), be.ptr(d_cols), words, be.ptr(d_status),
                be.stream)
    else:
        per = [np.asarray(w, np.int64) for _ in kinds for w in weights]
        items[:, 6], items[:, 7] = sa.exclusive_sum([len(w) for w in per]), [int(w.sum()) for w in per]
        flat = np.concatenate(per).astype(np.int32)
        d_items, d_weights = be.upload(items), be.upload(flat)
        be.call(name, be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work), be.ptr(d_weights), len(flat),
                be.ptr(d_cols), words, be.ptr(d_status), be.stream)
    assert not be.download(d_status, np.int32, len(work)).any()
    assert (be.download(d_cols, np.uint8, 4 * words + 64)[4 * words:] == 0x5C).all()
    cols = be.download(d_cols, np.int32, words)
    return [cols[o:o + (6 if kind == 0 else 7) * W].reshape(-1, W) for _, _, _, W, kind, o, *_ in items.tolist()]


@functools.lru_cache(maxsize=None)
def plane_mats():
    """prog_common.plane_texts as matrices, then one text each of 255, 256, 257, 65 537 and 2^20 rows (check_tall_columns')."""
    rng = np.random.default_rng(8)
    mats = [pc.codes(t) for t in pc.plane_texts()]
    for R, W in ((255, 300), (256, 64), (257, 257), (65537, 40), (pc.TALL_MAX, 8)):
        t = pc.related_codes(rng, W, rng.integers(0, 4, W), R, W)
        t[:, 0], t[:, 1], t[:, 2], t[:, 3] = 0, 4, 11, 4                 # all A, all '-', all N, one C among '-'
        t[R // 2, 3] = 1
        mats.append(t)
    return mats


def check_planes(be):
    """Kind 2's seventh plane is the NumPy statement of Oc and its first six are kind 0's; kinds 0 and 1 through the new entry are
    byte-equal to mprg_prog_columns'; with weights 1..5 the planes are those of the text with row r written w_r times."""
    mats = plane_mats()
    n = len(mats)
    new = _columns(be, mats, (0, 1, 2))
    old = _columns(be, mats, (0, 1), posgap=False)
    assert all((a == b).all() for a, b in zip(new[:2 * n], old))
    seen = set()
    for m, p0, p2 in zip(mats, new[:n], new[2 * n:]):
        Oc = pg.tables(m, m)[3]
        assert p2.shape[0] == 7 and (p2[:6] == p0).all() and (p2[6] == Oc).all(), m.shape
        seen |= set(Oc.tolist())
    assert {0, -704} <= seen and len(seen) > 20 and any((704 * v) % 7 for v in range(7))
    small = mats[:len(pc.plane_texts())]
    rng = np.random.default_rng(29)
    weights = [rng.integers(1, 6, len(m)) for m in small]
    got = _columns(be, small, (0, 1, 2), weights)
    want = _columns(be, [np.repeat(m, w, axis=0) for m, w in zip(small, weights)], (0, 1, 2))
    assert all((a == b).all() for a, b in zip(got, want))
    for m, w, p2 in zip(small, weights, got[2 * len(small):]):
        assert (p2[6] == pg.tables(m, m, w, w)[3]).all()
    ones = _columns(be, small, (0, 1, 2), [np.ones(len(m), np.int64) for m in small])
    assert all((a == b).all() for a, b in zip(ones, [new[k * n + i] for k in range(3) for i in range(len(small))]))
    old_w = _columns(be, small, (0, 1), weights, posgap=False)
    assert all((a == b).all() for a, b in zip(got[:2 * len(small)], old_w))


# ---- 3. band: the two entries on explicit tables
class Tables:
    """mprg_prog_columns_posgap over (X, Y) pairs of row-string tuples, Y as kind 2, as _prog_pairs lays them out."""

    def __init__(self, be, pairs):
        self.be, self.n = be, len(pairs)
        mats = [pc.codes(m) for xy in pairs for m in xy]
        off = sa.exclusive_sum([m.size for m in mats])
        text = np.concatenate([m.reshape(-1) for m in mats])
        self.d_text = be.upload(text)
        d_bufs = be.upload(np.array([[be.ptr(self.d_text), len(text)]], np.int64))
        n = self.n
        X = np.array([[0, off[2 * k], *mats[2 * k].shape] for k in range(n)], np.int64).reshape(-1, 4)
        Y = np.array([[0, off[2 * k + 1], *mats[2 * k + 1].shape] for k in range(n)], np.int64).reshape(-1, 4)
        self.WX, self.WY, self.RX = X[:, 3], Y[:, 3], X[:, 2]
        self.ycol = sa.exclusive_sum(7 * self.WY + 7 * self.WX)
        self.xcol = self.ycol + 7 * self.WY
        self.words = int((7 * self.WY + 7 * self.WX).sum())
        items = np.zeros((2 * n, sa.PG_ITEM_FIELDS), np.int64)
        items[:n, :4], items[:n, 4], items[:n, 5] = Y, 2, self.ycol
        items[n:, :4], items[n:, 4], items[n:, 5] = X, 1, self.xcol
        work = sa._tile_work(items[:, 3])
        self.d_cols, d_status = be.empty(4 * self.words), be.empty(4 * len(work))
        d_items, d_work = be.upload(items), be.upload(work)
        be.call("mprg_prog_columns_posgap", be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work),
                be.ptr(self.d_cols), self.words, be.ptr(d_status), be.stream)
        assert not be.download(d_status, np.int32, len(work)).any()
        self.d_leaves = be.upload(np.stack([np.zeros(n, np.int64), Y[:, 2], self.WY, self.ycol], 1).astype(np.int64))
        self.ops_off = sa.exclusive_sum(self.WX + self.WY)

    def pair_rows(self, idx, dlo, dhi, ws_off=None):
        idx = np.asarray(idx, np.int64)
        z = np.zeros(len(idx), np.int64)
        return np.stack([idx, self.xcol[idx], self.WX[idx], z if ws_off is None else ws_off, self.ops_off[idx], self.RX[idx],
                         np.asarray(dlo, np.int64), np.asarray(dhi, np.int64)], 1).astype(np.int64)

    def _run(self, call, need, rows):
        be, n = self.be, self.n
        ops_bytes = int((self.WX + self.WY).sum())
        d_ws, d_ops, d_out = be.empty(4 * int(need.sum())), be.empty(ops_bytes), be.empty(12 * n)
        d_pairs = be.upload(rows)
        be.call(call, be.ptr(self.d_cols), be.ptr(self.d_leaves), n, be.ptr(self.d_cols), self.words, be.ptr(d_pairs), n,
                be.ptr(d_ws), int(need.sum()), be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
        res = be.download(d_out, np.int32, 3 * n).reshape(-1, 3)
        assert not res[:, 0].any(), res[:, 0]
        ops = be.download(d_ops, np.uint8, ops_bytes)
        return [(ops[o:o + k][::-1].tobytes().decode(), int(s)) for o, k, s in zip(self.ops_off, res[:, 2], res[:, 1])]

    def banded(self, bands):
        """Every pair over its (dlo, dhi), one launch: [(ops forward, score)]."""
        dlo, dhi = np.array([b[0] for b in bands], np.int64), np.array([b[1] for b in bands], np.int64)
        need = pa.band_workspace_words(self.WX, self.WY, np.maximum(dlo, -self.WX), np.minimum(dhi, self.WY))
        return self._run("mprg_align_profile_pairs_posgap_banded", need, self.pair_rows(np.arange(self.n), dlo, dhi, sa.exclusive_sum(need)))

    def full(self):
        need = pa.workspace_words_v(self.WX, self.WY)
        z = np.zeros(self.n)
        return self._run("mprg_align_profile_pairs_posgap", need,
                         self.pair_rows(np.arange(self.n), z, z, sa.exclusive_sum(need))[:, :sa.PG_PAIR_FIELDS])

    def widths(self, idx, S0):
        """mprg_prog_band_widths_posgap for the pairs idx (repeats allowed) with the pass-1 scores S0: (SB, w*) per entry."""
        be, m = self.be, len(idx)
        out = np.zeros((m, 3), np.int32)
        out[:, 1] = S0
        d_bounds, d_status = be.empty(16 * m), be.empty(4 * m)
        z = np.zeros(m, np.int64)
        d_pairs, d_out = be.upload(self.pair_rows(idx, z, z)), be.upload(out)
        be.call("mprg_prog_band_widths_posgap", be.ptr(self.d_cols), be.ptr(self.d_leaves), self.n, be.ptr(self.d_cols), self.words,
                be.ptr(d_pairs), m, be.ptr(d_out), be.ptr(d_bounds), be.ptr(d_status), be.stream)
        assert not be.download(d_status, np.int32, m).any()
        return be.download(d_bounds, np.int64, 2 * m).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """progband_common.kernel_cases' pairs and bands (random bands over dp_cases' shapes, then one pair per width of its WIDTHS)
    with posgap_ref's banded result and the full DP's score."""
    return [(xy, b, pg.align_profiles_banded_np(*xy, *b), pg.align_profiles_np(*xy)[1]) for xy, b, _, _ in pbc.kernel_cases()]


def check_kernel(be):
    cases = kernel_cases()
    assert sum(want[1] < full for _, _, want, full in cases) >= 8 and any(want[1] == full for _, _, want, full in cases)
    assert sum(want != old for (_, _, want, _), (_, _, old, _) in zip(cases, pbc.kernel_cases())) >= 10
    t = Tables(be, [xy for xy, _, _, _ in cases])
    for (xy, b, want, _), g in zip(cases, t.banded([b for _, b, _, _ in cases])):
        assert g == want, (len(xy[0][0]), len(xy[1][0]), len(xy[0]), len(xy[1]), b)
    for (xy, _, _, full), g in zip(cases, t.full()):                      # the full entry over the same tables
        assert g[1] == full


def check_widths(be):
    cases = pbc.width_cases()
    idx, S0, want = [], [], []
    weaker = 0
    for k, (X, Y) in enumerate(cases):
        n, C = len(X[0]), len(Y[0])
        b = pg.bounds(X, Y)
        assert -704 <= b[3] <= 0 and -704 <= b[4] <= 0
        weaker += b[3] + b[4] > -1408
        top = min(n, C)
        scores = {b[0] + 5000, -10 ** 8}
        for w in sorted({0, 1, 2, 3, top // 3, top // 2, top - 2, top - 1, top} & set(range(top + 1))):
            u = pg.U(*b, n, C, w)
            assert u == pbr.U(*b[:3], n, C, w) + 1408 + b[3] + b[4]
            scores |= {u - 1, u, u + 1}                         # at, one below and one above the threshold
        for s in sorted(scores):
            idx.append(k)
            S0.append(s)
            want.append((b[0], pg.wstar(*b, n, C, s)))
    assert weaker >= 4 and len({w for _, w in want}) >= 30
    got = Tables(be, cases).widths(idx, S0)
    for k, s, w, g in zip(idx, S0, want, got.tolist()):
        assert tuple(g) == w, (k, s)
    got = Tables(be, [(("A",), ("ACGT", "A-GT"))]).widths([0, 0], [-10 ** 6, 10 ** 6])   # n = 1: ox is Ox[0]
    b = pg.bounds(("A",), ("ACGT", "A-GT"))
    assert got.tolist() == [[b[0], pg.wstar(*b, 1, 4, s)] for s in (-10 ** 6, 10 ** 6)]


@functools.lru_cache(maxsize=None)
def related_cases():
    return [(xy, pg.align_profiles_np(*xy)) for xy, _ in pbc.related_cases()]


@functools.lru_cache(maxsize=None)
def two_pass_spec():
    """The reference's (kind, cells) per merge of dp_cases + related_cases with W0 and the new U, and the merges' (n, C)."""
    cases = dp_cases() + related_cases()
    res = [pg.two_pass(X, Y, W0) for (X, Y), _ in cases]
    assert [r for r, _, _ in res] == [w for _, w in cases]      # the reference's own two passes give the unbanded result
    return [(k, c) for _, k, c in res], [(len(X[0]), len(Y[0])) for (X, Y), _ in cases]


def check_two_pass_merges(be):
    cases = dp_cases() + related_cases()
    log, sizes = two_pass_spec()
    kinds = Counter(k for k, _ in log)
    assert kinds["first"] >= 2 and kinds["second"] >= 2 and kinds["full"] >= 2, kinds
    pairs = [(pc.codes(x), pc.codes(y)) for (x, y), _ in cases]
    small = 4 * int(max(pa.workspace_words(n, C) for n, C in sizes))         # the largest full DP alone: every pass in several launches
    for budget in (pa.DEFAULT_BUDGET_BYTES, small):
        counters = {}
        got = sa.merge_profiles(be, pairs, budget_bytes=budget, band=W0, counters=counters, position_gaps=True)
        for ((x, y), want), (ops, score) in zip(cases, got):
            assert (ops.decode(), score) == want, (len(x), len(x[0]), len(y), len(y[0]))
        assert {k: v for k, v in counters.items() if k.startswith("prog_band_")} == pbr.counters(log, sizes)
        assert counters["position_gap_merges"] == len(cases)
    check_dp(be, band=True)                                     # the default w0
    check_tall_and_divisors(be, band=True)


def check_property(be):
    """progband_common.check_property's pairs and bands: whenever the new certificate closes both sides of the band, the banded ops
    and score are the full DP's."""
    rng = random.Random(77)
    cases, bands = [], []
    for k in range(40):
        L = rng.randint(20, 140)
        root = "".join(rng.choice("ACGT") for _ in range(L))
        sub, indel = rng.choice([(0.0, 0.0), (0.02, 0.01), (0.05, 0.04), (0.2, 0.1)])
        rows = pg.progressive_rows([sr.mutate(rng, root, sub, indel) or "A" for _ in range(rng.randint(2, 6))])
        cut = rng.randint(1, len(rows) - 1)
        X, Y = [tuple(pg.progressive_rows([r.replace("-", "") or "A" for r in part])) for part in (rows[:cut], rows[cut:])]
        if k % 5 == 0:
            X = tuple(pr.random_profiles(rng, len(X), len(X[0]), 0.3))
        n, C = len(X[0]), len(Y[0])
        cases.append((X, Y))
        bands.append((min(0, C - n) - rng.choice([0, 1, 3, 8, 20, 200]), max(0, C - n) + rng.choice([0, 1, 3, 8, 20, 200])))
    got = Tables(be, cases).banded(bands)
    n_closed = n_open = n_below = 0
    for (X, Y), b, g in zip(cases, bands, got):
        n, C = len(X[0]), len(Y[0])
        full = pg.align_profiles_np(X, Y)
        assert g[1] <= full[1]
        if all(pg.closed(*pg.bounds(X, Y), n, C, *b, g[1])):
            n_closed += 1
            assert g == full, (n, C, b)
        else:
            n_open += 1
            n_below += g[1] < full[1]
    assert n_closed >= 8 and n_open >= 8 and n_below >= 3, (n_closed, n_open, n_below)


# ---- 4. whole MSAs
@functools.lru_cache(maxsize=None)
def msa_spec():
    return [pg.progressive(l) for l in pc.msa_loci()]


def invariants(l, rows):
    assert [r.replace("-", "") for r in rows] == [sr.normalise(s) for s in l]
    assert not any(all(r[c] == "-" for r in rows) for c in range(len(rows[0]))) or not any(sr.normalise(s) for s in l)


def check_msas(be, **kw):
    loci, info = pc.msa_loci(), []
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, position_gaps=True, progression=info, **kw)
    changed = 0
    for l, m, got, (rows, want), (old, _) in zip(loci, msas, info, msa_spec(), pc.msa_spec()):
        assert m.rows_as_strings() == rows, l
        assert got == want, l
        invariants(l, rows)
        changed += rows != old
    assert changed >= 10
    return msas


def check_same_bytes(be):
    base = [m.rows_as_strings() for m in check_msas(be)]
    for kw in (dict(band=W0), dict(band=True, device_tree=True), dict(device_tree=True, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)):
        assert [m.rows_as_strings() for m in check_msas(be, **kw)] == base, kw


def check_flag_off(be):
    """Without the flag the bytes are prog_ref's, as today (and False is no flag)."""
    loci = pc.msa_loci()
    for kw in (dict(), dict(position_gaps=False)):
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, **kw)
        assert [m.rows_as_strings() for m in msas] == [rows for rows, _ in pc.msa_spec()]


def check_refine_afterwards(be):
    """refine = 2 after the flag: refine_ref (unweighted, the fixed open) on the new rows."""
    loci = pr.table_loci()[:8]
    info = []
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, position_gaps=True, refine=2, refinement=info)
    for l, m, got in zip(loci, msas, info):
        rows, acc, trail = rr.refine_rows(pg.progressive_rows(l), 2)
        assert m.rows_as_strings() == rows and got == (acc, trail[0], trail[-1])
    assert any(a for a, _, _ in info)


def composition_loci():
    """Small loci the composition modules already use: three of collapse_common's with copies, a table locus of each kind, a clade
    locus and weights_common's small ones."""
    from tests import collapse_common as cc
    from tests import weights_common as wc
    t = pr.table_loci()
    return list(cc.loci()[:3]) + [t[0], t[6], t[12], pr.clade_locus(42, 8)] + wc.small_loci()


@functools.lru_cache(maxsize=None)
def composition_spec():
    """Per flag the reference composition's rows of composition_loci, every merge by the new opens (posgap_ref.in_compositions)."""
    from tests import retree_ref as rt
    from tests import treerefine_ref as tf
    from tests import weights_ref as wr
    loci = composition_loci()
    with pg.in_compositions():
        return dict(collapse=[cr.progressive(l)[0] for l in loci], seq_weights=[wr.progressive(l)[0] for l in loci],
                    retree=[rt.progressive(l, 1)[0] for l in loci], refine_tree=[tf.progressive(l, 1)[0] for l in loci])


def check_compositions(be):
    loci = composition_loci()
    spec = composition_spec()
    plain = [pg.progressive_rows(l) for l in loci]
    for key, kw in (("collapse", dict(collapse=True)), ("seq_weights", dict(seq_weights=True)), ("retree", dict(retree=1)),
                    ("refine_tree", dict(refine_tree=1))):
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, position_gaps=True, **kw)
        got = [m.rows_as_strings() for m in msas]
        assert got == spec[key], key
        assert got != plain or key == "collapse", key            # (the stage did something on these loci)
        for l, rows in zip(loci, got):
            invariants(l, rows)


# ---- 5. the finding
FINDING_FIXED = (120490, 107062, 101051, 113019)      # shared pairs of the four loci with prog_ref alone: the yardstick
FINDING_NEW = (121442, 107748, 102554, 113609)        # ... with the new opens, as posgap_ref gives them


@functools.lru_cache(maxsize=None)
def finding():
    """Per locus diverged_locus(seed, 30, 250, 350), seeds 0-3: (sequences, true rows, prog_ref's rows, posgap_ref's rows)."""
    out = []
    for seed in range(4):
        seqs, truth = diverged_locus(seed, 30, 250, 350)
        out.append((seqs, truth, pr.progressive_rows(seqs), pg.progressive_rows(seqs)))
    return out


def check_finding_reference():
    fixed = tuple(cmp.by_histogram(rows, truth)[0] for _, truth, rows, _ in finding())
    new = tuple(cmp.by_histogram(rows, truth)[0] for _, truth, _, rows in finding())
    print("shared pairs, fixed opens:", fixed, "by occupancy:", new)
    assert fixed == FINDING_FIXED
    assert all(b > a for a, b in zip(fixed, new))
    assert new == FINDING_NEW


def check_finding(be):
    loci = finding()
    msas = sa.star_msas(be, [pc.records(s) for s, _, _, _ in loci], progressive=True, position_gaps=True, band=True, device_tree=True)
    assert [m.rows_as_strings() for m in msas] == [rows for _, _, _, rows in loci]
    msas = sa.star_msas(be, [pc.records(s) for s, _, _, _ in loci], progressive=True)
    assert [m.rows_as_strings() for m in msas] == [rows for _, _, rows, _ in loci]


# ---- 6. status codes
def check_abi_statuses(be):
    """The new entries, handed tables that point outside a buffer, report their status code and write nothing else
    (prog_common.check_abi_statuses' and progband_common.check_abi_statuses' pattern)."""
    POISON = 0x5C
    X, Y = ("AC-T", "A-GT"), ("ACGTA", "AC-TA", "ACGTN")
    text = np.concatenate([pc.codes(X).reshape(-1), pc.codes(Y).reshape(-1)])
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64))
    WORDS = 35 + 28                                              # Y's 7 planes of 5 columns, X's 7 of 4

    def untouched(buf, n):
        return (be.download(buf, np.uint8, n) == POISON).all()

    def columns(items, work, words=WORDS, weights=None):
        d_cols, d_status = be.full(4 * WORDS, POISON), be.full(4 * len(work), POISON)
        d_items, d_work = be.upload(np.array(items, np.int64)), be.upload(np.array(work, np.int32))
        if weights is None:
            be.call("mprg_prog_columns_posgap", be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work), be.ptr(d_cols),
                    words, be.ptr(d_status), be.stream)
        else:
            d_weights = be.upload(np.array(weights, np.int32))
            be.call("mprg_prog_columns_weighted_posgap", be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work),
                    be.ptr(d_weights), len(weights), be.ptr(d_cols), words, be.ptr(d_status), be.stream)
        return be.download(d_status, np.int32, len(work)).tolist(), untouched(d_cols, 4 * WORDS), d_cols
    good = [[0, 8, 3, 5, 2, 0], [0, 0, 2, 4, 1, 35]]
    status, clean, d_cols = columns(good, [[0, 0], [1, 0]])
    assert status == [0, 0] and not clean
    cols = be.download(d_cols, np.int32, WORDS)
    P, _, Dc, Oc, cx, ambx, _, Ic, _ = pg.tables(X, Y)
    assert cols[:35].reshape(7, 5).tolist() == [P[x].tolist() for x in "ACGT"] + [pr._column_tables(X, Y)[1].tolist(), Dc.tolist(), Oc.tolist()]
    assert Oc.tolist() == [-704, -704, -469, -704, -704]
    for items, work, words, code in (([[1, 8, 3, 5, 2, 0]], [[0, 0]], WORDS, 1), ([[0, 9, 3, 5, 2, 0]], [[0, 0]], WORDS, 1),
                                     ([[0, 8, 3, 5, 3, 0]], [[0, 0]], WORDS, 1), ([[0, 8, 3, 5, -1, 0]], [[0, 0]], WORDS, 1),   # no such kind
                                     (good, [[2, 0]], WORDS, 1), (good, [[0, 1]], WORDS, 1),
                                     ([[0, 8, 3, 5, 2, 0]], [[0, 0]], 34, 3),        # the seventh plane ends one word outside
                                     ([[0, 8, 3, 5, 2, 29]], [[0, 0]], WORDS, 3), ([[0, 8, 3, 5, 2, -1]], [[0, 0]], WORDS, 3)):
        assert columns(items, work, words)[:2] == ([code], True), (items, work, words)
    wgood = [[0, 8, 3, 5, 2, 0, 0, 6]]
    assert columns(wgood, [[0, 0]], weights=[1, 2, 3])[0] == [0]
    for items, weights, code in (([[0, 8, 3, 5, 3, 0, 0, 6]], [1, 2, 3], 1), ([[0, 8, 3, 5, 2, 0, 1, 6]], [1, 2, 3], 1),
                                 ([[0, 8, 3, 5, 2, 0, 0, 7]], [1, 2, 3], 1), ([[0, 8, 3, 5, 2, 29, 0, 6]], [1, 2, 3], 3)):
        assert columns(items, [[0, 0]], weights=weights)[:2] == ([code], True), (items, weights)
    # the old entries still refuse kind 2
    d_c, d_s = be.full(4 * WORDS, POISON), be.full(4, POISON)
    d_i, d_w = be.upload(np.array([good[0]], np.int64)), be.upload(np.zeros(2, np.int32))
    be.call("mprg_prog_columns", be.ptr(d_bufs), 1, be.ptr(d_i), 1, be.ptr(d_w), 1, be.ptr(d_c), WORDS, be.ptr(d_s), be.stream)
    assert be.download(d_s, np.int32, 1).tolist() == [1] and untouched(d_c, 4 * WORDS)

    full_need, band_need = int(pa.workspace_words(4, 5)), int(pa.band_workspace_words(4, 5, -4, 5))

    def pairs(call, pair, need, leaf=(0, 3, 5, 0), xwords=WORDS, ws_words=None, ops_bytes=9):
        d_ws, d_ops, d_out = be.full(4 * need, POISON), be.full(9, POISON), be.full(12, POISON)
        d_leaves, d_pairs = be.upload(np.array([leaf], np.int64)), be.upload(np.array([pair], np.int64))
        be.call(call, be.ptr(d_cols), be.ptr(d_leaves), 1, be.ptr(d_cols), xwords, be.ptr(d_pairs), 1, be.ptr(d_ws),
                need if ws_words is None else ws_words, be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
        return be.download(d_out, np.int32, 3).tolist(), untouched(d_ops, 9) and untouched(d_ws, 4 * need), be.download(d_ops, np.uint8, 9)
    want = pg.align_profiles(X, Y)
    for call, need, band in (("mprg_align_profile_pairs_posgap", full_need, []), ("mprg_align_profile_pairs_posgap_banded", band_need, [-4, 5])):
        out, clean, ops = pairs(call, [0, 35, 4, 0, 0, 2] + band, need)
        assert out == [0, want[1], len(want[0])] and ops[:out[2]][::-1].tobytes().decode() == want[0] and not clean
        for pair, kw, code in (([1, 35, 4, 0, 0, 2], {}, 3), ([-1, 35, 4, 0, 0, 2], {}, 3), ([0, 35, -1, 0, 0, 2], {}, 3),
                               ([0, 35, 4, 0, 0, 0], {}, 3), ([0, 35, 4, 0, 0, (1 << 20) + 1], {}, 3),      # R_X out of range
                               ([0, 35, 4, 0, 0, 2], dict(leaf=(0, 0, 5, 0)), 3),
                               ([0, 36, 4, 0, 0, 2], {}, 2), ([0, -1, 4, 0, 0, 2], {}, 2), ([0, 35, 4, 0, 0, 2], dict(xwords=WORDS - 1), 2),
                               ([0, 35, 4, 64, 0, 2], {}, 2), ([0, 35, 4, 1, 0, 2], {}, 2), ([0, 35, 4, 0, 1, 2], {}, 2),
                               ([0, 35, 4, 0, 0, 2], dict(ops_bytes=8), 2), ([0, 35, 4, 0, 0, 2], dict(ws_words=need - 1), 2),
                               ([0, 35, 999_996, 0, 0, 2], {}, 1)):
            b = band if pair[2] >= 0 and pair[2] < 10 else [-999_996, 5] if band else []
            assert pairs(call, pair + b, need, **kw)[:2] == ([code, 0, 0], True), (call, pair, kw)
    for band in ([1, 5], [-4, 0], [2, 1]):                                # (0, 0) or (n, C) outside the band
        assert pairs("mprg_align_profile_pairs_posgap_banded", [0, 35, 4, 0, 0, 2] + band, band_need)[:2] == ([3, 0, 0], True)
    ref = pg.align_profiles_banded(X, Y, -1, 2)
    out, _, ops = pairs("mprg_align_profile_pairs_posgap_banded", [0, 35, 4, 0, 0, 2, -1, 2], band_need)
    assert out == [0, ref[1], len(ref[0])] and ops[:out[2]][::-1].tobytes().decode() == ref[0]

    def widths(pair, out=(0, 0, 0), leaf=(0, 3, 5, 0), xwords=WORDS):
        d_bounds, d_status = be.full(16, POISON), be.full(4, POISON)
        d_leaves, d_pairs = be.upload(np.array([leaf], np.int64)), be.upload(np.array([pair], np.int64))
        d_out = be.upload(np.array(out, np.int32))
        be.call("mprg_prog_band_widths_posgap", be.ptr(d_cols), be.ptr(d_leaves), 1, be.ptr(d_cols), xwords, be.ptr(d_pairs), 1,
                be.ptr(d_out), be.ptr(d_bounds), be.ptr(d_status), be.stream)
        return be.download(d_status, np.int32, 1).tolist(), untouched(d_bounds, 16), be.download(d_bounds, np.int64, 2).tolist()
    b = pg.bounds(X, Y)
    for s in (want[1], want[1] - 3000, b[0]):
        assert widths([0, 35, 4, 0, 0, 2, 0, 0], (0, s, 0)) == ([0], False, [b[0], pg.wstar(*b, 4, 5, s)])
    for pair, kw, code in (([1, 35, 4, 0, 0, 2, 0, 0], {}, 3), ([-1, 35, 4, 0, 0, 2, 0, 0], {}, 3), ([0, 35, -1, 0, 0, 2, 0, 0], {}, 3),
                           ([0, 35, 4, 0, 0, 0, 0, 0], {}, 3), ([0, 35, 4, 0, 0, (1 << 20) + 1, 0, 0], {}, 3),
                           ([0, 35, 4, 0, 0, 2, 0, 0], dict(leaf=(0, 0, 5, 0)), 3), ([0, 35, 4, 0, 0, 2, 0, 0], dict(leaf=(0, 3, 0, 0)), 3),
                           ([0, 35, 4, 0, 0, 2, 0, 0], dict(out=(2, 0, 0)), 3),                           # pass 1 refused the merge
                           ([0, 36, 4, 0, 0, 2, 0, 0], {}, 2), ([0, -1, 4, 0, 0, 2, 0, 0], {}, 2), ([0, 35, 4, 0, 0, 2, 0, 0], dict(xwords=WORDS - 1), 2),
                           ([0, 35, 999_996, 0, 0, 2, 0, 0], {}, 1)):
        assert widths(pair, **kw)[:2] == ([code], True), (pair, kw)


# ---- 7. the command line
def cli_loci():
    return [pr.table_loci()[0], pr.clade_locus(0, 6)]


def write_inputs(src):
    """The two loci as FASTA files under src: {the name of the file from_msa writes: posgap_ref's text}."""
    want = {}
    for k, l in enumerate(cli_loci()):
        recs = [(f"s{i} x", s) for i, s in enumerate(l)]
        (src / f"g{k}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"g{k}.fa"] = pg.progressive_fasta(recs)
    assert want != {f"g{k}.fa": pr.progressive_fasta([(f"s{i} x", s) for i, s in enumerate(l)]) for k, l in enumerate(cli_loci())}
    return want


def check_cli(be, tmp_path, caplog):
    """from_msa.run with --unaligned --progressive --position-gaps --msa-dir (in process): the files are posgap_ref's and the log
    has the flag's line; without the flag the files are prog_ref's and the line is absent."""
    import logging
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    want = write_inputs(src)
    merges = sum(len(l) - 1 for l in cli_loci())

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None, progressive=True)
        base.update(kw)
        return Namespace(**base)
    for flag in (True, False):
        caplog.clear()
        d = tmp_path / f"msas{flag}"
        with caplog.at_level(logging.INFO):
            from_msa.run(opts(output_prefix=str(tmp_path / f"o{flag}" / "a"), msa_dir=str(d), position_gaps=flag), be)
        got = {p.name: p.read_text() for p in d.iterdir()}
        lines = [r.getMessage() for r in caplog.records if "--position-gaps:" in r.getMessage()]
        if flag:
            assert got == want and len(lines) == 1 and f"--position-gaps: {merges} merges" in lines[0]
        else:
            assert got != want and not lines
            assert got == {f"g{k}.fa": pr.progressive_fasta([(f"s{i} x", s) for i, s in enumerate(l)]) for k, l in enumerate(cli_loci())}


def check_parser(capsys):
    """--position-gaps without --progressive is a parser error."""
    import pytest
    from make_prg_amd import __main__ as cli
    with pytest.raises(SystemExit) as exc:
        cli.main(["from_msa", "-i", "x", "-o", "y", "--unaligned", "--position-gaps"])
    assert exc.value.code == 2 and "--position-gaps needs --progressive" in capsys.readouterr().err
