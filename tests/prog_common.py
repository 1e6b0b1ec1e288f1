"""What the emulated and the GPU tests of `from_msa --unaligned --progressive` share: the profile pairs of the DP check, the tall
pairs (8 to 2^20 rows a side, and 1 x 1 merges whose numerators sit on and beside multiples of R_X) and tall column texts, the
loci of the whole-MSA check with their reference (computed once per process), the reference compositions with
--adjust-direction and --refine, and the status codes of the new C ABI entries for tables that point outside their buffers."""
import functools
import random

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.msa import encode
from tests import align_ref as ar
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import star_ref as sr
from tests import strand_ref as st

WX = (1, 63, 64, 65, 128, 129, 200)       # around the 64-column strip and the 128-column ring
WY = (1, 127, 128, 129, 300)
ROWS = (1, 2, 3, 7)


def records(seqs):
    return [(f"r{i} desc {i}", s) for i, s in enumerate(seqs)]


def codes(rows) -> np.ndarray:
    return encode(np.frombuffer("".join(rows).encode(), np.uint8)).reshape(len(rows), -1)


@functools.lru_cache(maxsize=None)
def dp_cases():
    """((X, Y) as tuples of row strings, prog_ref's (ops, score)): every W_X x W_Y of the lists above with the row counts taken in
    turn, dense and mostly-gap columns, ambiguity codes, and two pairs with one side much longer than the other."""
    rng = random.Random(11)
    shapes = [(wx, wy) for wx in WX for wy in WY] + [(3, 700), (700, 3), (130, 130)]
    out = []
    for k, (wx, wy) in enumerate(shapes):
        rx, ry = ROWS[k % 4], ROWS[(k // 4 + k) % 4]
        gx, gy = (0.1, 0.75, 0.3)[k % 3], (0.1, 0.3, 0.75)[(k // 3) % 3]
        X = tuple(pr.random_profiles(rng, rx, wx, gx, amb=0.1 if k % 2 else 0.0))
        Y = tuple(pr.random_profiles(rng, ry, wy, gy, amb=0.1 if k % 5 == 0 else 0.02))
        out.append(((X, Y), pr.align_profiles_np(X, Y)))
    return out


def check_dp(be, **kw):
    cases = dp_cases()
    assert {len(x) for (x, _), _ in cases} == set(ROWS) and {len(y) for (_, y), _ in cases} == set(ROWS)
    got = sa.merge_profiles(be, [(codes(x), codes(y)) for (x, y), _ in cases], **kw)
    for ((x, y), want), (ops, score) in zip(cases, got):
        assert (ops.decode(), score) == want, (len(x), len(x[0]), len(y), len(y[0]))


TALL = (8, 9, 31, 33, 64, 255, 256, 257, 1000, 4095, 4096, 65537)        # rows per side: around the powers of two pg_div's shift turns on
TALL_MAX = 1 << 20                                                       # PG_MAX_ROWS
TALL_WX, TALL_WY = (63, 65, 130), (66, 129)                              # around the strip and the ring
DIVISORS = (255, 256, 257, 65535, 65536, 65537, TALL_MAX - 1, TALL_MAX)  # R_X just below, at and just above a power of two
Y_POOL = ("AAAAAAAAA", "CCCCCCCCC", "---------", "AAAAACC-N", "AAAAAAAC-", "AACCGGTT-", "A--------", "AAAANNN--", "AAAAAAAAC")


def related_codes(rng, L, anc, R, W, spare=()):
    """An R x W matrix of cell codes whose columns are W of the ancestor's L (in order): its base, 6 % another base, 3 % an
    ambiguity code, '-' at a rate of the column's own (2 %, 10 % or 60 %); no all-gap column."""
    cols = np.sort(rng.choice(L, W, replace=False))
    base = anc[cols].astype(np.uint8)
    u = rng.random((R, W), dtype=np.float32)
    m = np.repeat(base[None], R, 0)
    sub = u < 0.06
    m[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
    amb = (u >= 0.06) & (u < 0.09)
    m[amb] = rng.integers(5, 12, int(amb.sum()), dtype=np.uint8)
    m[u > 1 - rng.choice([0.02, 0.1, 0.6], W, p=[0.6, 0.3, 0.1]).astype(np.float32)[None]] = 4
    empty = (m == 4).all(0)
    m[0, empty] = base[empty]
    return m


def engineered_columns(R):
    """1 x 1 merges whose score is one quotient num / R_X exactly (the column pair always beats the two gaps): per class of
    numerator (X's column, Y's column, num).  X's column: a A's, m N's, the rest '-'; Y's: a column of Y_POOL (9 rows).  The
    classes: an exact multiple q R of R_X, one above and one below it, for q > 0 and q < 0; the largest numerator there is,
    1 280 R_X (all A against all A); -576 R_X (all A against all C); the smallest, -640 R_X, both ways (all A against all '-',
    all '-' against all A).  (-1 280 R_X does not exist: no term of a numerator is below -640 per row.)"""
    pool = codes(Y_POOL).T.copy()                                        # 9 rows x the pool's columns
    P, Pamb, Dc, _, _, _, _ = pr._column_tables(pool, pool)

    def column(a, m):
        return np.concatenate([np.zeros(a, np.uint8), np.full(m, 11, np.uint8), np.full(R - a - m, 4, np.uint8)]).reshape(R, 1)
    out = {}
    a = np.arange(R + 1, dtype=np.int64)
    for sign in (1, -1):
        for name, rem in (("multiple", 0), ("above", 1), ("below", R - 1)):
            found = None
            for j in range(1, pool.shape[1]):
                for m in range(4):
                    num = a[:R + 1 - m] * int(P["A"][j]) + m * int(Pamb[j]) + (R - m - a[:R + 1 - m]) * int(Dc[j])
                    hit = np.nonzero((num % R == rem) & (num * sign >= R))[0]
                    if len(hit) and found is None:
                        found = (column(int(hit[len(hit) // 2]), m), pool[:, j:j + 1], int(num[hit[len(hit) // 2]]))
            assert found is not None, (R, sign, name)
            out[name, sign] = found
    out["largest", 1] = (column(R, 0), pool[:, 0:1], 1280 * R)
    out["mismatch", -1] = (column(R, 0), pool[:, 1:2], -576 * R)
    out["smallest, Y's gaps", -1] = (column(R, 0), pool[:, 2:3], -640 * R)
    out["smallest, X's gaps", -1] = (column(0, 0), pool[:, 0:1], -640 * R)
    return out


@functools.lru_cache(maxsize=None)
def tall_dp_cases():
    """((X, Y) as matrices of cell codes, prog_ref's (ops, score)): related sides (columns of one ancestor) with every row count
    of TALL on either side and 2^20 rows once on each, then engineered_columns of every R_X of DIVISORS."""
    rng = np.random.default_rng(17)
    shapes = [(rx, TALL_WX[k % 3], TALL[(5 * k + 3) % len(TALL)], TALL_WY[k % 2]) for k, rx in enumerate(TALL)]
    shapes += [(TALL_MAX, 8, 31, 12), (255, 10, TALL_MAX, 8)]            # (a 2^20-row side stays narrow: k_prog_columns walks a column's rows one by one)
    out = []
    for rx, wx, ry, wy in shapes:
        L = max(wx, wy) + 8
        anc = rng.integers(0, 4, L)
        X, Y = related_codes(rng, L, anc, rx, wx), related_codes(rng, L, anc, ry, wy)
        out.append(((X, Y), pr.align_profiles_np(X, Y)))
    for R in DIVISORS:
        for (name, sign), (X, Y, num) in engineered_columns(R).items():
            # through the reference: the numerator is what the class says, and the merge's score is its quotient
            assert int(pr.numerators(X, Y)[0, 0]) == num and num * sign >= R and len(X) == R, (R, name)
            assert {"multiple": num % R == 0, "above": num % R == 1, "below": num % R == R - 1}.get(name, abs(num) in (1280 * R, 576 * R, 640 * R))
            want = pr.align_profiles_np(X, Y)
            assert want == ("M", ar.tdiv(num, R)), (R, name)
            out.append(((X, Y), want))
    return out


def check_tall_dp(be, **kw):
    """merge_profiles (band=True: the banded two passes) on tall_dp_cases: ops and score, exactly."""
    cases = tall_dp_cases()
    assert {len(x) for (x, _), _ in cases} >= set(TALL + DIVISORS) and {len(y) for (_, y), _ in cases} >= set(TALL + (TALL_MAX,))
    related = cases[:len(TALL) + 2]
    assert set("".join(ops for _, (ops, _) in related)) == set("MID") and sum(score > 0 for _, (_, score) in related) >= 3
    got = sa.merge_profiles(be, [xy for xy, _ in cases], **kw)
    for ((x, y), want), (ops, score) in zip(cases, got):
        assert (ops.decode(), score) == want, (x.shape, y.shape)


def check_tall_columns(be):
    """mprg_prog_columns called directly, kind 0 and kind 1, on texts of 255 to 2^20 rows (one of them across a 256-column tile):
    every plane equals the NumPy statement with C's truncating division."""
    rng = np.random.default_rng(8)
    texts = []
    for R, W in ((255, 300), (256, 64), (257, 257), (65537, 40), (TALL_MAX, 8)):
        t = related_codes(rng, W, rng.integers(0, 4, W), R, W)
        t[:, 0], t[:, 1], t[:, 2], t[:, 3] = 0, 4, 11, 4                 # all A, all '-', all N, one C among '-'
        t[R // 2, 3] = 1
        texts.append(t)
    off = sa.exclusive_sum([t.size for t in texts])
    text = np.concatenate([t.reshape(-1) for t in texts])
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64))
    items, work, words = [], [], 0
    for kind in (0, 1):
        for t, o in zip(texts, off.tolist()):
            work += [[len(items), tile] for tile in range(-(-t.shape[1] // 256))]
            items.append([0, o, *t.shape, kind, words])
            words += (6 + kind) * t.shape[1]
    d_cols, d_status = be.full(4 * words + 64, 0x5C), be.full(4 * len(work), 0x5C)
    d_items, d_work = be.upload(np.array(items, np.int64)), be.upload(np.array(work, np.int32))
    be.call("mprg_prog_columns", be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work), be.ptr(d_cols), words,
            be.ptr(d_status), be.stream)
    assert not be.download(d_status, np.int32, len(work)).any()
    assert (be.download(d_cols, np.uint8, 4 * words + 64)[4 * words:] == 0x5C).all()
    cols = be.download(d_cols, np.int32, words)
    for (_, _, R, W, kind, o), t in zip(items, texts + texts):
        P, Pamb, Dc, cx, ambx, _, Ic = pr._column_tables(t, t)
        want = [P[x] for x in "ACGT"] + [Pamb, Dc] if kind == 0 else [cx[x] for x in "ACGT"] + [ambx, cx["-"], Ic]
        assert (cols[o:o + (6 + kind) * W].reshape(6 + kind, W) == np.stack(want)).all(), (R, W, kind)
        assert min(int(v.min()) for v in want) < 0 < max(int(v.max()) for v in want)


PLANE_ROWS, PLANE_WIDTHS = (1, 2, 3, 7), (1, 255, 256, 257)               # the widths: around k_prog_columns' 256-column tile


@functools.lru_cache(maxsize=None)
def plane_texts():
    """16 texts of row strings over all twelve codes: an all-gap column, an all-ambiguity column and a column with one residue
    among gaps (its numerators are negative and, for 3 and 7 rows, no multiples of R) in each of 255 columns or more; a text of
    one column is one of the three in turn (all-gap, all-ambiguity, one residue, one residue: the last two have 3 and 7 rows)."""
    rng = random.Random(23)
    out = []
    for k, R in enumerate(PLANE_ROWS):
        for W in PLANE_WIDTHS:
            t = [[rng.choice("ACGT-RYKMSWN") for _ in range(W)] for _ in range(R)]
            special = (["-"] * R, [rng.choice("RYKMSWN") for _ in range(R)], ["-"] * (R // 2) + [rng.choice("ACGT")] + ["-"] * (R - R // 2 - 1))
            for j, col in ((0, special[min(k, 2)]),) if W == 1 else ((W // 2, special[0]), (W - 1, special[1]), (0, special[2])):
                for r in range(R):
                    t[r][j] = col[r]
            out.append(tuple("".join(r) for r in t))
    return out


def check_planes_agree(be):
    """The four producers of planes on plane_texts: mprg_align_profiles, mprg_prog_columns kind 0 and the plain-Python profile are
    equal, kind 1 equals the plain-Python X tables; mprg_prog_columns_weighted gives both with weights 1, and with weights 1..5 the
    unweighted planes of the text with row r written w_r times; mprg_refine_profiles, for every row of every text of two rows or
    more, gives mprg_align_profiles of the text without it."""
    from tests import collapse_common as cc                              # (it imports this module)
    from tests import collapse_ref as cr
    from tests import refine_common as rc
    texts = plane_texts()
    assert {(len(t), len(t[0])) for t in texts} == {(R, W) for R in PLANE_ROWS for W in PLANE_WIDTHS}
    assert all(64 * (9 + 10 * (R - 1)) % R for R in (3, 7))                # a base against one other base among gaps: -64 (9 + 10 (R - 1)) / R
    mats = [codes(t) for t in texts]

    def planes(got):
        status, raw, items = got
        assert not any(status)
        cols = raw.view(np.int32)
        return [cols[o:o + (6 + kind) * W].reshape(6 + kind, W) for _, _, _, W, kind, o, *_ in items]
    plain = planes(cc._columns(be, mats))
    for k, t in enumerate(texts):
        P, Dc, cx, Ic = pr.column_tables(t, t)
        want = np.array([[p[x] for p in P] for x in "ACGTN"] + [Dc])
        assert (plain[k] == want).all() and (rc.align_profiles(be, t) == want).all(), (len(t), len(t[0]))
        assert (plain[len(texts) + k] == np.array([[c[x] for c in cx] for x in ("A", "C", "G", "T", "amb", "-")] + [Ic])).all(), (len(t), len(t[0]))
    ones = planes(cc._columns(be, mats, [np.ones(len(t), np.int64) for t in texts]))
    assert all((a == b).all() for a, b in zip(ones, plain))
    rng = np.random.default_rng(29)
    weights = [rng.integers(1, 6, len(t)) for t in texts]
    got = planes(cc._columns(be, mats, weights))
    want = planes(cc._columns(be, [codes(cr.expanded(t, w.tolist())) for t, w in zip(texts, weights)]))
    assert all((a == b).all() for a, b in zip(got, want)) and any(int(w.sum()) > len(w) for w in weights)
    msas = [list(t) for t in texts if len(t) >= 2]
    d_text, nbytes, toff, R, W = rc.upload_msas(be, msas)
    rtab, d_counts, _, n_cols, _, _ = sa.refine_counts(be, d_text, nbytes, toff, R, W)
    row_locus, row_in = np.repeat(np.arange(len(msas)), R), np.concatenate([np.arange(n) for n in R])
    d_prof, poff, words = sa.refine_profiles(be, d_text, nbytes, rtab, d_counts, n_cols, row_locus, row_in)
    prof = be.download(d_prof, np.int32, words)
    for k, r, p in zip(row_locus.tolist(), row_in.tolist(), poff.tolist()):
        m = msas[k]
        assert (prof[p:p + 6 * len(m[0])].reshape(6, -1) == rc.align_profiles(be, m[:r] + m[r + 1:])).all(), (len(m), len(m[0]), r)


def msa_loci():
    """Edge, special, random and the 18 table loci: balanced trees and caterpillars, one to several rounds."""
    return sr.edge_loci() + rr.special_loci() + sr.random_loci(3) + sr.random_loci(21, 20) + pr.table_loci()


@functools.lru_cache(maxsize=None)
def msa_spec():
    return [pr.progressive(l) for l in msa_loci()]


def check_msas(be, **kw):
    loci, info, timings = msa_loci(), [], {}
    msas = sa.star_msas(be, [records(l) for l in loci], progressive=True, progression=info, timings=timings, **kw)
    for l, m, got, (rows, want) in zip(loci, msas, info, msa_spec()):
        assert m.rows_as_strings() == rows, l
        assert got == want, l
        assert m.descriptions == [t for t, _ in records(l)]
    rounds = [r for _, r, _ in info]
    leaves = [n for n, _, _ in info]
    assert max(rounds) >= 6 and any(r == n - 1 and n >= 4 for n, r, _ in info) and any(2 <= r < n - 1 for n, r, _ in info)
    assert min(leaves) == 1 and timings["tree_s"] > 0 and timings["progressive_s"] > 0


def check_distances(be, loci):
    norm = [[sr.normalise(s) for s in l] for l in loci]
    got = sa.prog_shared(be, [sa.locus_codes(str(k), records(l)) for k, l in enumerate(loci)])
    for l, (shared, nw) in zip(norm, got):
        D, S, want_nw = pr.distances(l)
        assert nw.tolist() == want_nw, l
        assert np.triu(shared, 1).tolist() == np.triu(np.array(S, np.int64).reshape(len(l), len(l)), 1).tolist(), l
        assert sa.prog_distance_matrix(shared, nw).tolist() == D, l


def flipped_loci():
    rng = random.Random(4)
    loci = [pr.clade_locus(s, 8) for s in range(10, 16)] + [rr.diverged_locus(s, 8) for s in range(16, 20)] + sr.random_loci(31, 16)
    return [[st.rc(s) if i and rng.random() < 0.4 else s for i, s in enumerate(l)] for l in loci]


@functools.lru_cache(maxsize=None)
def flipped_spec():
    """Per locus (titles, progressive rows, those rows refined by two rounds) of the reference composition: strand_ref's
    orientation, prog_ref on the oriented sequences, refine_ref on its rows."""
    out = []
    for l in flipped_loci():
        rev, _, ori = st.oriented(l)
        rows = pr.progressive_rows(ori)
        out.append((st.titles(records(l), rev), rows, rr.refine_rows(rows, 2)))
    return out


def check_compositions(be):
    recs = [records(l) for l in flipped_loci()]
    spec = flipped_spec()
    msas = sa.star_msas(be, recs, progressive=True, adjust_direction=True)
    assert [(m.descriptions, m.rows_as_strings()) for m in msas] == [(t, rows) for t, rows, _ in spec]
    assert sum(t.startswith(sa.REVERSED_PREFIX) for m in msas for t in m.descriptions) >= 20
    for band in (False, True):
        info = []
        msas = sa.star_msas(be, recs, progressive=True, adjust_direction=True, refine=2, refinement=info, band=band)
        for m, got, (t, _, (rows, acc, trail)) in zip(msas, info, spec):
            assert m.descriptions == t and m.rows_as_strings() == rows and got == (acc, trail[0], trail[-1])
        assert any(a for a, _, _ in info) and any(not a for a, _, _ in info)


def check_abi_statuses(be):
    """The new entries, handed tables that point outside a buffer, report their status code and write nothing else."""
    POISON = 0x5C
    X, Y = ["AC-T", "A-GT"], ["ACGTA", "AC-TA", "ACGTN"]
    text = np.concatenate([codes(X).reshape(-1), codes(Y).reshape(-1)])
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64))

    def untouched(buf, n):
        return (be.download(buf, np.uint8, n) == POISON).all()

    def columns(items, work, words=58):
        d_cols, d_status = be.full(4 * 58, POISON), be.full(4 * len(work), POISON)
        d_items, d_work = be.upload(np.array(items, np.int64)), be.upload(np.array(work, np.int32))
        be.call("mprg_prog_columns", be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work), be.ptr(d_cols), words,
                be.ptr(d_status), be.stream)
        return be.download(d_status, np.int32, len(work)).tolist(), untouched(d_cols, 4 * 58), d_cols
    good = [[0, 8, 3, 5, 0, 0], [0, 0, 2, 4, 1, 30]]
    status, clean, d_cols = columns(good, [[0, 0], [1, 0]])
    assert status == [0, 0] and not clean
    cols = be.download(d_cols, np.int32, 58)
    P, Dc = ar.profile(Y)
    assert cols[:30].reshape(6, 5).tolist() == [[p[x] for p in P] for x in "ACGTN"] + [Dc]
    assert cols[30:].reshape(7, 4).tolist() == [[2, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 2], [0, 0, 0, 0], [0, 1, 1, 0],
                                                [-640, -320, -320, -640]]
    for items, work, words, code in (([[1, 8, 3, 5, 0, 0]], [[0, 0]], 58, 1),        # no such buffer
                                     ([[0, 9, 3, 5, 0, 0]], [[0, 0]], 58, 1),        # the text ends one byte outside
                                     ([[0, -1, 3, 5, 0, 0]], [[0, 0]], 58, 1),
                                     ([[0, 8, 0, 5, 0, 0]], [[0, 0]], 58, 1),
                                     ([[0, 8, 3, 5, 2, 0]], [[0, 0]], 58, 1),        # no such kind
                                     (good, [[2, 0]], 58, 1), (good, [[-1, 0]], 58, 1), (good, [[0, 1]], 58, 1), (good, [[0, -1]], 58, 1),
                                     (good, [[1, 0]], 57, 3),                        # the planes end one word outside
                                     ([[0, 8, 3, 5, 0, 29]], [[0, 0]], 58, 3), ([[0, 8, 3, 5, 0, -1]], [[0, 0]], 58, 3)):
        assert columns(items, work, words)[:2] == ([code], True), (items, work, words)

    def pairs(pair, leaf=(0, 3, 5, 0), xwords=58, ws_words=None, ops_bytes=9):
        need = sa.pa.workspace_words(4, 5)
        d_ws, d_ops, d_out = be.empty(4 * need), be.full(9, POISON), be.full(12, POISON)
        d_leaves, d_pairs = be.upload(np.array([leaf], np.int64)), be.upload(np.array([pair], np.int64))
        be.call("mprg_align_profile_pairs", be.ptr(d_cols), be.ptr(d_leaves), 1, be.ptr(d_cols), xwords, be.ptr(d_pairs), 1, be.ptr(d_ws),
                need if ws_words is None else ws_words, be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
        out = be.download(d_out, np.int32, 3).tolist()
        return out, untouched(d_ops, 9), be.download(d_ops, np.uint8, 9)
    out, clean, ops = pairs([0, 30, 4, 0, 0, 2])
    want = pr.align_profiles(X, Y)
    assert out == [0, want[1], len(want[0])] and ops[:out[2]][::-1].tobytes().decode() == want[0]
    for pair, kw, code in (([1, 30, 4, 0, 0, 2], {}, 3), ([-1, 30, 4, 0, 0, 2], {}, 3), ([0, 30, -1, 0, 0, 2], {}, 3),
                           ([0, 30, 4, 0, 0, 0], {}, 3), ([0, 30, 4, 0, 0, (1 << 20) + 1], {}, 3),      # R_X out of range
                           ([0, 30, 4, 0, 0, 2], dict(leaf=(0, 0, 5, 0)), 3),
                           ([0, 31, 4, 0, 0, 2], {}, 2), ([0, -1, 4, 0, 0, 2], {}, 2), ([0, 30, 4, 0, 0, 2], dict(xwords=57), 2),
                           ([0, 30, 4, 64, 0, 2], {}, 2), ([0, 30, 4, 1, 0, 2], {}, 2), ([0, 30, 4, 0, 1, 2], {}, 2),
                           ([0, 30, 4, 0, 0, 2], dict(ops_bytes=8), 2), ([0, 30, 999_996, 0, 0, 2], {}, 1)):
        assert pairs(pair, **kw)[:2] == ([code, 0, 0], True), (pair, kw)

    d_ops = be.upload(np.frombuffer(want[0][::-1].encode(), np.uint8))
    k = len(want[0])

    def rows(table, out_bytes=None, ops_bytes=k, ascii=1):
        n = 5 * k
        d_out, d_status = be.full(n, POISON), be.full(4 * len(table), POISON)
        d_rows = be.upload(np.array(table, np.int64))
        be.call("mprg_prog_rows", be.ptr(d_bufs), 1, be.ptr(d_ops), ops_bytes, be.ptr(d_rows), len(table), be.ptr(d_out),
                n if out_bytes is None else out_bytes, ascii, be.ptr(d_status), be.stream)
        return be.download(d_status, np.int32, len(table)).tolist(), be.download(d_out, np.uint8, n).tobytes()
    table = [[0, 8 + 5 * r, 5, 0, k, 0, r * k, k] for r in range(3)] + [[0, 4 * r, 4, 0, k, 1, (3 + r) * k, k] for r in range(2)]
    nx, ny = pr.merge_rows(X, Y, want[0])
    assert rows(table) == ([0] * 5, "".join(ny + nx).encode())
    assert rows(table, ascii=0) == ([0] * 5, codes(ny + nx).tobytes())
    assert rows([[0, 8, 5, 0, -1, 0, 0, 7]]) == ([0], b"ACGTA--" + bytes([POISON]) * (5 * k - 7))
    blank = bytes([POISON]) * (5 * k)
    for row, kw, code in (([1, 8, 5, 0, k, 0, 0, k], {}, 1), ([0, 19, 5, 0, k, 0, 0, k], {}, 1), ([0, -1, 5, 0, k, 0, 0, k], {}, 1),
                          ([0, 8, 5, 0, k, 2, 0, k], {}, 1),
                          ([0, 8, 5, 0, k, 0, 4 * k + 1, k], {}, 3), ([0, 8, 5, 0, k, 0, -1, k], {}, 3), ([0, 8, 5, 0, k, 0, 0, k], dict(out_bytes=k - 1), 3),
                          ([0, 8, 5, 0, k, 0, 0, k + 1], {}, 2), ([0, 8, 5, 1, k, 0, 0, k], {}, 2), ([0, 8, 5, 0, k, 0, 0, k], dict(ops_bytes=k - 1), 2),
                          ([0, 8, 5, 0, -1, 0, 0, 4], {}, 2)):
        assert rows([row], **kw) == ([code], blank), (row, kw)
    assert rows([[0, 8, 4, 0, k, 0, 0, k]])[0] == [2]          # a row with a cell less than the ops consume

    seqs = ["ACGTACGTAC", "ACGTTCGTAC", ""]
    packed = np.concatenate([sa.locus_codes("l", records(seqs))[i] for i in range(3)] + [np.zeros(1, np.uint8)])
    d_codes = be.upload(packed)

    def distances(stab, ltab, work, words=9, codes_bytes=21):
        d_shared, d_nw, d_status = be.full(4 * 9, POISON), be.full(24, POISON), be.full(4 * len(work), POISON)
        d_seqs, d_loci, d_work = be.upload(np.array(stab, np.int64)), be.upload(np.array(ltab, np.int64)), be.upload(np.array(work, np.int32))
        be.call("mprg_prog_distances", be.ptr(d_codes), codes_bytes, be.ptr(d_seqs), 3, be.ptr(d_loci), 1, be.ptr(d_work), len(work),
                be.ptr(d_shared), words, be.ptr(d_nw), be.ptr(d_status), be.stream)
        return (be.download(d_status, np.int32, len(work)).tolist(), untouched(d_shared, 36) and untouched(d_nw, 24),
                be.download(d_shared, np.uint32, 9).tolist(), be.download(d_nw, np.int64, 3).tolist())
    stab, ltab = [[0, 10], [10, 10], [20, 0]], [[0, 3, 0, 0]]
    status, clean, shared, nw = distances(stab, ltab, [[0, 0], [0, 1], [0, 2]])
    _, S, want_nw = pr.distances(seqs)
    assert status == [0, 0, 0] and nw == want_nw == [5, 5, 0] and [shared[1], shared[2], shared[5]] == [S[0][1], S[0][2], S[1][2]]
    for s2, l2, work, kw in ((stab, ltab, [[1, 0]], {}), (stab, ltab, [[-1, 0]], {}), (stab, ltab, [[0, 3]], {}), (stab, ltab, [[0, -1]], {}),
                             (stab, [[1, 3, 0, 0]], [[0, 0]], {}), (stab, [[0, 3, 0, 1]], [[0, 0]], {}), (stab, ltab, [[0, 0]], dict(words=8)),
                             ([[0, 10], [10, 12], [20, 0]], ltab, [[0, 0]], {}), ([[0, 10], [-1, 10], [20, 0]], ltab, [[0, 0]], {}),
                             (stab, ltab, [[0, 0]], dict(codes_bytes=19))):
        assert distances(s2, l2, work, **kw)[:2] == ([1], True), (s2, l2, work, kw)
