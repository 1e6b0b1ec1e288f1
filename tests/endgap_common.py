"""What the emulated and the GPU tests of `from_msa --unaligned --progressive --free-end-gaps` share (the spec: star_align.py,
"Free end gaps"; its plain-Python statement: tests/endgap_ref.py): the profile pairs of the DP check (the last row and column at
strip and ring edges, fragments, overhangs, ties between a free run and a match, tall sides), the banded entries, the widths entry,
the two passes, whole MSAs and their compositions, the four fragment loci of the finding, the status codes of the five new entries
and the command line's inputs.  Every check takes posgap: the opens of "Position gaps" inside the matrix, and their entries."""
import functools
import random
from collections import Counter

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from make_prg_amd.utils.synthetic import fragment_locus
from tests import band_ref as br
from tests import collapse_ref as cr
from tests import compare_ref as cmp
from tests import endgap_ref as eg
from tests import posgap_common as pgc
from tests import posgap_ref as pg
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import progband_common as pbc
from tests import refine_ref as rr
from tests import star_ref as sr

W0 = pbc.W0
LAST_ROWS, LAST_COLS = (63, 64, 65, 128, 129), (63, 64, 65, 130)


def entry(posgap, banded=False):
    return "mprg_align_profile_pairs" + ("_posgap" if posgap else "") + "_endgap" + ("_banded" if banded else "")


def flag_off(X, Y, posgap):
    return pg.align_profiles_np(X, Y) if posgap else pr.align_profiles_np(X, Y)


# ---- 2. the DP against the reference
def _family(rng, L, m, sub=0.05, indel=0.03):
    root = "".join(rng.choice("ACGT") for _ in range(L))
    return root, [sr.mutate(rng, root, sub, indel) or "A" for _ in range(m)]


@functools.lru_cache(maxsize=None)
def extra_pairs():
    """(X, Y) beyond prog_common.dp_cases' shapes: the last row as lane 63 of a strip or lane 0 of a new one against the last column
    at a ring-block edge; X a fragment of Y at its start, in its middle and at its end (n << C); Y a fragment of X with overhang at
    both ends (n >> C); two sides that overlap only by their ends; tandem repeats, where a free trailing run ties with a match."""
    rng = random.Random(31)
    out = []
    for k, (n, C) in enumerate((n, C) for n in LAST_ROWS for C in LAST_COLS):
        X = tuple(pr.random_profiles(rng, pc.ROWS[k % 4], n, (0.1, 0.6)[k % 2], amb=0.05))
        Y = tuple(pr.random_profiles(rng, pc.ROWS[(k + 1) % 4], C, (0.1, 0.3, 0.7)[k % 3], amb=0.05))
        out.append((X, Y))
    root, seqs = _family(rng, 300, 5)
    whole = tuple(pr.progressive_rows(seqs[:3]))
    for a, m in ((0, 40), (130, 45), (len(seqs[3]) - 50, 50)):                  # X a fragment of Y: start, middle, end
        out.append((tuple(pr.progressive_rows([seqs[3][a:a + m], seqs[4][a:a + m]])), whole))
    out.append((whole, tuple(pr.progressive_rows([seqs[3][90:150], seqs[4][88:151]]))))      # Y a fragment of X, overhang at both ends
    out.append(((seqs[0],), (seqs[1][120:200],)))
    out.append(((seqs[0][:180],), (seqs[1][120:],)))                            # the end of X against the start of Y
    out.append((tuple(pr.progressive_rows([s[170:] for s in seqs[:2]])), tuple(pr.progressive_rows([s[:200] for s in seqs[2:]]))))
    for unit, a, b in (("A", 1, 2), ("A", 2, 1), ("AC", 3, 5), ("ACG", 22, 24), ("ACGT", 17, 16), ("AC", 33, 31)):   # ties
        out.append(((unit * a,), (unit * b,)))
        out.append(((unit * a, unit * a), (unit * b, unit * b, unit * b)))
    return out


def ties_with_a_free_run(X, Y, posgap=False):
    """At (n, C) the diagonal ties with the free run of the last row or of the last column."""
    H, D, I, sc, _, _, n, C = eg._cells(X, Y, -len(X[0]), len(Y[0]), posgap, True)
    return H[n - 1][C - 1] + sc(n - 1, C - 1) == H[n][C] and H[n][C] in (D[n][C], I[n][C])


@functools.lru_cache(maxsize=None)
def dp_cases(posgap):
    """((X, Y), endgap_ref's (ops, score)): prog_common.dp_cases' pairs, then extra_pairs."""
    pairs = [xy for xy, _ in pc.dp_cases()] + extra_pairs()
    return [(xy, eg.align_profiles_np(*xy, posgap=posgap)) for xy in pairs]


def check_dp(be, posgap, **kw):
    cases = dp_cases(posgap)
    shapes = {(len(x[0]), len(y[0])) for (x, y), _ in cases}
    assert (1, 1) in shapes and {(n, C) for n in LAST_ROWS for C in LAST_COLS} <= shapes
    assert sum(want != flag_off(*xy, posgap) for xy, want in cases) >= 30       # the free ends change results, or nothing is tested
    assert sum(ties_with_a_free_run(*xy, posgap) for xy in extra_pairs()[-12:]) >= 6
    assert sum(want[0].startswith("DDDDD") or want[0].startswith("IIIII") for _, want in cases) >= 10
    assert sum(want[0].endswith("DDDDD") or want[0].endswith("IIIII") for _, want in cases) >= 10
    got = sa.merge_profiles(be, [(pc.codes(x), pc.codes(y)) for (x, y), _ in cases], position_gaps=posgap, free_end_gaps=True, **kw)
    for ((x, y), want), (ops, score) in zip(cases, got):
        assert (ops.decode(), score) == want, (len(x), len(x[0]), len(y), len(y[0]))


@functools.lru_cache(maxsize=None)
def tall_cases(posgap):
    """posgap_common.tall_cases' related sides of 8, 255, 257 and 4 096 rows (on X's side), with endgap_ref's result."""
    return [(xy, eg.align_profiles_np(*xy, posgap=posgap)) for xy, _ in pgc.tall_cases()]


def check_tall(be, posgap, **kw):
    cases = tall_cases(posgap)
    assert {x.shape[0] for (x, _), _ in cases} == set(pgc.TALL_ROWS)
    got = sa.merge_profiles(be, [xy for xy, _ in cases], position_gaps=posgap, free_end_gaps=True, **kw)
    for ((x, y), want), (ops, score) in zip(cases, got):
        assert (ops.decode(), score) == want, (x.shape, y.shape)


# ---- 3. band: the entries on explicit tables
def tables(be, pairs, posgap):
    """The column tables of the pairs as _prog_pairs lays them out: Y as kind 2 (7 planes) for the opens by occupancy, as kind 0."""
    return (pgc.Tables if posgap else pbc.Tables)(be, pairs)


def _run(t, call, need, rows):
    be, n = t.be, t.n
    ops_bytes = int((t.WX + t.WY).sum())
    d_ws, d_ops, d_out = be.empty(4 * int(need.sum())), be.empty(ops_bytes), be.empty(12 * n)
    d_pairs = be.upload(rows)
    be.call(call, be.ptr(t.d_cols), be.ptr(t.d_leaves), n, be.ptr(t.d_cols), t.words, be.ptr(d_pairs), n, be.ptr(d_ws), int(need.sum()),
            be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
    res = be.download(d_out, np.int32, 3 * n).reshape(-1, 3)
    assert not res[:, 0].any(), res[:, 0]
    ops = be.download(d_ops, np.uint8, ops_bytes)
    return [(ops[o:o + k][::-1].tobytes().decode(), int(s)) for o, k, s in zip(t.ops_off, res[:, 2], res[:, 1])]


def banded(t, bands, posgap):
    """Every pair of the tables over its (dlo, dhi), one launch of the banded entry: [(ops forward, score)]."""
    dlo, dhi = np.array([b[0] for b in bands], np.int64), np.array([b[1] for b in bands], np.int64)
    need = pa.band_workspace_words(t.WX, t.WY, np.maximum(dlo, -t.WX), np.minimum(dhi, t.WY))
    return _run(t, entry(posgap, True), need, t.pair_rows(np.arange(t.n), dlo, dhi, sa.exclusive_sum(need)))


def full(t, posgap):
    need = pa.workspace_words_v(t.WX, t.WY)
    z = np.zeros(t.n)
    return _run(t, entry(posgap), need, t.pair_rows(np.arange(t.n), z, z, sa.exclusive_sum(need))[:, :sa.PG_PAIR_FIELDS])


def widths(t, idx, S0):
    """mprg_prog_band_widths_endgap for the pairs idx (repeats allowed) with the pass-1 scores S0: (SB', w*) per entry."""
    be, m = t.be, len(idx)
    out = np.zeros((m, 3), np.int32)
    out[:, 1] = S0
    d_bounds, d_status = be.empty(16 * m), be.empty(4 * m)
    z = np.zeros(m, np.int64)
    d_pairs, d_out = be.upload(t.pair_rows(idx, z, z)), be.upload(out)
    be.call("mprg_prog_band_widths_endgap", be.ptr(t.d_cols), be.ptr(t.d_leaves), t.n, be.ptr(t.d_cols), t.words, be.ptr(d_pairs), m,
            be.ptr(d_out), be.ptr(d_bounds), be.ptr(d_status), be.stream)
    assert not be.download(d_status, np.int32, m).any()
    return be.download(d_bounds, np.int64, 2 * m).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def kernel_cases(posgap):
    """((X, Y), (dlo, dhi), endgap_ref's banded (ops, score), the full DP's score): progband_common.kernel_cases' pairs and bands;
    then bands in which only some rows reach column C, in which the last row lies only partly inside, and that touch either corner
    with no room (the exact corridor) on a pair whose optimum wants a free run."""
    out = [(xy, b) for xy, b, _, _ in pbc.kernel_cases()]
    rng = random.Random(37)
    for k, (n, C, lo, hi) in enumerate(((100, 130, 0, 0), (100, 130, 5, 0), (130, 100, 0, 0), (130, 100, 0, 7), (70, 200, 3, 3),
                                        (200, 70, 3, 3), (65, 65, 0, 0), (129, 130, 64, 1), (64, 130, 1, 64), (128, 63, 2, 2))):
        X = tuple(pr.random_profiles(rng, pc.ROWS[k % 4], n, (0.1, 0.6)[k % 2], amb=0.05))
        Y = tuple(pr.random_profiles(rng, pc.ROWS[(k + 2) % 4], C, (0.1, 0.3)[k % 2], amb=0.05))
        out.append(((X, Y), (min(0, C - n) - lo, max(0, C - n) + hi)))
    frag = extra_pairs()[len(LAST_ROWS) * len(LAST_COLS):][:7]
    out += [(xy, (min(0, len(xy[1][0]) - len(xy[0][0])) - w, max(0, len(xy[1][0]) - len(xy[0][0])) + w)) for xy in frag for w in (0, 9)]
    return [(xy, b, eg.align_profiles_banded_np(*xy, *b, posgap), eg.align_profiles_np(*xy, posgap=posgap)[1]) for xy, b in out]


def check_kernel(be, posgap):
    cases = kernel_cases(posgap)
    shape = lambda xy: (len(xy[0][0]), len(xy[1][0]))      # noqa: E731
    clamped = [br.clamp(*shape(xy), *b) for xy, b, _, _ in cases]
    # column C reached by only some rows (the rows above n - (C - dhi) do not reach it), the last row partly inside (its first
    # columns lie below dlo), both corners with no room beside them
    assert sum(0 < hi < shape(xy)[1] and shape(xy)[1] - hi < shape(xy)[0] for (xy, _, _, _), (lo, hi) in zip(cases, clamped)) >= 8
    assert sum(-shape(xy)[0] < lo and shape(xy)[0] + lo > 0 for (xy, _, _, _), (lo, hi) in zip(cases, clamped)) >= 8
    assert sum((lo, hi) == (min(0, shape(xy)[1] - shape(xy)[0]), max(0, shape(xy)[1] - shape(xy)[0])) for (xy, _, _, _), (lo, hi) in zip(cases, clamped)) >= 8
    assert sum(want[1] < whole for _, _, want, whole in cases) >= 8 and any(want[1] == whole for _, _, want, whole in cases)
    t = tables(be, [xy for xy, _, _, _ in cases], posgap)
    for (xy, b, want, _), g in zip(cases, banded(t, [b for _, b, _, _ in cases], posgap)):
        assert g == want, (shape(xy), len(xy[0]), len(xy[1]), b)
    for (xy, _, _, whole), g in zip(cases, full(t, posgap)):                # the full entry over the same tables
        assert g[1] == whole


# ---- 4. the widths kernel against the linear search
@functools.lru_cache(maxsize=None)
def width_cases():
    """progband_common.width_cases' pairs, then Y's with many columns of B_j <= 0 (all gaps but an ambiguity code, or N alone): while
    there are more of them than k, U(w) = SB'; the last Y has no other column, so U(w) = SB' = 0 for every w and w* = min(n, C) for
    every S0 <= 0."""
    rng = random.Random(41)
    out = list(pbc.width_cases())
    for n, C, dead in ((30, 40, 36), (40, 30, 25), (12, 60, 58), (20, 25, 25)):
        X = tuple(pr.random_profiles(rng, 2, n, 0.1))
        cols = ["A" * 3] * (C - dead) + [rng.choice(["N--", "NNN", "-N-", "RY-"]) for _ in range(dead)]
        rng.shuffle(cols)
        out.append((X, tuple("".join(c[r] for c in cols) for r in range(3))))
    return out


def check_widths(be):
    cases = width_cases()
    idx, S0, want = [], [], []
    flat = all_dead = 0
    for k, (X, Y) in enumerate(cases):
        n, C = len(X[0]), len(Y[0])
        SB, loss = eg.bounds(X, Y)
        assert 0 <= loss[0] and loss[-1] <= 1280 and SB == sum(loss)
        top = min(n, C)
        dead = [w for w in range(top + 1) if max(0, C - n) + w + 1 <= loss.count(0)]      # more dead columns than k
        assert all(eg.U(SB, loss, n, C, w) == SB for w in dead)
        flat += len(dead) >= 10
        if loss.count(0) == C:
            all_dead += 1
            assert SB == 0 and eg.wstar(SB, loss, n, C, 0) == eg.wstar(SB, loss, n, C, -1) == top and eg.wstar(SB, loss, n, C, 1) == 0
        scores = {SB + 5000, SB, SB - 1, -10 ** 8}
        for w in sorted({0, 1, 2, 3, top // 3, top // 2, top - 2, top - 1, top} & set(range(top + 1))):
            u = eg.U(SB, loss, n, C, w)
            scores |= {u - 1, u, u + 1}                         # at, one below and one above the threshold
        for s in sorted(scores):
            idx.append(k)
            S0.append(s)
            want.append((SB, eg.wstar(SB, loss, n, C, s)))
    assert flat >= 4 and all_dead >= 1 and len({w for _, w in want}) >= 30, (flat, all_dead, len({w for _, w in want}))
    for posgap in (False, True):                                # a profile of kind 0, a profile of kind 2: the same answers
        got = widths(tables(be, cases, posgap), idx, S0)
        for k, s, w, g in zip(idx, S0, want, got.tolist()):
            assert tuple(g) == w, (k, s, posgap)


# ---- 5. two passes
@functools.lru_cache(maxsize=None)
def two_pass_cases(posgap):
    """dp_cases, progband_common.related_cases' sides, and near-identical sides that the weaker bound still certifies in pass 1."""
    rng = random.Random(43)
    near = []
    for L, m, cut in ((120, 4, 0), (200, 5, 0), (90, 3, 0), (150, 4, 40)):
        _, seqs = _family(rng, L, m, 0.004, 0.0)
        near.append((tuple(pr.progressive_rows([s[cut:] for s in seqs[:m // 2]])), tuple(pr.progressive_rows(seqs[m // 2:]))))
    pairs = [xy for xy, _ in dp_cases(posgap)] + [xy for xy, _ in pbc.related_cases()] + near
    return [(xy, eg.align_profiles_np(*xy, posgap=posgap)) for xy in pairs]


@functools.lru_cache(maxsize=None)
def two_pass_spec(posgap):
    """The reference's (kind, cells) per merge of two_pass_cases with W0 and the new U, and the merges' (n, C)."""
    cases = two_pass_cases(posgap)
    res = [eg.two_pass(X, Y, W0, posgap) for (X, Y), _ in cases]
    assert [r for r, _, _ in res] == [w for _, w in cases]      # the reference's own two passes give the unbanded result
    return [(k, c) for _, k, c in res], [(len(X[0]), len(Y[0])) for (X, Y), _ in cases]


def check_two_pass_merges(be, posgap):
    cases = two_pass_cases(posgap)
    log, sizes = two_pass_spec(posgap)
    kinds = Counter(k for k, _ in log)
    assert kinds["first"] >= 2 and kinds["second"] >= 2 and kinds["full"] >= 2, kinds
    pairs = [(pc.codes(x), pc.codes(y)) for (x, y), _ in cases]
    small = 4 * int(max(pa.workspace_words(n, C) for n, C in sizes))         # the largest full DP alone: every pass in several launches
    from tests import progband_ref as pbr
    for budget in (pa.DEFAULT_BUDGET_BYTES, small):
        counters = {}
        got = sa.merge_profiles(be, pairs, budget_bytes=budget, band=W0, counters=counters, position_gaps=posgap, free_end_gaps=True)
        for ((x, y), want), (ops, score) in zip(cases, got):
            assert (ops.decode(), score) == want, (len(x), len(x[0]), len(y), len(y[0]))
        assert {k: v for k, v in counters.items() if k.startswith("prog_band_")} == pbr.counters(log, sizes)
        assert counters["free_end_gap_merges"] == len(cases) and counters.get("position_gap_merges", 0) == (len(cases) if posgap else 0)
    check_dp(be, posgap, band=True)                             # the default w0
    check_tall(be, posgap, band=True)


# ---- 6. whole MSAs
@functools.lru_cache(maxsize=None)
def msa_spec(posgap):
    return [eg.progressive(l, posgap) for l in pc.msa_loci()]


def check_msas(be, posgap, **kw):
    loci, info = pc.msa_loci(), []
    timings = {}
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, position_gaps=posgap, free_end_gaps=True, progression=info,
                        timings=timings, **kw)
    changed = 0
    old = pgc.msa_spec() if posgap else pc.msa_spec()
    for l, m, got, (rows, want), (before, _) in zip(loci, msas, info, msa_spec(posgap), old):
        assert m.rows_as_strings() == rows, l
        assert got == want, l
        pgc.invariants(l, rows)
        changed += rows != before
    assert changed >= 5 and timings["free_end_gap_merges"] > 0
    return msas


def check_same_bytes(be, posgap):
    base = [m.rows_as_strings() for m in check_msas(be, posgap)]
    for kw in (dict(band=W0), dict(band=True, device_tree=True), dict(device_tree=True, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)):
        assert [m.rows_as_strings() for m in check_msas(be, posgap, **kw)] == base, kw


def check_flag_off(be):
    """Without the flag the bytes are prog_ref's (posgap_ref's with position_gaps), as today, and False is no flag."""
    loci = pc.msa_loci()
    for kw, spec in ((dict(), pc.msa_spec()), (dict(free_end_gaps=False), pc.msa_spec()), (dict(position_gaps=True, free_end_gaps=False), pgc.msa_spec())):
        timings = {}
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, timings=timings, **kw)
        assert [m.rows_as_strings() for m in msas] == [rows for rows, _ in spec]
        assert "free_end_gap_merges" not in timings


def check_refine_afterwards(be, posgap):
    """refine = 2 after the flag: refine_ref (charged ends, the fixed open) on the new rows."""
    loci = pr.table_loci()[:8]
    info = []
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, position_gaps=posgap, free_end_gaps=True, refine=2, refinement=info)
    for l, m, got in zip(loci, msas, info):
        rows, acc, trail = rr.refine_rows(eg.progressive_rows(l, posgap), 2)
        assert m.rows_as_strings() == rows and got == (acc, trail[0], trail[-1])
    assert any(a for a, _, _ in info)


def large_locus():
    """Twelve records over four alleles: with large_loci and max_leaves = 4 it is built progressively over its four classes."""
    alleles = pr.clade_locus(7, 4)
    return [alleles[(5 * i) % 4] for i in range(12)]


@functools.lru_cache(maxsize=None)
def composition_spec(posgap):
    """Per flag the reference composition's rows of posgap_common.composition_loci (large_loci: of large_locus), every merge with
    free end gaps (endgap_ref.in_compositions)."""
    from tests import retree_ref as rt
    from tests import treerefine_ref as tf
    from tests import weights_ref as wr
    loci = pgc.composition_loci()
    with eg.in_compositions(posgap):
        return dict(collapse=[cr.progressive(l)[0] for l in loci], seq_weights=[wr.progressive(l)[0] for l in loci],
                    retree=[rt.progressive(l, 1)[0] for l in loci], refine_tree=[tf.progressive(l, 1)[0] for l in loci],
                    large_loci=[cr.progressive(large_locus())[0]])


def check_compositions(be, posgap):
    loci = pgc.composition_loci()
    spec = composition_spec(posgap)
    plain = [eg.progressive_rows(l, posgap) for l in loci]
    for key, kw in (("collapse", dict(collapse=True)), ("seq_weights", dict(seq_weights=True)), ("retree", dict(retree=1)),
                    ("refine_tree", dict(refine_tree=1))):
        msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, position_gaps=posgap, free_end_gaps=True, **kw)
        got = [m.rows_as_strings() for m in msas]
        assert got == spec[key], key
        assert got != plain or key == "collapse", key            # (the stage did something on these loci)
        for l, rows in zip(loci, got):
            pgc.invariants(l, rows)
    big, info = large_locus(), []
    kw = dict(progressive=True, collapse=True, max_leaves=4, position_gaps=posgap, free_end_gaps=True, progression=info)
    m, = sa.star_msas(be, [pc.records(big)], large_loci=True, **kw)
    assert info[0][0] == 4 and not info[0][2], info                           # four leaves, built progressively
    assert m.rows_as_strings() == spec["large_loci"][0]
    pgc.invariants(big, m.rows_as_strings())
    info.clear()
    m, = sa.star_msas(be, [pc.records(big)], **kw)                            # without large_loci the locus is left to the star pass
    assert info[0][2] and m.rows_as_strings() != spec["large_loci"][0]


# ---- 7. the finding
# shared pairs with the truth of fragment_locus(seed, 20, 250, 350), seeds 0-3: (fixed open, + free end gaps, opens by occupancy,
# + free end gaps), as the references give them; and the truth's own pairs
FINDING = ((36431, 38008, 36221, 38073), (38832, 39335, 38914, 39417), (28004, 29838, 27605, 29910), (41136, 41555, 41294, 41713))
FINDING_TRUTH = (39388, 41104, 32334, 43872)


@functools.lru_cache(maxsize=None)
def finding():
    """Per locus: (sequences, true rows, (prog_ref's rows, endgap_ref's, posgap_ref's, endgap_ref's with the opens by occupancy))."""
    out = []
    for seed in range(4):
        seqs, truth = fragment_locus(seed, 20, 250, 350)
        out.append((seqs, truth, (pr.progressive_rows(seqs), eg.progressive_rows(seqs, False), pg.progressive_rows(seqs),
                                  eg.progressive_rows(seqs, True))))
    return out


def check_finding_reference():
    got = tuple(tuple(cmp.by_histogram(rows, truth)[0] for rows in forms) for _, truth, forms in finding())
    print("shared pairs (fixed, + free ends, by occupancy, + free ends):", got)
    assert tuple(cmp.by_histogram(truth, truth)[0] for _, truth, _ in finding()) == FINDING_TRUTH
    assert all(f[1] > f[0] and f[3] > f[2] for f in got)
    assert got == FINDING
    for seqs, truth, _ in finding():
        assert [r.replace("-", "") for r in truth] == seqs and sum(len(s) < 200 for s in seqs) >= 2


def check_finding(be):
    loci = finding()
    recs = [pc.records(s) for s, _, _ in loci]
    for k, kw in enumerate((dict(), dict(free_end_gaps=True), dict(position_gaps=True), dict(position_gaps=True, free_end_gaps=True))):
        msas = sa.star_msas(be, recs, progressive=True, band=True, device_tree=True, **kw)
        assert [m.rows_as_strings() for m in msas] == [forms[k] for _, _, forms in loci], kw


# ---- 8. status codes
def check_abi_statuses(be):
    """The five new entries, handed tables that point outside a buffer, report their status code and write nothing else
    (posgap_common.check_abi_statuses' pattern, on its tables: Y's 7 planes of 5 columns at 0, X's 7 of 4 at 35; the entries with
    the fixed open read the first six of Y's)."""
    POISON = 0x5C
    X, Y = ("AC-T", "A-GT"), ("ACGTA", "AC-TA", "ACGTN")
    t = pgc.Tables(be, [(X, Y)])
    d_cols, WORDS = t.d_cols, 35 + 28
    assert t.words == WORDS and t.xcol.tolist() == [35]

    def untouched(buf, n):
        return (be.download(buf, np.uint8, n) == POISON).all()
    full_need, band_need = int(pa.workspace_words(4, 5)), int(pa.band_workspace_words(4, 5, -4, 5))

    def pairs(call, pair, need, leaf=(0, 3, 5, 0), xwords=WORDS, ws_words=None, ops_bytes=9):
        d_ws, d_ops, d_out = be.full(4 * need, POISON), be.full(9, POISON), be.full(12, POISON)
        d_leaves, d_pairs = be.upload(np.array([leaf], np.int64)), be.upload(np.array([pair], np.int64))
        be.call(call, be.ptr(d_cols), be.ptr(d_leaves), 1, be.ptr(d_cols), xwords, be.ptr(d_pairs), 1, be.ptr(d_ws),
                need if ws_words is None else ws_words, be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
        return be.download(d_out, np.int32, 3).tolist(), untouched(d_ops, 9) and untouched(d_ws, 4 * need), be.download(d_ops, np.uint8, 9)
    for posgap in (False, True):
        want = eg.align_profiles(X, Y, posgap)
        assert want[1] == eg.overlap_score(X, Y, posgap)
        for call, need, band in ((entry(posgap), full_need, []), (entry(posgap, True), band_need, [-4, 5])):
            out, clean, ops = pairs(call, [0, 35, 4, 0, 0, 2] + band, need)
            assert out == [0, want[1], len(want[0])] and ops[:out[2]][::-1].tobytes().decode() == want[0] and not clean
            out, _, ops = pairs(call, [0, 35, 0, 0, 0, 2] + ([0, 5] if band else []), need)      # n = 0: C D ops, score 0
            assert out == [0, 0, 5] and ops[:5].tobytes() == b"DDDDD"
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
            assert pairs(entry(posgap, True), [0, 35, 4, 0, 0, 2] + band, band_need)[:2] == ([3, 0, 0], True)
        ref = eg.align_profiles_banded(X, Y, -1, 2, posgap)
        out, _, ops = pairs(entry(posgap, True), [0, 35, 4, 0, 0, 2, -1, 2], band_need)
        assert out == [0, ref[1], len(ref[0])] and ops[:out[2]][::-1].tobytes().decode() == ref[0]

    def widths_call(pair, out=(0, 0, 0), leaf=(0, 3, 5, 0), xwords=WORDS):
        d_bounds, d_status = be.full(16, POISON), be.full(4, POISON)
        d_leaves, d_pairs = be.upload(np.array([leaf], np.int64)), be.upload(np.array([pair], np.int64))
        d_out = be.upload(np.array(out, np.int32))
        be.call("mprg_prog_band_widths_endgap", be.ptr(d_cols), be.ptr(d_leaves), 1, be.ptr(d_cols), xwords, be.ptr(d_pairs), 1,
                be.ptr(d_out), be.ptr(d_bounds), be.ptr(d_status), be.stream)
        return be.download(d_status, np.int32, 1).tolist(), untouched(d_bounds, 16), be.download(d_bounds, np.int64, 2).tolist()
    b = eg.bounds(X, Y)
    for s in (eg.align_profiles(X, Y)[1], b[0] - 3000, b[0]):
        assert widths_call([0, 35, 4, 0, 0, 2, 0, 0], (0, s, 0)) == ([0], False, [b[0], eg.wstar(*b, 4, 5, s)])
    for pair, kw, code in (([1, 35, 4, 0, 0, 2, 0, 0], {}, 3), ([-1, 35, 4, 0, 0, 2, 0, 0], {}, 3), ([0, 35, -1, 0, 0, 2, 0, 0], {}, 3),
                           ([0, 35, 4, 0, 0, 0, 0, 0], {}, 3), ([0, 35, 4, 0, 0, (1 << 20) + 1, 0, 0], {}, 3),
                           ([0, 35, 4, 0, 0, 2, 0, 0], dict(leaf=(0, 0, 5, 0)), 3), ([0, 35, 4, 0, 0, 2, 0, 0], dict(leaf=(0, 3, 0, 0)), 3),
                           ([0, 35, 4, 0, 0, 2, 0, 0], dict(out=(2, 0, 0)), 3),                           # pass 1 refused the merge
                           ([0, 36, 4, 0, 0, 2, 0, 0], {}, 2), ([0, -1, 4, 0, 0, 2, 0, 0], {}, 2), ([0, 35, 4, 0, 0, 2, 0, 0], dict(xwords=WORDS - 1), 2),
                           ([0, 35, 999_996, 0, 0, 2, 0, 0], {}, 1)):
        assert widths_call(pair, **kw)[:2] == ([code], True), (pair, kw)


# ---- 9. the command line
def cli_loci():
    """A table locus and a small locus with partial records."""
    return [pr.table_loci()[0], fragment_locus(5, 7, 120, 160, share=0.7)[0]]


def check_cli(be, tmp_path, caplog):
    """from_msa.run with --unaligned --progressive --free-end-gaps --msa-dir (in process): the files are endgap_ref's and the log has
    the flag's line; without the flag the files are prog_ref's and the line is absent."""
    import logging
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    loci = cli_loci()
    recs =[[(f"s{i} x", s) for i, s in enumerate(l)] for l in loci]
    for k, r in enumerate(recs):
        (src / f"g{k}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in r))
    old = {f"g{k}.fa": pr.progressive_fasta(r) for k, r in enumerate(recs)}
    merges = sum(len(l) - 1 for l in loci)

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None, progressive=True)
        base.update(kw)
        return Namespace(**base)
    for flag, posgap in ((True, False), (True, True), (False, False)):
        caplog.clear()
        d = tmp_path / f"msas{flag}{posgap}"
        with caplog.at_level(logging.INFO):
            from_msa.run(opts(output_prefix=str(tmp_path / f"o{flag}{posgap}" / "a"), msa_dir=str(d), free_end_gaps=flag, position_gaps=posgap), be)
        got = {p.name: p.read_text() for p in d.iterdir()}
        lines = [r.getMessage() for r in caplog.records if "--free-end-gaps:" in r.getMessage()]
        if flag:
            want = {f"g{k}.fa": eg.progressive_fasta(r, posgap) for k, r in enumerate(recs)}
            assert got == want and got != old and len(lines) == 1 and f"--free-end-gaps: {merges} merges" in lines[0]
        else:
            assert got == old and not lines


def check_parser(capsys):
    """--free-end-gaps without --progressive is a parser error."""
    import pytest
    from make_prg_amd import __main__ as cli
    with pytest.raises(SystemExit) as exc:
        cli.main(["from_msa", "-i", "x", "-o", "y", "--unaligned", "--free-end-gaps"])
    assert exc.value.code == 2 and "--free-end-gaps needs --progressive" in capsys.readouterr().err
