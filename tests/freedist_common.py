"""The checks of `from_msa --unaligned --progressive --pair-distances --free-end-distances` (make_prg_amd/from_msa/star_align.py,
"Free end distances"; csrc/al_scores.inc, csrc/al_scores_band.inc), for any backend: tests/test_freedist_emulated.py runs them on the
CPU emulation build, tests/test_gpu_freedist.py on the MI355X.  The statement (tests/freedist_ref.py) against itself and against the
finding's table; mprg_align_pair_scores_endgap and mprg_align_pair_scores_endgap_banded called directly against
tests/freepairs_ref.py's DPs, against mprg_align_pairs_endgap on the same tables and against the charged kernels (pairdist_common's
shapes around the 64-row strip and the 128-column ring, guard words around every buffer), their refusals, the host's two passes, whole
MSAs with the other flags, what moves, and the command line."""
import functools
import random

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from make_prg_amd.utils.synthetic import fragment_locus
from tests import band_ref as br
from tests import compare_ref as cmp
from tests import endgap_common as egc
from tests import freedist_ref as fd
from tests import freepairs_ref as fp
from tests import pairdist_common as pdc
from tests import pairdist_ref as pd
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import star_ref as sr
from tests import star_trace as tr
from tests import strand_ref as st

FULL, BANDED = "mprg_align_pair_scores_endgap", "mprg_align_pair_scores_endgap_banded"
FREE, CHARGED = (FULL, BANDED), (pdc.FULL, pdc.BANDED)
PAIRS = ("mprg_align_pairs_endgap", "mprg_align_pairs_endgap_banded")
GUARD32, POISON_TAB = pdc.GUARD32, pdc.POISON_TAB
Batch, guards_hold, check_tab, seq_codes = pdc.Batch, pdc.guards_hold, pdc.check_tab, pdc.seq_codes


# ---- 1. the statement against itself
def check_statement():
    """The four facts on pairdist_ref's 300 pairs, ambiguity codes included, and free=False is pairdist_ref's score."""
    pairs = pd.random_pairs(3)
    assert len(pairs) == 300 and sum(1 for a, b in pairs if set(a + b) - set("ACGT")) >= 80
    above = 0
    for a, b in pairs:
        s = fd.score(a, b)
        assert s == fd.score(b, a), (a, b)
        assert s % 64 == 0, (a, b, s)
        assert 0 <= s <= 1280 * min(pd.acgt(a), pd.acgt(b)), (a, b, s)
        assert s >= pd.score(a, b) == fd.score(a, b, False), (a, b, s)
        assert 0 <= fd.shared(a, b) <= min(pd.MATCH * pd.acgt(a), pd.MATCH * pd.acgt(b))
        above += s > pd.score(a, b)
    assert above >= 150 and any(fd.score(a, b) == 0 for a, b in pairs)


def check_substrings():
    """An ACGT-only record that is an exact substring of another, cut from the front, the middle or the end: s'' = nw'' of the shorter,
    D'' = 0; with charged ends it is far away."""
    rng = random.Random(83)
    for L, cuts in ((150, ((0, 30), (40, 100), (110, 150))), (70, ((0, 64), (5, 70), (33, 34))), (300, ((0, 90), (100, 165), (236, 300)))):
        root = "".join(rng.choice("ACGT") for _ in range(L))
        for a, b in cuts:
            piece = root[a:b]
            assert fd.score(piece, root) == fd.score(root, piece) == 1280 * len(piece)
            nw = pd.MATCH * len(piece)
            assert fd.shared(piece, root) == nw and pd.distance(fd.shared(piece, root), nw, pd.MATCH * L) == 0
            assert fd.distances([root, piece], [0, 1])[0][1] == 0 < fd.distances([root, piece], [0, 1], free=False)[0][1]


# the issue's table: per seed of fragment_locus(seed, 20, 250, 350) every fragment's D'' to its nearest full-length record with
# charged ends and with free ends, and the median full-full D'' of either form
TABLE = (((34362, 28368, 65536, 53248, 44103, 65536), (13502, 12285, 9988, 12115, 11604, 13441), (13778, 13778)),
         ((61027, 55582, 42576), (7949, 9615, 14587), (15393, 15381)),
         ((46301, 65536, 65536, 65536, 51187, 29434), (14684, 16869, 9120, 23006, 16411, 13568), (15666, 15452)),
         ((26230, 65536, 65536), (14815, 9020, 8946), (14333, 14194)))


@functools.lru_cache(maxsize=None)
def fragment_loci():
    return [fragment_locus(seed, 20, 250, 350) for seed in range(4)]


def check_table():
    """The finding's table from the statement alone; every fragment nearer than with charged ends and nearer than twice the median
    distance of two full-length records; the merge lists of the two forms differ in all four loci."""
    for (seqs, _), (want_charged, want_free, want_median) in zip(fragment_loci(), TABLE):
        charged, m_charged = fd.nearest_full(seqs, False)
        free, m_free = fd.nearest_full(seqs, True)
        print("charged:", charged, "free:", free, "median full-full:", (m_charged, m_free))
        assert 3 <= len(free) <= 6
        assert all(f < c and f < 2 * m_free for f, c in zip(free, charged))
        assert max(free) <= 23006 < 2 * m_free
        assert (tuple(charged), tuple(free), (m_charged, m_free)) == (want_charged, want_free, want_median)
        assert fd.merges(seqs, True) != fd.merges(seqs, False)


# ---- 2., 3. the kernels against the DPs
def launch(be, b: Batch, entries=FREE, ptab=None, n_leaves=None, ws_words=None, tab_words=None):
    """pairdist_common.launch for the entries given: (status per pair, score per pair, the table, the workspace with its front
    guard, the pairs' offsets and needs); the guard words of `out` and of the table are asserted here."""
    table, need, total = b.table()
    ptab = table if ptab is None else ptab
    assert ptab.shape[1] == (sa.AL_SCORE_PAIR_FIELDS if b.bands is None else sa.AL_SCORE_BAND_PAIR_FIELDS)
    d_leaves, d_prof, keep = pdc.profiles(be, b)
    n = len(ptab)
    d_ws = be.upload(np.full(64 + total, GUARD32, np.int32))
    d_out = be.upload(np.full(2 * n + 4, GUARD32, np.int32))
    d_tab = be.upload(np.full(b.tab_words + 4, POISON_TAB, np.uint32))
    d_seqs, d_pairs = be.upload(b.seqbuf), be.upload(ptab)
    be.call(entries[0] if b.bands is None else entries[1], be.ptr(d_prof), be.ptr(d_leaves), len(b.leaf_tab) if n_leaves is None else n_leaves,
            be.ptr(d_seqs), be.ptr(d_pairs), n, be.ptr(d_ws) + 256, total if ws_words is None else ws_words, be.ptr(d_tab) + 8,
            b.tab_words if tab_words is None else tab_words, be.ptr(d_out) + 8, be.stream)
    out = be.download(d_out, np.int32, 2 * n + 4)
    tab = be.download(d_tab, np.uint32, b.tab_words + 4)
    ws = be.download(d_ws, np.int32, 64 + total)
    assert (out[:2] == GUARD32).all() and (out[-2:] == GUARD32).all(), "a word beside out was written"
    assert (tab[:2] == POISON_TAB).all() and (tab[-2:] == POISON_TAB).all(), "a word beside the table was written"
    res = out[2:-2].reshape(-1, 2)
    return res[:, 0].tolist(), res[:, 1].tolist(), tab[2:-2], ws, table[:, 3], need


def traceback_scores(be, b: Batch):
    """mprg_align_pairs_endgap (or _endgap_banded) on the same leaves, sequences and bands: (status, score) per pair."""
    d_leaves, d_prof, keep = pdc.profiles(be, b)
    pc_ = b.C[b.pl]
    if b.bands is None:
        words = pa.workspace_words(b.pn, pc_)
    else:
        lo, hi = np.maximum(b.bands[:, 0], -b.pn), np.minimum(b.bands[:, 1], pc_)
        words = pa.band_workspace_words(b.pn, pc_, lo, hi)
    ops_off, ops_bytes = sa.exclusive_sum(b.pn + pc_), int((b.pn + pc_).sum())
    cols = [b.pl, b.soff, b.pn, sa.exclusive_sum(words), ops_off] + ([] if b.bands is None else [b.bands[:, 0], b.bands[:, 1]])
    d_pairs, d_seqs = be.upload(np.stack(cols, 1).astype(np.int64)), be.upload(b.seqbuf)
    d_ws, d_ops, d_out = be.empty(4 * int(words.sum())), be.empty(ops_bytes), be.empty(12 * len(b.pl))
    be.call(PAIRS[0] if b.bands is None else PAIRS[1], be.ptr(d_prof), be.ptr(d_leaves), len(b.leaf_tab), be.ptr(d_seqs),
            be.ptr(d_pairs), len(b.pl), be.ptr(d_ws), int(words.sum()), be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
    res = be.download(d_out, np.int32, 3 * len(b.pl)).reshape(-1, 3)
    return res[:, 0].tolist(), res[:, 1].tolist()


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """pairdist_common.kernel_cases' leaves and pairs (leaves of 1 and 3 rows, C and n over 1, 63, 64, 65, 127, 128, 129, 200 and
    n = 0, a pair count that is no multiple of 4) with freepairs_ref's scores."""
    leaves, pairs, charged = pdc.kernel_cases()
    assert len(pairs) % 4 and {len(l) for l in leaves} == {1, 3}
    assert {len(s) for _, s in pairs} == {0, 70} | set(pdc.SIZES) and {len(l[0]) for l in leaves} == set(pdc.SIZES)
    want = [fp.align_pair_np(leaves[l], s)[1] for l, s in pairs]
    assert all(w == 0 for w, (_, s) in zip(want, pairs) if not s)
    return leaves, pairs, want, charged


def check_kernel(be):
    leaves, pairs, want, charged = kernel_cases()
    b = Batch(leaves, pairs, dst=pdc.scattered_dst(len(pairs)))
    assert (b.dst[::7] == -1).all() and len(set(b.dst[b.dst >= 0].tolist())) == (b.dst >= 0).sum()
    status, score, tab, ws, ws_off, need = launch(be, b)
    assert status == [0] * len(pairs)
    bad = [k for k in range(len(pairs)) if score[k] != want[k]]
    assert not bad, [(k, pairs[k][0], len(pairs[k][1]), score[k], want[k]) for k in bad[:5]]
    assert traceback_scores(be, b) == (status, score)               # the forms agree
    old = launch(be, b, CHARGED)[1]
    assert old == charged and all(s >= o for s, o in zip(score, old))
    assert 2 * sum(s != o for s, o in zip(score, old)) >= len(pairs)        # (this test does not pass on the charged kernel)
    check_tab(tab, b.dst, status, score)
    assert min(score) == 0 and any(s > 0 for s in score) and (tab == POISON_TAB).sum() > 5
    guards_hold(ws, ws_off, need)


def certified(rows, s, dlo, dhi, S0):
    """The statement certifies the band: it is the whole matrix, or U at the smaller of its two half-widths is below S0."""
    n, C = len(s), len(rows[0])
    if br.clamp(n, C, dlo, dhi) == (-n, C):
        return True
    w = min(min(0, C - n) - dlo, dhi - max(0, C - n))
    return fp.wstar(*fp.bounds(rows), n, C, S0) <= w


@functools.lru_cache(maxsize=None)
def banded_cases():
    """kernel_cases' pairs, each with a band from pairdist_common.HALF_WIDTHS in turn (unclamped: the kernel clamps at -n and at C);
    freepairs_ref's banded score, and whether the statement certifies the band."""
    leaves, pairs, full, _ = kernel_cases()
    bands, want, cert = [], [], []
    for k, (l, s) in enumerate(pairs):
        n, C = len(s), len(leaves[l][0])
        wm, wp = pdc.HALF_WIDTHS[k % len(pdc.HALF_WIDTHS)]
        dlo, dhi = min(0, C - n) - wm, max(0, C - n) + wp
        bands.append((dlo, dhi))
        want.append(fp.align_pair_banded_np(leaves[l], s, dlo, dhi)[1])
        cert.append(certified(leaves[l], s, dlo, dhi, want[-1]))
    return bands, want, cert


def check_banded_conditions():
    """The conditions on the banded test's input, by the statement alone."""
    leaves, pairs, full, _ = kernel_cases()
    bands, want, cert = banded_cases()
    shapes = [(len(s), len(leaves[l][0])) for l, s in pairs]
    assert {np.sign(C - n) for n, C in shapes} == {-1, 0, 1}
    assert any(lo < -n for (lo, hi), (n, C) in zip(bands, shapes)) and any(hi > C for (lo, hi), (n, C) in zip(bands, shapes))
    assert any(lo == min(0, C - n) and hi == max(0, C - n) for (lo, hi), (n, C) in zip(bands, shapes))          # w = 0
    assert all(want[k] == full[k] for k in range(len(pairs)) if cert[k])
    print("certified:", sum(cert), "banded below full:", sum(w < f for w, f in zip(want, full)))
    assert sum(cert) >= 40 and sum(w < f for w, f in zip(want, full)) >= 10
    assert all(w <= f for w, f in zip(want, full))


def check_banded_kernel(be):
    leaves, pairs, full, _ = kernel_cases()
    bands, want, cert = banded_cases()
    check_banded_conditions()
    shapes = [(len(s), len(leaves[l][0])) for l, s in pairs]
    b = Batch(leaves, pairs, bands=bands, dst=pdc.scattered_dst(len(pairs)))
    status, score, tab, ws, ws_off, need = launch(be, b)
    assert status == [0] * len(pairs)
    bad = [k for k in range(len(pairs)) if score[k] != want[k]]
    assert not bad, [(k, shapes[k], bands[k], score[k], want[k]) for k in bad[:5]]
    assert all(score[k] == full[k] for k in range(len(pairs)) if cert[k])
    assert traceback_scores(be, b) == (status, score)
    check_tab(tab, b.dst, status, score)
    guards_hold(ws, ws_off, need)


# ---- 4. the refusals
def check_refusals(be):
    """pairdist_common.check_refusals' cases on the two new entries: one pair of three bad, one way at a time: its status is the
    header's, nothing of it is written (score 0, its table entry and its row buffer untouched), and the pairs beside it are what they
    are alone."""
    rng = random.Random(23)
    leaf = ["".join(rng.choice("ACGT") for _ in range(70))]
    seqs = [pdc.related(rng, leaf[0], n) for n in (66, 70, 75)]
    want = [fp.align_pair_np(leaf, s)[1] for s in seqs]
    for banded in (False, True):
        bands = [(-10, 12)] * 3 if banded else None
        b = Batch([leaf], [(0, s) for s in seqs], bands=bands)
        wantb = want if not banded else [fp.align_pair_banded_np(leaf, s, -10, 12)[1] for s in seqs]
        table, need, total = b.table()
        status, score, tab, ws, ws_off, nd = launch(be, b)
        assert status == [0, 0, 0] and score == wantb
        check_tab(tab, b.dst, status, score)

        def refused(code, column=None, value=None, **kw):
            ptab = table.copy()
            if column is not None:
                ptab[1, column] = value
            status, score, tab, ws, ws_off, nd = launch(be, b, ptab=ptab, **kw)
            assert status == [0, code, 0] and score == [wantb[0], 0, wantb[2]], (banded, column, value, kw, status, score)
            check_tab(tab, b.dst, status, score)
            guards_hold(ws, ws_off, nd, untouched=(1,))
        refused(3, 0, 1)                                             # a leaf index of n_leaves, and of -1
        refused(3, 0, -1)
        refused(3, 2, -1)                                            # n < 0
        refused(1, 2, pa.MAX_LEN - 70)                               # n + C = 10^6: from the tables alone, whatever the workspace
        refused(2, 3, int(table[1, 3]) + 1)                          # wsoff misaligned, negative, and one block short of its need
        refused(2, 3, -64)
        refused(2, 3, total - int(need[1]) + 64)
        refused(2, 4, b.tab_words)                                   # dst one past the table, and far past it
        refused(2, 4, b.tab_words + 1000)
        if banded:                                                   # a band without (0, 0) or without (n, C)
            assert len(seqs[1]) == len(leaf[0])                      # (delta = 0: the band must hold diagonal 0)
            for lo, hi in ((1, 12), (-10, -1)):
                ptab = table.copy()
                ptab[1, 5], ptab[1, 6] = lo, hi
                bb = Batch([leaf], [(0, s) for s in seqs], bands=[(-10, 12), (lo, hi), (-10, 12)])
                assert traceback_scores(be, bb)[0] == [0, 3, 0]
                status, score, tab, ws, ws_off, nd = launch(be, b, ptab=ptab)
                assert status == [0, 3, 0] and score == [wantb[0], 0, wantb[2]]
                guards_hold(ws, ws_off, nd, untouched=(1,))
        # the last pair's row buffer one word outside the workspace: the others are written
        status, score, tab, ws, ws_off, nd = launch(be, b, ws_words=total - 64 - 1)
        assert status == [0, 0, 2] and score == [wantb[0], wantb[1], 0]
        check_tab(tab, b.dst, status, score)
    # a pair of 10^6 cells in all is refused with a workspace of one block
    b = Batch([leaf], [(0, seqs[0])])
    ptab = b.table()[0]
    ptab[0, 2] = pa.MAX_LEN
    assert launch(be, b, ptab=ptab, ws_words=64)[0] == [1]


# ---- 5. the two passes
@functools.lru_cache(maxsize=None)
def two_pass_locus(w0=16):
    """Four sequences built like pairdist_common.two_pass_locus' (a base of 600 nt; the base with every 40th base substituted: 15
    mismatches cost more than w0 columns of the counted bound, so a second pass; the base less 10 nt: certified in pass 1; 200
    unrelated nt: the band spans the columns, so the full DP) and an exact substring of the base: (sequences, per pair a < b (second
    pass run, sent to the full DP)) by freepairs_ref's two-pass statement."""
    rng = np.random.default_rng(11)
    L = 600
    base = "".join(rng.choice(list("ACGT"), L))
    sub = "".join("ACGT"[("ACGT".index(ch) + 1) % 4] if p % 40 == 15 else ch for p, ch in enumerate(base))
    near = base[:300] + base[310:]
    far = "".join(rng.choice(list("ACGT"), 200))
    seqs = [base, sub, near, far, base[150:420]]
    routes = {}
    for a in range(len(seqs)):
        for b in range(a + 1, len(seqs)):
            res, second, full, _ = fd.two_pass(seqs[a], seqs[b], w0)
            assert res[1] == fd.score(seqs[a], seqs[b])
            routes[a, b] = (second, full)
    return seqs, routes


def check_two_pass_conditions(w0=16):
    seqs, routes = two_pass_locus(w0)
    second, full = sum(r[0] for r in routes.values()), sum(r[1] for r in routes.values())
    print("pairs:", len(routes), "second passes:", second, "full:", full)
    assert second >= 1 and full >= 1 and len(routes) - second - full >= 1
    assert fd.distances(seqs, range(5))[0][4] == 0


def check_two_pass(be, w0=16):
    """The host's two passes return the full DP's overlap scores for every pair, and the counters name each route's count."""
    check_two_pass_conditions(w0)
    seqs, routes = two_pass_locus(w0)
    second, full = sum(r[0] for r in routes.values()), sum(r[1] for r in routes.values())
    want_s, want_nw = fd.tables(seqs)
    assert want_s != pd.tables(seqs)[0]
    for band in (None, w0):
        counters = {}
        (s, nw), = sa.prog_pair_tables(be, [[seq_codes(x) for x in seqs]], band=band, counters=counters, free_ends=True)
        assert nw.tolist() == want_nw and np.triu(s, 1).tolist() == np.triu(np.array(want_s), 1).tolist() and not np.tril(s).any(), band
        assert counters["pair_dist_pairs"] == counters["free_end_distance_pairs"] == len(routes)
        if band is not None:
            assert (counters["pair_dist_second_passes"], counters["pair_dist_full_pairs"]) == (second, full)
            assert counters["pair_dist_cells"] == sum(fd.two_pass(seqs[a], seqs[b], w0)[3] for a, b in routes)
        else:
            assert counters["pair_dist_cells"] == sum(len(seqs[a]) * len(seqs[b]) for a, b in routes)
    counters = {}
    (s, nw), = sa.prog_pair_tables(be, [[seq_codes(x) for x in seqs]], counters=counters)       # the switch off: pairdist_ref's
    assert np.triu(s, 1).tolist() == np.triu(np.array(pd.tables(seqs)[0]), 1).tolist() and "free_end_distance_pairs" not in counters


# ---- 6. whole MSAs
def plain_loci():
    """Two loci without fragments."""
    return pdc.some_loci()[:2]


def msa_loci():
    return [s for s, _ in fragment_loci()] + plain_loci()


FORMS = (dict(), dict(free_end_gaps=True), dict(free_end_gaps=True, free_end_pairs=True, refine=2))


@functools.lru_cache(maxsize=None)
def msa_spec(form: int, free: bool = True):
    kw = FORMS[form]
    return [fd.composed(l, free=free, **kw)[0] for l in msa_loci()]


def run(be, loci, **kw):
    msas = sa.star_msas(be, [pc.records(l) for l in loci], progressive=True, pair_distances=True, **kw)
    return [m.rows_as_strings() for m in msas]


def check_msas(be, **kw):
    """The rows equal the statement's, alone, with free_end_gaps, and with free_end_gaps, free_end_pairs and refine = 2; the
    counters; on the fragment loci the flag changes MSAs."""
    loci = msa_loci()
    n_pairs = sum(fd.progressive(l)[1][1] for l in loci)
    for form, extra in enumerate(FORMS):
        info, timings = [], {}
        got = run(be, loci, free_end_distances=True, pair_distancing=info, timings=timings, **extra, **kw)
        assert got == msa_spec(form), extra
        assert info == [fd.progressive(l)[1] for l in loci]
        assert timings["free_end_distance_pairs"] == timings["pair_dist_pairs"] == n_pairs
        for l, rows in zip(loci, got):
            pdc.invariants(l, rows)
    assert msa_spec(0)[:4] == [fd.progressive(l)[0] for l in loci[:4]]
    for form in range(len(FORMS)):
        assert sum(a != b for a, b in zip(msa_spec(form)[:4], msa_spec(form, False)[:4])) >= 1, form
    off = run(be, loci[:4], **kw)
    assert off == msa_spec(0, False)[:4] == [pd.progressive(l)[0] for l in loci[:4]] and off != msa_spec(0)[:4]


# ---- 7. the same bytes
def small_loci():
    """Loci for the compositions: three fragment loci of 9 records of 100 to 140 nt (by the statement: retree accepts a rebuild of
    the first, refine_tree a step of the second, seq_weights changes the third) and a locus without fragments."""
    return [fragment_locus(seed, 9, 100, 140, share=0.4)[0] for seed in (11, 14, 13)] + plain_loci()[:1]


def check_same_bytes(be):
    """band, device_tree and a small budget with several launches give the bytes of the plain flagged run, on small loci where a
    pass-1 half-width of 8 helps (at BAND_W0 a band spans these short matrices: check_same_bytes_msa_loci has the default band)."""
    loci = small_loci()
    want = [fd.progressive(l)[0] for l in loci]
    base = [fd.progressive(l)[1] for l in loci]
    assert any(len(s) < 90 for l in loci[:2] for s in l) and want != [pd.progressive(l)[0] for l in loci]
    assert run(be, loci, free_end_distances=True) == want
    for kw in (dict(band=True), dict(device_tree=True), dict(band=8, device_tree=True),
               dict(budget_bytes=1 << 15, chunk_bytes=1 << 14), dict(budget_bytes=1 << 15, band=8, device_tree=True)):
        info, timings = [], {}
        wrapped = tr.TraceBackend(be)
        assert run(wrapped, loci, free_end_distances=True, pair_distancing=info, timings=timings, **kw) == want, kw
        assert info == base and timings["free_end_distance_pairs"] == sum(i[1] for i in base)
        calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
        if "budget_bytes" in kw:
            assert calls.count(FULL) + calls.count(BANDED) >= 4, calls             # several launches
        if "band" in kw:
            assert timings["pair_dist_second_passes"] >= 0 and timings["pair_dist_full_pairs"] >= 0
            assert BANDED in calls or kw["band"] is True             # (at BAND_W0 a band spans these short matrices)


def check_same_bytes_msa_loci(be):
    """On the loci of check_msas (the four fragment loci of the finding and two without fragments) the default band, device_tree and
    a budget that forces several launches give the bytes of the plain flagged run; the default band takes every route: pass 1, second
    passes from certified_widths_endgap and pairs sent to the full DP."""
    loci, want = msa_loci(), msa_spec(0)
    base = [fd.progressive(l)[1] for l in loci]
    n_pairs = sum(i[1] for i in base)
    small = 4 * int(pa.workspace_words(600, 600))                 # (holds the widest merge; the pairs' row buffers need many times as much)
    for kw in (dict(band=True), dict(device_tree=True), dict(budget_bytes=small), dict(band=True, device_tree=True, budget_bytes=small)):
        info, timings = [], {}
        wrapped = tr.TraceBackend(be)
        assert run(wrapped, loci, free_end_distances=True, pair_distancing=info, timings=timings, **kw) == want, kw
        assert info == base and timings["free_end_distance_pairs"] == timings["pair_dist_pairs"] == n_pairs
        calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
        assert not {pdc.FULL, pdc.BANDED} & set(calls)
        if "budget_bytes" in kw:
            assert calls.count(FULL) + calls.count(BANDED) >= 4, calls             # several launches
        if "band" in kw:
            assert BANDED in calls and FULL in calls and calls.count("mprg_align_bounds_endgap") >= 1
            assert timings["pair_dist_second_passes"] > 0 and 0 < timings["pair_dist_full_pairs"] < n_pairs
        else:
            assert BANDED not in calls


def check_compositions_msa_loci(be):
    """seq_weights, retree = 1 and refine_tree = 1 on the loci of check_msas, on the device's tree with the default band: the
    statement's rows on the overlap scores' tree."""
    loci = msa_loci()
    for kw in (dict(seq_weights=True), dict(retree=1), dict(refine_tree=1)):
        assert run(be, loci, free_end_distances=True, device_tree=True, band=True, **kw) == [fd.composed(x, **kw)[0] for x in loci], kw
    assert any(fd.composed(x, seq_weights=True)[0] != fd.progressive(x)[0] for x in loci[:4])


def check_compositions(be):
    """collapse on a locus with copies, adjust_direction on a locus with a reversed record, seq_weights, retree = 1 and
    refine_tree = 1: each the statement's rows on the overlap scores' tree (these options change the MSA, so the reference's
    composition is what they are compared with).  On small_loci, chosen so that by the statement every stage does something;
    check_compositions_msa_loci runs the last three on check_msas' loci too."""
    loci = small_loci()
    l = loci[0]
    copies = l + [l[2], l[5], l[2]]
    rows, want, _ = fd.progressive(copies, collapse=True)
    assert want == (len(l), len(l) * (len(l) - 1) // 2, "pairs")
    for device_tree in (False, True):
        info = []
        got, = run(be, [copies], free_end_distances=True, collapse=True, pair_distancing=info, device_tree=device_tree)
        assert got == rows and info == [want]
        assert got[2] == got[len(l)] == got[len(l) + 2] and got[5] == got[len(l) + 1]
    flipped = [l[0]] + [st.rc(s) if k in (1, 4) else s for k, s in enumerate(l[1:])]
    rev, _, ori = st.oriented(flipped)
    assert any(rev) and ori == l
    m, = sa.star_msas(be, [pc.records(flipped)], progressive=True, pair_distances=True, free_end_distances=True, adjust_direction=True)
    assert m.descriptions == st.titles(pc.records(flipped), rev) and m.rows_as_strings() == fd.progressive(l)[0]
    for kw in (dict(seq_weights=True), dict(seq_weights=True, device_tree=True, band=True), dict(retree=1), dict(refine_tree=1)):
        ref = {k: v for k, v in kw.items() if k not in ("device_tree", "band")}
        assert run(be, loci, free_end_distances=True, **kw) == [fd.composed(x, **ref)[0] for x in loci], kw
    assert any(fd.composed(x, seq_weights=True)[0] != fd.progressive(x)[0] for x in loci)
    assert any(fd.composed(x, retree=1)[1][1] for x in loci) and any(fd.composed(x, refine_tree=1)[2][1] for x in loci)
    assert any(fd.composed(x, seq_weights=True)[0] != pd.composed(x, seq_weights=True)[0] for x in loci)     # (q from these D'')


# ---- 8. the flag off, and what moves
def check_trace(be):
    """With the flag off the pinned pair_distances scenario's calls, uploads and downloads are what they were, and no entry of the
    flag is called; with it on the charged score entries and mprg_align_bounds are not called."""
    lines, entry = tr.run(be, "pair_distances")
    assert entry == tr.golden()["pair_distances"]
    calls = {line.split()[1] for line in lines if line.startswith("call ")}
    assert {pdc.FULL, pdc.BANDED, "mprg_align_bounds"} <= calls and not calls & {FULL, BANDED, "mprg_align_bounds_endgap"}
    loci = small_loci()
    n_leaves = sum(fd.progressive(l)[1][0] for l in loci)
    for band in (None, 8):
        wrapped = tr.TraceBackend(be)
        run(wrapped, loci, free_end_distances=True, band=band, device_tree=True)
        calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
        assert FULL in calls or BANDED in calls
        assert not {pdc.FULL, pdc.BANDED, "mprg_align_bounds"} & set(calls)
        assert calls.count("mprg_align_bounds_endgap") == (0 if band is None else 1)
        first = min(k for k, line in enumerate(wrapped.lines) if line.startswith("call mprg_align_profiles"))
        last = max(k for k, line in enumerate(wrapped.lines) if line.startswith("call mprg_prog_tree"))
        bounds = [line for line in wrapped.lines[first:last + 1] if line.startswith("download int64")]
        assert bounds == ([] if band is None else [f"download int64 {3 * n_leaves}"])        # {SB', m', z} per leaf


def check_parameters(be):
    import pytest
    recs = [pc.records(pr.clade_locus(42, 8))]
    for kw in (dict(), dict(progressive=True), dict(pair_distances=True)):
        with pytest.raises(ValueError):
            sa.star_msas(be, recs, free_end_distances=True, **kw)
    opts = sa.Options(progressive=True, pair_dist=512, free_end_distances=True)
    assert not opts.star().free_end_distances and not sa.Options().free_end_distances


# ---- 9. the finding
# residue pairs shared with the truth of fragment_locus(seed, 20, 250, 350), seeds 0-3, as the references give them: (progressive
# with free end gaps on the 6-mer tree, pair distances + free end gaps, + free end distances, pair distances + free end gaps + free
# end pairs + refine 2, + free end distances)
FINDING = ((38008, 37854, 37927, 38095, 37950), (39335, 37775, 39113, 39164, 39305), (29838, 26914, 30503, 29614, 30249),
           (41555, 40617, 42030, 41930, 42032))


@functools.lru_cache(maxsize=None)
def finding():
    """Per fragment locus: (true rows, the five forms' rows)."""
    out = []
    for k, ((seqs, truth), (_, _, kmer)) in enumerate(zip(fragment_loci(), egc.finding())):
        out.append((truth, (kmer[1], msa_spec(1, False)[k], msa_spec(1)[k], msa_spec(2, False)[k], msa_spec(2)[k])))
    return out


def check_finding_reference():
    got = tuple(tuple(cmp.by_histogram(rows, truth)[0] for rows in forms) for truth, forms in finding())
    print("shared pairs (6-mer tree + free end gaps, pair distances + free end gaps, + free end distances, "
          "pair distances + free end gaps + free end pairs + refine 2, + free end distances):", got)
    assert tuple(f[0] for f in got) == tuple(f[1] for f in egc.FINDING)
    assert got == FINDING


# ---- 10. the command line
def check_parser(capsys):
    """--free-end-distances without --pair-distances or without --progressive is a parser error, exit status 2."""
    import pytest
    from make_prg_amd.__main__ import main
    for argv, message in ((["--unaligned", "--progressive"], "--free-end-distances needs --pair-distances"),
                          (["--unaligned"], "--free-end-distances needs --progressive"), ([], "--free-end-distances needs --progressive"),
                          (["--unaligned", "--pair-distances"], " needs --progressive")):        # (--pair-distances' own error comes first)
        with pytest.raises(SystemExit) as exc:
            main(["from_msa", "-i", "d", "-o", "o", "--free-end-distances"] + argv)
        assert exc.value.code == 2 and message in capsys.readouterr().err


def check_cli(be, tmp_path, caplog):
    """from_msa.run with --unaligned --progressive --pair-distances --free-end-distances --msa-dir (in process): the files are the
    statement's and the log has the flag's line once, with the pair count; without the flag the files are pairdist_ref's and the
    line is absent."""
    import logging
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    ls = small_loci()
    recs = [[(f"s{i} x", s) for i, s in enumerate(l)] for l in ls]
    for k, r in enumerate(recs):
        (src / f"g{k}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in r))
    old = {f"g{k}.fa": pd.fasta(r) for k, r in enumerate(recs)}
    pairs = sum(fd.progressive(l)[1][1] for l in ls)

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None, progressive=True, pair_distances=True)
        base.update(kw)
        return Namespace(**base)
    for flag in (True, False):
        caplog.clear()
        d = tmp_path / f"msas{flag}"
        with caplog.at_level(logging.INFO):
            from_msa.run(opts(output_prefix=str(tmp_path / f"o{flag}" / "a"), msa_dir=str(d), free_end_distances=flag), be)
        got = {p.name: p.read_text() for p in d.iterdir()}
        lines = [r.getMessage() for r in caplog.records if "--free-end-distances:" in r.getMessage()]
        if flag:
            want = {f"g{k}.fa": fd.fasta(r) for k, r in enumerate(recs)}
            assert got == want and got != old and len(lines) == 1 and f"--free-end-distances: {pairs} pair scores with free ends" in lines[0]
        else:
            assert got == old and not lines
