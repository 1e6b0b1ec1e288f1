"""The checks of `compare_msa` that run on the CPU emulation (tests/test_compare_emulated.py) and on the GPU
(tests/test_gpu_compare.py): a backend in, assertions inside.  tests/compare_ref.py is the statement they are held against."""
import functools
import gzip
import random

import numpy as np
import pytest

from make_prg_amd.from_msa import msa_compare as mc
from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.msa import MSA, encode
from make_prg_amd.utils.synthetic import diverged_locus, synth_rows
from tests import compare_ref as cr

INT32_MAX = 0x7fffffff
POISON = 0xA5
POISON_WORD = int(np.frombuffer(bytes([POISON] * 4), np.int32)[0])
ROWS = (1, 2, 3, 63, 64, 65, 128, 129)              # the P classes, and both sides of a wavefront
WIDTHS = (1, 63, 64, 65, 130)                       # the map's 64-column chunks


def msa(rows, ids=None):
    return MSA.from_strings(list(rows), ids)


def aligned(rng, seqs, W):
    return cr.random_alignment(rng, seqs, W - max((len(s) for s in seqs), default=0))


def shaped(rng, R, WT, WR, alphabet="ACGT"):
    """(test rows, reference rows) of R random sequences at exactly these widths: some rows empty, all-gap columns happen."""
    top = min(WT, WR)
    seqs = ["".join(rng.choice(alphabet) for _ in range(rng.choice((0, top, rng.randint(0, top))))) for _ in range(R)]
    return aligned(rng, seqs, WT), aligned(rng, seqs, WR)


@functools.lru_cache(maxsize=None)
def shape_loci():
    """Every R of ROWS with every width of WIDTHS on either side, W_T != W_R."""
    rng = random.Random(11)
    out = []
    for a, R in enumerate(ROWS):
        for b, WT in enumerate(WIDTHS):
            WR = WIDTHS[(a + b + 1) % len(WIDTHS)]
            if WR == WT:
                WR = WIDTHS[(a + b + 2) % len(WIDTHS)]
            out.append(shaped(rng, R, WT, WR, "ACGT" if (a + b) % 3 else "ACGTRYKMSWN"))
    return out


@functools.lru_cache(maxsize=None)
def shape_spec():
    return [cr.by_histogram(t, r) for t, r in shape_loci()]


def reversed_locus():
    """Rows given reversed on the test side: palindromes, ambiguity codes, an empty row; ids through _R_."""
    seqs = ["ACGT", "AATT", "ACGTRYKMSWN", "", "GGATCC", "ACCA", "NNRY", "TTTTA"]
    flip = [False, True, True, True, True, False, True, False]
    rng = random.Random(5)
    ref = aligned(rng, seqs, 14)
    test = aligned(rng, [cr.revcomp(s) if f else s for s, f in zip(seqs, flip)], 17)
    ref_ids = [f"s{i}" for i in range(len(seqs))]
    test_ids = [("_R_" if f else "") + i for i, f in zip(ref_ids, flip)]
    return test, ref, test_ids, ref_ids, flip


def counts(c):
    return tuple(int(v) for v in c[:6])


# ---- the statement against itself
def check_reference_forms_agree():
    rng = random.Random(2)
    for _ in range(300):
        t, r = cr.random_pair(rng)
        assert cr.by_definition(t, r) == cr.by_histogram(t, r), (t, r)
        got = cr.by_histogram(t, t)
        assert got[0] == got[1] == got[2] and got[3] == got[4] == got[5], t
    assert cr.by_definition(["AC-GT", "ACG-T", "A-CGT"], ["ACGT-", "ACGT-", "AC-GT"]) == (5, 10, 9, 4, 1, 1)
    assert cr.by_histogram(["AC-GT", "ACG-T", "A-CGT"], ["ACGT-", "ACGT-", "AC-GT"]) == (5, 10, 9, 4, 1, 1)
    test, ref, ti, ri, flip = reversed_locus()
    rows, rev = cr.match(ti, ri)
    assert rev == flip and rows == list(range(len(ri)))
    assert cr.by_definition(test, ref, rows, rev) == cr.by_histogram(test, ref, rows, rev)


# ---- the kernels through compare_msas
def check_kernel(be):
    loci = shape_loci()
    for layout in (mc.ROW_MAJOR, mc.COLUMN_MAJOR):
        got = mc.compare_msas(be, [msa(t) for t, _ in loci], [msa(r) for _, r in loci], layout=layout)
        for k, (c, want) in enumerate(zip(got, shape_spec())):
            assert c.skipped is None and counts(c) == want, (layout, k, len(loci[k][0]), c, want)
    small = mc.compare_msas(be, [msa(t) for t, _ in loci], [msa(r) for _, r in loci], budget_bytes=5000)          # several groups
    assert [counts(c) for c in small] == shape_spec()
    ex = mc.compare_msas(be, [msa(["AC-GT", "ACG-T", "A-CGT"])], [msa(["ACGT-", "ACGT-", "AC-GT"])])[0]
    assert counts(ex) == (5, 10, 9, 4, 1, 1) and ex.sp == 0.5 and ex.modeler == 5 / 9 and ex.tc == ex.cs == 0.25
    # a reference of one column, rows without a residue, MSAs without a column or a residue: ratios None
    for t, r, want in ((["A--", "-A-", "---"], ["A", "A", "-"], (0, 1, 0, 1, 0, 0)), (["-", "-"], ["--", "--"], (0,) * 6),
                       (["", ""], ["", ""], (0,) * 6), (["A"], ["-A"], (0,) * 6)):
        c = mc.compare_msas(be, [msa(t)], [msa(r)])[0]
        assert counts(c) == want == cr.by_histogram(t, r), (t, r, c)
    none = mc.compare_msas(be, [msa(["-", "-"])], [msa(["--", "--"])])[0]
    assert none.sp is None and none.modeler is None and none.tc is None and none.cs is None and none.skipped is None


def check_identity(be):
    """T against T: shared = ref_pairs = test_pairs and ref_columns = kept = identical."""
    loci = shape_loci()[::3]
    for c in mc.compare_msas(be, [msa(t) for t, _ in loci], [msa(t) for t, _ in loci]):
        assert c.shared == c.ref_pairs == c.test_pairs and c.ref_columns == c.kept_columns == c.identical_columns


def check_tall(be):
    """8 192 rows x 3 columns: a segment is the whole tile; 8 193 rows: skipped, nothing launched for it."""
    rng = random.Random(8)
    seqs = [rng.choice(("A", "C", "AC", "", "ACG")) for _ in range(mc.CMP_MAX_ROWS)]
    ref, test = aligned(rng, seqs, 3), aligned(rng, seqs, 4)
    small_t, small_r = ["AC-", "A-C"], ["AC", "AC"]
    got = mc.compare_msas(be, [msa(small_t), msa(test), msa(test + ["A---"]), msa(small_t)],
                          [msa(small_r), msa(ref), msa(ref + ["A--"]), msa(small_r)])
    assert counts(got[1]) == cr.by_histogram(test, ref) and got[1].skipped is None
    assert got[2] == mc.Comparison(0, 0, 0, 0, 0, 0, "rows")
    assert counts(got[0]) == counts(got[3]) == cr.by_histogram(small_t, small_r)
    assert counts(mc.total(got)) == tuple(a + 2 * b for a, b in zip(counts(got[1]), counts(got[0])))


def check_reversed(be):
    test, ref, ti, ri, flip = reversed_locus()
    want = cr.by_histogram(test, ref, *cr.match(ti, ri))
    assert counts(mc.compare_msas(be, [msa(test, ti)], [msa(ref, ri)])[0]) == want
    # matched by id: the test rows in another order
    order = [3, 0, 7, 1, 6, 2, 5, 4]
    assert counts(mc.compare_msas(be, [msa([test[i] for i in order], [ti[i] for i in order])], [msa(ref, ri)])[0]) == want
    # by position (an id twice), the flag from the prefix at the same position
    ri2 = ["s0"] + ri[1:-1] + ["s0"]
    ti2 = [("_R_" if f else "") + i for i, f in zip(ri2, flip)]
    assert counts(mc.compare_msas(be, [msa(test, ti2)], [msa(ref, ri2)])[0]) == want
    # a record whose own id begins with _R_ on both sides is no reversed row
    assert mc.match_rows(["_R_a", "a"], ["a", "_R_a"]) == ([1, 0], [False, False])
    assert mc.match_rows(["_R_a", "b"], ["b", "a"]) == ([1, 0], [False, True])
    with pytest.raises(mc.RowMatchError, match="locus L7"):
        mc.compare_msas(be, [msa(["A", "C"], ["a", "b"])], [msa(["A"], ["a"])], names=["L7"])


# ---- the entry points called directly
def _pack(texts, pad):
    """The texts one behind the other, `pad` bytes of poison before each: (bytes, offsets)."""
    parts, offs, at = [], [], 0
    for t in texts:
        parts.append(np.full(pad, POISON, np.uint8))
        at += pad
        offs.append(at)
        parts.append(np.ascontiguousarray(t, np.uint8).reshape(-1))
        at += t.size
    return np.concatenate(parts), offs


def codes_of(rows):
    W = len(rows[0])
    return encode(np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), W))


def direct(be, loci, layout, gap_words=3, order=None, rev=None, poff_gap=1):
    """mprg_msa_compare_map and _columns on (test rows, reference rows) loci: the test texts at odd offsets in buffer 0, the
    reference texts in buffer 1, tpos, tmap and the status words poisoned, gap_words poisoned words between the loci's tmap and m
    parts.  Returns (counts (n, 6), map status, columns status, tmap words, m words, the locus table)."""
    tc, rc = [codes_of(t) for t, _ in loci], [codes_of(r) for _, r in loci]
    n = len(loci)
    tb, toffs = _pack(tc, 3)
    rb, roffs = _pack(rc, 5)
    R = np.array([len(x) for x in rc], np.int64)
    WT, WR = np.array([x.shape[1] for x in tc], np.int64), np.array([x.shape[1] for x in rc], np.int64)
    tmap_off = mc.exclusive_sum(R * WR + gap_words) + gap_words
    m_off = mc.exclusive_sum(WT + gap_words) + gap_words
    tmap_words, m_words = int((R * WR + gap_words).sum()) + gap_words, int((WT + gap_words).sum()) + gap_words
    table = np.stack([np.zeros(n, np.int64), toffs, WT, np.ones(n, np.int64), roffs, WR, R, tmap_off, np.full(n, layout, np.int64), m_off],
                     1).astype(np.int64)
    cap = np.concatenate([(x != 4).sum(axis=1) for x in rc]).astype(np.int64)
    rows = np.stack([np.repeat(np.arange(n), R), mc._ranges(np.zeros(n, np.int64), R),
                     np.concatenate([np.arange(r) if order is None else np.asarray(order[k]) for k, r in enumerate(R)]),
                     np.concatenate([np.zeros(r, np.int64) if rev is None else np.asarray(rev[k], np.int64) for k, r in enumerate(R)]),
                     mc.exclusive_sum(cap + poff_gap), cap], 1).astype(np.int64)
    d_t, d_r = be.upload(tb), be.upload(rb)
    d_bufs = be.upload(np.array([[be.ptr(d_t), len(tb)], [be.ptr(d_r), len(rb)]], np.int64))
    return raw_launch(be, d_bufs, 2, table, rows, int((cap + poff_gap).sum()), tmap_words, m_words, keep=(d_t, d_r))


def raw_launch(be, d_bufs, n_bufs, table, rows, tpos_words, tmap_words, m_words, work=None, keep=()):
    n = len(table)
    if work is None:
        blocks = mc.column_blocks(table[:, 6], table[:, 5])
        work = np.stack([np.repeat(np.arange(n), blocks), mc._ranges(np.zeros(n, np.int64), blocks)], 1).astype(np.int32)
    d_table, d_rows, d_work = be.upload(table), be.upload(rows), be.upload(work)
    d_tpos, d_tmap, d_m = be.full(4 * tpos_words, POISON), be.full(4 * tmap_words, POISON), be.zeros(4 * m_words)
    d_counts, d_s1, d_s2 = be.zeros(48 * n), be.full(4 * len(rows), POISON), be.full(4 * len(work), POISON)
    be.call("mprg_msa_compare_map", be.ptr(d_bufs), n_bufs, be.ptr(d_table), n, be.ptr(d_rows), len(rows), be.ptr(d_tpos), tpos_words,
            be.ptr(d_tmap), tmap_words, be.ptr(d_m), m_words, be.ptr(d_s1), be.stream)
    be.call("mprg_msa_compare_columns", be.ptr(d_table), n, be.ptr(d_work), len(work), be.ptr(d_tmap), tmap_words, be.ptr(d_m), m_words,
            be.ptr(d_counts), be.ptr(d_s2), be.stream)
    out = (be.download(d_counts, np.int64, 6 * n).reshape(n, 6), be.download(d_s1, np.int32, len(rows)), be.download(d_s2, np.int32, len(work)),
           be.download(d_tmap, np.int32, tmap_words), be.download(d_m, np.int32, m_words), table)
    del keep
    return out


def expected_tmap(test, ref, layout, order=None, rev=None):
    t = cr.t_columns(test, ref, order, rev)
    R, W = len(ref), len(ref[0])
    v = np.full((R, W), INT32_MAX, np.int64)
    for k, row in enumerate(ref):
        v[k, cr.columns_of(row)] = t[k]
    return (v.T if layout else v).reshape(-1)


def check_direct(be):
    """Odd text offsets, two buffers, several loci in one launch, poisoned outputs: the counts, every tmap word, every m word, and
    the words between the loci untouched."""
    rng = random.Random(21)
    loci = [shaped(rng, 3, 5, 7), shaped(rng, 65, 66, 63, "ACGTRYKMSWN"), shaped(rng, 1, 130, 1), shaped(rng, 9, 1, 64), shaped(rng, 130, 7, 9)]
    test, ref, _, _, flip = reversed_locus()
    order = [list(range(len(r))) for _, r in loci] + [list(range(len(ref)))]
    order[1] = rng.sample(range(65), 65)
    loci[1] = ([loci[1][0][order[1].index(i)] for i in range(65)], loci[1][1])          # test row order[k] holds reference row k
    rev = [[0] * len(r) for _, r in loci] + [[int(f) for f in flip]]
    loci.append((test, ref))
    for layout in (mc.ROW_MAJOR, mc.COLUMN_MAJOR):
        got, s1, s2, tmap, m, table = direct(be, loci, layout, order=order, rev=rev)
        assert not s1.any() and not s2.any()
        used_t, used_m = np.zeros(len(tmap), bool), np.zeros(len(m), bool)
        for k, (t, r) in enumerate(loci):
            assert tuple(got[k]) == cr.by_histogram(t, r, order[k], [bool(x) for x in rev[k]]), (layout, k)
            lo, words = int(table[k, 7]), len(r) * len(r[0])
            assert np.array_equal(tmap[lo:lo + words], expected_tmap(t, r, layout, order[k], [bool(x) for x in rev[k]])), (layout, k)
            used_t[lo:lo + words] = True
            mo = int(table[k, 9])
            assert np.array_equal(m[mo:mo + len(t[0])], [sum(row[c] != "-" for row in t) for c in range(len(t[0]))])
            used_m[mo:mo + len(t[0])] = True
        assert (tmap[~used_t] == POISON_WORD).all() and not m[~used_m].any()


def check_refusals(be):
    t, r = ["AC-GT", "ACG-T", "A-CGT"], ["ACGT-", "ACGT-", "AC-GT"]
    ids = ["x", "y", "z"]
    ok_t, ok_r = msa(["AC", "A-"]), msa(["AC", "-A"])
    for bad, text in ((["AC-GT", "ACT-T", "A-CGT"], "same sequence"), (["AC-GT", "AC--T", "A-CGT"], "same number of residues"),
                      (["AC-GT-", "ACG-TA", "A-CGT-"], "same number of residues")):
        with pytest.raises(mc.SequenceMismatchError, match=r"locus second, record 2 \(y\)") as exc:
            mc.compare_msas(be, [ok_t, msa(bad, ids)], [ok_r, msa(r, ids)], names=["first", "second"])
        assert text in str(exc.value) and isinstance(exc.value, ValueError)
    # a row given unreversed under a reversed id, and a reversed row under a plain id (AACG is no palindrome)
    t2, r2 = ["AAC-G", "AACG-"], ["AACG", "AACG"]
    with pytest.raises(mc.SequenceMismatchError, match=r"locus 0, record 2 \(z\).*reversed"):
        mc.compare_msas(be, [msa(t2, ["x", "_R_z"])], [msa(r2, ["x", "z"])])
    with pytest.raises(mc.SequenceMismatchError, match=r"locus 0, record 1 \(x\)"):
        mc.compare_msas(be, [msa([cr.revcomp("AACG") + "-", t2[1]], ["x", "z"])], [msa(r2, ["x", "z"])])
    rt = [cr.revcomp("AACG") + "-", t2[1]]
    assert counts(mc.compare_msas(be, [msa(rt, ["_R_x", "z"])], [msa(r2, ["x", "z"])])[0]) == cr.by_histogram(rt, r2, [0, 1], [True, False])
    # a palindrome reads the same reversed: no error, and the reversal still moves its columns
    pal_t, pal_r = ["AATT-", "AA-TT"], ["AATT", "AATT"]
    got = mc.compare_msas(be, [msa(pal_t, ["_R_a", "b"])], [msa(pal_r, ["a", "b"])])[0]
    assert counts(got) == cr.by_histogram(pal_t, pal_r, [0, 1], [True, False]) != cr.by_histogram(pal_t, pal_r)
    with pytest.raises(mc.CompareError, match=r"locus 0, record 2 \(s1\) of the test MSA: character 'X'"):
        mc.compare_msas(be, [msa(["AC", "AX"])], [msa(["AC", "AC"])])
    # the status words of a substitution, a missing residue and a wrong flag, called directly
    got, s1, s2, tmap, m, _ = direct(be, [(t, r), (["AC-GT", "ACT-T", "A-CGT"], r), (["AC-GT", "AC--T", "A-CGT"], r),
                                          (["AAC-G", "AACG-", "AACG-"], ["AACG"] * 3)], 1, rev=[[0, 0, 0]] * 3 + [[0, 1, 0]])
    assert s1.tolist() == [0, 0, 0, 0, mc.CMP_CODE, 0, 0, mc.CMP_COUNT, 0, 0, mc.CMP_CODE, 0] and not s2.any()
    assert tuple(got[0]) == (5, 10, 9, 4, 1, 1)


def check_bad_ranges(be):
    """A range outside its table or buffer: the status word, and nothing else written."""
    t, r = codes_of(["AC-GT", "ACG-T", "A-CGT"]), codes_of(["ACGT-", "ACGT-", "AC-GT"])
    text = np.concatenate([t.reshape(-1), r.reshape(-1)])
    good = [0, 0, 5, 0, 15, 5, 3, 0, 0, 0]
    row = [0, 0, 0, 0, 0, 4]
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64))
    cases = []
    for f, v in ((0, 1), (0, -1), (1, 16), (1, -1), (2, 6), (2, 0), (3, 2), (4, 16), (5, 0), (5, 1 << 31), (6, 4), (6, 0), (7, 1), (7, -1), (8, 2), (9, 1),
                 (9, -4)):
        bad = list(good)
        bad[f] = v
        cases.append((bad, row, f in (0, 1, 3, 4)))          # (the columns kernel does not read the texts)
    for f, v in ((0, 1), (0, -1), (1, 3), (1, -1), (2, 3), (2, -1), (3, 2), (3, -1), (4, 9), (4, -1), (5, 13), (5, -1)):
        bad = list(row)
        bad[f] = v
        cases.append((good, bad, True))
    for lo, bad_row, columns_run in cases:
        got, s1, s2, tmap, m, _ = raw_launch(be, d_bufs, 1, np.array([lo], np.int64), np.array([bad_row] * 3, np.int64), 12, 15, 5,
                                             np.array([[0, 0]], np.int32))
        assert (s1 == mc.CMP_BAD_ITEM).all(), (lo, bad_row, s1)
        assert (tmap == POISON_WORD).all() and not m.any() and not got.any(), (lo, bad_row)
        assert s2.tolist() == [0 if columns_run else mc.CMP_BAD_ITEM], (lo, s2)
    # the columns' own refusals: a locus index, a block outside the locus, more than CMP_MAX_ROWS rows
    rows3 = np.array([[0, k, k, 0, 4 * k, 4] for k in range(3)], np.int64)
    for work in ([[1, 0]], [[-1, 0]], [[0, 1]], [[0, -1]]):
        got, s1, s2, _, _, _ = raw_launch(be, d_bufs, 1, np.array([good], np.int64), rows3, 12, 15, 5, np.array(work, np.int32))
        assert not s1.any() and (s2 == mc.CMP_BAD_ITEM).all() and not got.any(), work
    tall = [0, 0, 1, 0, 0, 1, mc.CMP_MAX_ROWS + 1, 0, 0, 0]
    d_tall = be.upload(np.full(mc.CMP_MAX_ROWS + 1, 4, np.uint8))
    d_b2 = be.upload(np.array([[be.ptr(d_tall), mc.CMP_MAX_ROWS + 1]], np.int64))
    got, s1, s2, _, _, _ = raw_launch(be, d_b2, 1, np.array([tall], np.int64), np.array([[0, 0, 0, 0, 0, 0]], np.int64), 0, mc.CMP_MAX_ROWS + 1, 1,
                                      np.array([[0, 0]], np.int32))
    assert s1.tolist() == [0] and s2.tolist() == [mc.CMP_BAD_ITEM] and not got.any()
    got, s1, s2, _, _, _ = raw_launch(be, d_bufs, 1, np.array([good], np.int64), rows3, 12, 15, 5)
    assert not s1.any() and not s2.any() and tuple(got[0]) == (5, 10, 9, 4, 1, 1)


# ---- properties
def check_properties(be):
    rng = random.Random(31)
    loci = [shaped(rng, R, WT, WR) for R, WT, WR in ((5, 9, 12), (17, 40, 33), (70, 30, 35), (2, 6, 6))] + [cr.random_pair(rng) for _ in range(20)]
    base = [counts(c) for c in mc.compare_msas(be, [msa(t) for t, _ in loci], [msa(r) for _, r in loci])]
    for c in base:
        assert c[0] <= min(c[1], c[2]) and c[5] <= c[4] <= c[3]
    perm, gapped = [], []
    for t, r in loci:
        p = rng.sample(range(len(t)), len(t))
        perm.append(([t[i] for i in p], [r[i] for i in p]))

        def with_gaps(rows):
            at = sorted(rng.randint(0, len(rows[0])) for _ in range(3))
            return [x[:at[0]] + "-" + x[at[0]:at[1]] + "--" + x[at[1]:at[2]] + "-" + x[at[2]:] for x in rows]
        gapped.append((with_gaps(t), with_gaps(r)))
    # (ids by position: permuting both MSAs together is another pair of MSAs of the same records)
    assert [counts(c) for c in mc.compare_msas(be, [msa(t) for t, _ in perm], [msa(r) for _, r in perm])] == base
    assert [counts(c) for c in mc.compare_msas(be, [msa(t) for t, _ in gapped], [msa(r) for _, r in gapped])] == base


# ---- whole MSAs against their truth
@functools.lru_cache(maxsize=None)
def truth_loci():
    """(name, sequences, true rows): synth_rows loci and diverged loci of 8 sequences."""
    out = []
    for seed, (S, C, clades) in ((0, (12, 120, 2)), (1, (30, 300, 3)), (2, (7, 200, 2))):
        rows = [r.decode() for r in synth_rows(seed, S, C, clades)]
        out.append((f"synth{seed}", [cr.ungap(r) for r in rows], rows))
    for seed in (3, 4):
        seqs, rows = diverged_locus(seed, 8)
        out.append((f"diverged{seed}", seqs, rows))
    return out


def check_integration(be):
    from tests import star_ref as sr
    loci = truth_loci()
    recs = [[(f"s{i}", s) for i, s in enumerate(seqs)] for _, seqs, _ in loci]
    msas = sa.star_msas(be, recs, names=[n for n, _, _ in loci])
    truth = [msa(rows) for _, _, rows in loci]
    got = mc.compare_msas(be, msas, truth, names=[n for n, _, _ in loci])
    centre = sa.centres(be, [sa.locus_codes(n, r) for (n, _, _), r in zip(loci, recs)])
    for (name, seqs, rows), m, c, cen in zip(loci, msas, got, centre):
        star = m.rows_as_strings()
        assert [cr.ungap(x) for x in star] == seqs
        assert counts(c) == cr.by_histogram(star, rows), name
        assert 0 < c.shared <= c.ref_pairs
        # the pairs with the centre row: every other row with the centre as a locus of two rows
        cen = int(cen)
        others = [a for a in range(len(seqs)) if a != cen]
        two = mc.compare_msas(be, [msa([star[a], star[cen]]) for a in others], [msa([rows[a], rows[cen]]) for a in others])
        assert (sum(x.shared for x in two), sum(x.ref_pairs for x in two)) == sr.pair_recovery(rows, star, cen), name


def check_flipped(be):
    """--adjust-direction: a record star_msas reversed matches, through its _R_ title, the row another alignment of the same file
    gives it, as a reversed row; against the truth, which holds every record in the family's orientation, a row is reversed where
    the aligner's choice and the file's flip disagree."""
    name, seqs, rows = truth_loci()[3]
    flip = [False, True, False, False, True, True, False, False]
    given = [cr.revcomp(s) if f else s for s, f in zip(seqs, flip)]
    orientation = []
    m = sa.star_msas(be, [[(f"s{i}", s) for i, s in enumerate(given)]], adjust_direction=True, orientation=orientation)[0]
    assert list(orientation[0][0]) == flip and [i.startswith("_R_") for i in m.ids] == flip
    star = m.rows_as_strings()
    ids = [f"s{i}" for i in range(8)]
    other = aligned(random.Random(6), given, max(map(len, given)) + 9)
    got = mc.compare_msas(be, [m], [msa(other, ids)])[0]
    assert counts(got) == cr.by_histogram(star, other, *cr.match(m.ids, ids))
    wrong = [("_R_" if a != b else "") + i for i, a, b in zip(ids, orientation[0][0], flip)]
    got = mc.compare_msas(be, [msa(star, wrong)], [msa(rows, ids)])[0]
    assert counts(got) == cr.by_histogram(star, rows) and got.sp > 0.5


def check_diverged_locus():
    for seed in (3, 17, 40):
        seqs, rows = diverged_locus(seed, 12)
        assert seqs == cr.old_diverged_seqs(seed, 12)
        assert [cr.ungap(r) for r in rows] == seqs and len({len(r) for r in rows}) == 1
        assert all(any(r[c] != "-" for r in rows) for c in range(len(rows[0])))
    # an insertion has columns of its own: no other row holds a residue there
    seqs, rows = diverged_locus(3, 12)
    own = sum(1 for c in range(len(rows[0])) if sum(r[c] != "-" for r in rows) == 1)
    assert own > 0


# ---- the command line
def cli_files(tmp_path):
    """A directory pair: a.fa, b.fa(.gz on the test side), c.fa; returns (test dir, reference dir, {locus: counts})."""
    rng = random.Random(41)
    td, rd = tmp_path / "test", tmp_path / "ref"
    td.mkdir()
    rd.mkdir()
    want = {}
    for name in "abc":
        t, r = shaped(rng, 6, 30, 33, "ACGTN")
        ids = [f"r{i}" for i in range(6)]
        fasta_t = "".join(f">{i}\n{x}\n" for i, x in zip(ids, t))
        fasta_r = "".join(f">{i} reference\n{x}\n" for i, x in reversed(list(zip(ids, r))))
        if name == "b":
            with gzip.open(td / "b.fa.gz", "wt") as fh:
                fh.write(fasta_t)
        else:
            (td / f"{name}.fa").write_text(fasta_t)
        (rd / f"{name}.fa").write_text(fasta_r)
        want[name] = cr.by_histogram(t, r)
    return td, rd, want


def clustal_text(ids, rows):
    out = ["CLUSTAL W (1.83) multiple sequence alignment", "", ""]
    for lo in range(0, len(rows[0]), 60):
        out += [f"{i:<16}{r[lo:lo + 60]}" for i, r in zip(ids, rows)] + ["", ""]
    return "\n".join(out) + "\n"


def parse_tsv(text):
    lines = [l.split("\t") for l in text.splitlines()]
    assert lines[0] == ["locus", "shared", "ref_pairs", "test_pairs", "ref_columns", "kept_columns", "identical_columns", "SP", "Modeler",
                        "TC", "CS", "skipped"]
    return {l[0]: l[1:] for l in lines[1:]}


def check_tsv(text, want):
    got = parse_tsv(text)
    assert list(got) == sorted(want) + ["total"]
    for name, c in want.items():
        assert tuple(int(v) for v in got[name][:6]) == c and got[name][10] == "-"
        for v, (a, b) in zip(got[name][6:10], ((c[0], c[1]), (c[0], c[2]), (c[5], c[3]), (c[4], c[3]))):
            assert v == ("NA" if b == 0 else f"{a / b:.6f}")
    tot = tuple(sum(c[f] for c in want.values()) for f in range(6))
    assert tuple(int(v) for v in got["total"][:6]) == tot and got["total"][6] == f"{tot[0] / tot[1]:.6f}"
