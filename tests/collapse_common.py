"""What the emulated and the GPU tests of `from_msa --unaligned --collapse-identical` share: mprg_star_identical and
mprg_prog_columns_weighted called directly through the C ABI, and whole MSAs on small loci with duplicates injected, against the
spec's plain-Python statement (tests/collapse_ref.py) and against the flag-off run."""
import functools
import random

import numpy as np
import pytest

from make_prg_amd.backend import MprgError
from make_prg_amd.from_msa import star_align as sa
from tests import collapse_ref as cr
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import star_ref as sr
from tests import strand_ref as st

POISON = 0x5C
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 128, 129)


# ---- mprg_star_identical
def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _changed(s, i):
    return s[:i] + ("C" if s[i] != "C" else "G") + s[i + 1:]


@functools.lru_cache(maxsize=None)
def identical_loci():
    rng = random.Random(7)
    s = _seq(rng, 130)
    loci = [["ACGTACGTTGCA"],                                               # one record
            [s[:70]] * 5,                                                   # all identical
            [_seq(rng, 40) for _ in range(6)],                              # none identical
            [s, _changed(s, 0), _changed(s, 65), _changed(s, 129), s, _changed(s, 129), _changed(s, 0), _changed(s, 65)],
            ["ACGTACGT", "ACGTACGTAA", "ACGTACGT", "ACGTACG", "ACGTACGTAA"],  # a sequence that is a prefix of another
            ["AAA", "CCC", "GGG", "CCC", "GGG", "N", "n"],                    # classes whose first member is not record 0
            ["", "ACGT", "", "--", "ACGT"]]                                 # empty records stay their own
    for n in LENGTHS:
        t = _seq(rng, n)
        loci.append([t, t, _changed(t, n - 1), t, _changed(t, n - 1), _changed(t, 0)] if n else ["", "A", ""])
    # 300 records, interleaved classes: seven sequences of one length (two of them one byte apart), three of other lengths
    base = [_seq(rng, 70) for _ in range(6)]
    base += [_changed(base[0], 69), base[1][:69], base[2] + "A", _seq(rng, 5)]
    loci.append([base[(a * a + a // 7) % len(base)] for a in range(300)])
    # more records than one tile of hashes holds: classes that begin in the first, the second and the third tile
    pool = [_seq(rng, rng.randint(1, 12)) for _ in range(900)]
    loci.append([pool[a] if a % 3 else pool[rng.randrange(a + 1)] for a in range(900)] + [pool[rng.randrange(900)] for _ in range(400)])
    return loci


def check_identical(be):
    loci = identical_loci()
    norm = [[sr.normalise(x) for x in l] for l in loci]
    want = [cr.classes(l) for l in norm]
    assert any(r != list(range(len(r))) for r in want) and max(map(len, loci)) > 1024
    assert any(r[a] == a and a > 600 and r.count(a) > 1 for r in want[-1:] for a in r)      # a class that begins behind the first tile
    codes = [sa.locus_codes(str(k), pc.records(l)) for k, l in enumerate(loci)]
    for bits in (64, 1, 0):
        got = sa.identical(be, codes, bits)
        assert [g.tolist() for g in got] == want, bits


def check_identical_refusals(be):
    """A bad locus between good ones: its status, none of its rep written, the words around rep untouched."""
    seqs = ["ACGTAC", "ACGTAC", "TTTT", "GG", "GG", "ACGTAC", "TTTT"]
    packed = np.frombuffer("".join(seqs).encode(), np.uint8)
    d_codes = be.upload(sa.encode(packed))
    off = sa.exclusive_sum([len(x) for x in seqs])
    stab = [[int(o), len(x)] for o, x in zip(off, seqs)]
    ltab = [[0, 2, 0, 0], [2, 3, 0, 0], [5, 2, 0, 0]]

    def run(stab, ltab, codes_bytes=len(packed), n_seqs=len(seqs), bits=64):
        d_rep, d_status = be.full(4 * (len(seqs) + 8), POISON), be.full(4 * len(ltab), POISON)
        d_seqs, d_loci = be.upload(np.array(stab, np.int64)), be.upload(np.array(ltab, np.int64))
        be.call("mprg_star_identical", be.ptr(d_codes), codes_bytes, be.ptr(d_seqs), n_seqs, be.ptr(d_loci), len(ltab), bits,
                be.ptr(d_rep) + 16, be.ptr(d_status), be.stream)
        rep = be.download(d_rep, np.int32, len(seqs) + 8)
        assert (rep[:4].view(np.uint8) == POISON).all() and (rep[-4:].view(np.uint8) == POISON).all()
        return be.download(d_status, np.int32, len(ltab)).tolist(), rep[4:-4].tolist()
    blank = int(np.full(4, POISON, np.uint8).view(np.int32)[0])
    assert run(stab, ltab) == ([0, 0, 0], [0, 0, 0, 1, 1, 0, 1])
    bad_seq = [list(x) for x in stab]
    for entry in ([9, 25], [-1, 2], [30, 2], [10, -1]):
        bad_seq[3] = entry                                          # a sequence of the middle locus outside the codes
        assert run(bad_seq, ltab) == ([0, sa.CENTRE_BAD, 0], [0, 0, blank, blank, blank, 0, 1]), entry
    for entry in ([2, 6, 0, 0], [-1, 3, 0, 0], [2, -1, 0, 0], [8, 1, 0, 0]):     # the locus outside the sequence table
        got = run(stab, [ltab[0], entry, ltab[2]])
        assert got == ([0, sa.CENTRE_BAD, 0], [0, 0, blank, blank, blank, 0, 1]), entry
    assert run(stab, ltab, codes_bytes=len(packed) - 1) == ([0, 0, sa.CENTRE_BAD], [0, 0, 0, 1, 1, blank, blank])
    for bits in (-1, 65):
        with pytest.raises(MprgError, match="filter_bits"):
            run(stab, ltab, bits=bits)


# ---- mprg_prog_columns_weighted
def _columns(be, texts, weights=None, sums=None, weights_words=None, woffs=None):
    """Both kinds of every text (R x W matrices of cell codes) through mprg_prog_columns, or with weights (per text an int array)
    through mprg_prog_columns_weighted: (status words, the planes as one int32 array, each item's fields, nothing else written)."""
    off = sa.exclusive_sum([t.size for t in texts])
    text = np.concatenate([t.reshape(-1) for t in texts])
    d_text = be.upload(text)
    d_bufs = be.upload(np.array([[be.ptr(d_text), len(text)]], np.int64))
    items, work, words = [], [], 0
    woff = sa.exclusive_sum([len(t) for t in texts]).tolist() if woffs is None else woffs
    for kind in (0, 1):
        for k, (t, o) in enumerate(zip(texts, off.tolist())):
            work += [[len(items), tile] for tile in range(-(-t.shape[1] // 256))]
            items.append([0, o, *t.shape, kind, words] + ([] if weights is None else [woff[k], int(weights[k].sum()) if sums is None else sums[k]]))
            words += (6 + kind) * t.shape[1]
    d_cols, d_status = be.full(4 * words + 64, POISON), be.full(4 * len(work), POISON)
    d_items, d_work = be.upload(np.array(items, np.int64)), be.upload(np.array(work, np.int32))
    if weights is None:
        be.call("mprg_prog_columns", be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work), be.ptr(d_cols), words,
                be.ptr(d_status), be.stream)
    else:
        flat = np.concatenate(weights).astype(np.int32)
        d_weights = be.upload(flat)
        be.call("mprg_prog_columns_weighted", be.ptr(d_bufs), 1, be.ptr(d_items), len(items), be.ptr(d_work), len(work),
                be.ptr(d_weights), len(flat) if weights_words is None else weights_words, be.ptr(d_cols), words, be.ptr(d_status), be.stream)
    raw = be.download(d_cols, np.uint8, 4 * words + 64)
    assert (raw[4 * words:] == POISON).all()
    return be.download(d_status, np.int32, len(work)).tolist(), raw[:4 * words].copy(), items


def _texts(rng, shapes):
    out = []
    for R, W in shapes:
        t = pc.related_codes(rng, W, rng.integers(0, 4, W), R, W)
        t[:, 0] = 0                                                  # all A
        if W > 3:
            t[:, 1], t[:, 2], t[:, 3] = 4, 11, 4                     # all '-', all N, one C among '-'
            t[R // 2, 3] = 1
        out.append(t)
    return out


def check_weighted_columns(be):
    rng = np.random.default_rng(12)
    shapes = [(R, W) for R in (1, 2, 300) for W in (1, 255, 256, 257)]
    texts = _texts(rng, shapes)
    # all weights 1: mprg_prog_columns, byte for byte
    plain = _columns(be, texts)
    ones = _columns(be, texts, [np.ones(len(t), np.int64) for t in texts])
    assert not any(plain[0]) and ones[0] == plain[0] and (ones[1] == plain[1]).all()
    # weights 1 to 5: the unweighted call on the text with row r written w_r times
    weights = [rng.integers(1, 6, len(t)) for t in texts]
    got = _columns(be, texts, weights)
    want = _columns(be, [np.repeat(t, w, axis=0) for t, w in zip(texts, weights)])
    assert not any(got[0]) and not any(want[0]) and (got[1] == want[1]).all()
    assert any(int(w.sum()) % 2 and int(w.sum()) > len(w) for w in weights)
    # a weight sum of exactly 2^20, in two rows and in three hundred
    tall = _texts(rng, [(2, 6), (300, 5)])
    tall[0][0, 4], tall[0][1, 4], tall[0][:, 5] = 4, 2, (1, 4)        # the light row's cells decide a quotient
    w_tall = [np.array([(1 << 20) - 1, 1]), np.concatenate([np.full(299, 3495), [(1 << 20) - 299 * 3495]])]
    assert all(int(w.sum()) == 1 << 20 and w.min() >= 1 for w in w_tall)
    got = _columns(be, tall, w_tall)
    want = _columns(be, [np.repeat(t, w, axis=0) for t, w in zip(tall, w_tall)])
    assert not any(got[0]) and not any(want[0]) and (got[1] == want[1]).all()


def check_weighted_refusals(be):
    t = [pc.codes(["ACGTA", "AC-TA", "ACGTN"])]
    ok = _columns(be, t, [np.array([2, 1, 3])])
    assert ok[0] == [0, 0] and not (ok[1] == POISON).all()

    def refused(code=1, **kw):
        status, raw, _ = _columns(be, t, **kw)
        assert status == [code, code] and (raw == POISON).all(), kw
    refused(weights=[np.array([2, 0, 4])])                               # a weight below 1, the sum as stated
    refused(weights=[np.array([2, -1, 5])])
    refused(weights=[np.array([2, 1, 3])], sums=[5])                     # the stated sum is not the sum
    refused(weights=[np.array([2, 1, 3])], sums=[7])
    refused(weights=[np.array([1 << 20, 1, 1])])                         # more than 2^20 rows
    refused(weights=[np.array([2, 1, 3])], weights_words=2)              # the weights end outside their buffer
    refused(weights=[np.array([2, 1, 3])], woffs=[1])
    refused(weights=[np.array([2, 1, 3])], woffs=[-1])


# ---- whole MSAs
def _with_copies(rng, seqs, n):
    """n copies of records picked at random, put at random places behind the first record."""
    out = list(seqs)
    for _ in range(n):
        out.insert(rng.randint(1, len(out)), rng.choice(out))
    return out


@functools.lru_cache(maxsize=None)
def loci():
    """Small loci, 50-300 nt: clade and mutated families with copies injected (copies of the centre among them), a locus of one
    class, two identical records, copies of empty records, and a locus without duplicates."""
    rng = random.Random(19)
    out = []
    for seed, n, dups in ((1, 8, 6), (2, 10, 12), (3, 6, 18)):
        out.append(_with_copies(rng, pr.clade_locus(seed, n, L=(50, 300)), dups))
    fam = pr.clade_locus(4, 7, L=(60, 120))
    c = sr.centre([sr.normalise(s) for s in fam])
    out.append(fam[:3] + [fam[c]] * 2 + fam[3:] + [fam[c], fam[0], fam[c]])   # copies of the centre, in front of it and behind it
    one = "".join(rng.choice("ACGT") for _ in range(90))
    out.append([one] * 12)                                               # one class
    out.append([one[:50], one[:50]])                                     # two identical records
    out.append(["", one[:60], "--", sr.mutate(rng, one[:60]), one[:60], "", sr.mutate(rng, one[:60]), one[:60].lower()] * 2)
    base = "".join(rng.choice("ACGT") for _ in range(150))
    fam = [sr.mutate(rng, base, 0.08, 0.03) for _ in range(5)] + ["ACGTNNRYACGTKMSWACGT" * 3]
    out.append(_with_copies(rng, fam, 9))                                # ambiguity codes in a class
    out.append(pr.clade_locus(5, 12, L=(50, 300)))                       # no duplicates
    assert len(set(out[-1])) == len(out[-1])
    return out


@functools.lru_cache(maxsize=None)
def spec():
    """Per locus collapse_ref's (rows, (classes, rounds, fell back), merges)."""
    return [cr.progressive(l) for l in loci()]


def n_classes(l):
    """(records, representatives with the empty records among them, classes of non-empty records) of a locus."""
    norm = [sr.normalise(s) for s in l]
    rep = cr.classes(norm)
    return len(l), sum(1 for a, r in enumerate(rep) if r == a), sum(1 for a, r in enumerate(rep) if r == a and norm[a])


def invariants(l, rows, equal_rows=True):
    norm = [sr.normalise(s) for s in l]
    assert [r.replace("-", "") for r in rows] == norm
    assert len({len(r) for r in rows}) == 1 and all(any(r[j] != "-" for r in rows) for j in range(len(rows[0])))
    if equal_rows:
        first = {}
        for s, r in zip(norm, rows):
            assert first.setdefault(s, r) == r


def check_star(be):
    """Star, with and without band and refine: the flag-off bytes, from a pair per class but the centre's."""
    recs = [pc.records(l) for l in loci()]
    want = [sr.star_fasta(r) for r in recs]
    counts = [n_classes(l) for l in loci()]
    for band in (False, True):
        for refine in (0, 2):
            timings, info = {}, []
            off = sa.star_msas(be, recs, band=band, refine=refine)
            on = sa.star_msas(be, recs, band=band, refine=refine, collapse=True, timings=timings, refinement=info)
            assert [sa.msa_fasta(m) for m in on] == [sa.msa_fasta(m) for m in off], (band, refine)
            if not refine:
                assert [sa.msa_fasta(m) for m in on] == want
            assert timings["collapse_records"] == sum(n for n, _, _ in counts) and timings["collapse_classes"] == sum(c for _, c, _ in counts)
            assert timings["collapse_pairs"] == sum(c - 1 for _, _, c in counts) < sum(n for n, _, _ in counts) - len(counts) - 40
            assert timings["collapse_s"] > 0
            for l, m in zip(loci(), on):
                invariants(l, m.rows_as_strings())


def check_progressive(be, **kw):
    """Progressive: collapse_ref's rows from a merge per class but one; band the same bytes; equal rows for equal sequences, also
    after refine; a locus without duplicates keeps its --progressive bytes."""
    recs = [pc.records(l) for l in loci()]
    timings, info = {}, []
    msas = sa.star_msas(be, recs, progressive=True, collapse=True, progression=info, timings=timings, **kw)
    for l, m, got, (rows, want, _) in zip(loci(), msas, info, spec()):
        assert m.rows_as_strings() == rows, l
        assert got == want, l
        assert m.descriptions == [t for t, _ in pc.records(l)]
        invariants(l, rows)
    assert timings["collapse_merges"] == sum(m for _, _, m in spec()) == sum(n_classes(l)[2] - 1 for l in loci())
    assert timings["collapse_classes"] == sum(n_classes(l)[1] for l in loci()) and timings["collapse_s"] > 0
    plain = sa.star_msas(be, recs, progressive=True, **kw)
    assert sa.msa_fasta(msas[-1]) == sa.msa_fasta(plain[-1]) and msas[-1].rows_as_strings() == pr.progressive_rows(loci()[-1])
    text = [sa.msa_fasta(m) for m in msas]
    counters = {}
    banded = sa.star_msas(be, recs, progressive=True, collapse=True, band=True, timings=counters, **kw)
    assert [sa.msa_fasta(m) for m in banded] == text and counters["prog_band_merges"] == timings["collapse_merges"]
    refined = []
    for band in (False, True):
        info = []
        refined.append(sa.star_msas(be, recs, progressive=True, collapse=True, refine=2, refinement=info, band=band, **kw))
        for l, m in zip(loci(), refined[-1]):
            invariants(l, m.rows_as_strings())
    assert [sa.msa_fasta(m) for m in refined[0]] == [sa.msa_fasta(m) for m in refined[1]]
    assert any(a for a, _, _ in info) and [sa.msa_fasta(m) for m in refined[0]] != text


@functools.lru_cache(maxsize=None)
def flipped_loci():
    """Loci with reverse-complemented copies: a record and its rc fall into one class once the records are oriented."""
    rng = random.Random(23)
    out = []
    for seed in (6, 7, 8):
        fam = pr.clade_locus(seed, 6, L=(80, 200))
        l = list(fam)
        for _ in range(7):
            s = rng.choice(fam)
            l.insert(rng.randint(1, len(l)), st.rc(s) if rng.random() < 0.6 else s)
        out.append(l)
    return out


def check_adjust_direction(be):
    recs = [pc.records(l) for l in flipped_loci()]
    off = sa.star_msas(be, recs, adjust_direction=True)
    timings = {}
    on = sa.star_msas(be, recs, adjust_direction=True, collapse=True, timings=timings)
    assert [(m.descriptions, m.rows_as_strings()) for m in on] == [(m.descriptions, m.rows_as_strings()) for m in off]
    n_rev = 0
    msas = sa.star_msas(be, recs, adjust_direction=True, progressive=True, collapse=True)
    for l, m in zip(flipped_loci(), msas):
        rev, _, ori = st.oriented(l)
        assert len(set(ori)) < len(set(l))                           # classes that exist only after the orientation
        assert m.descriptions == st.titles(pc.records(l), rev) and m.rows_as_strings() == cr.progressive(ori)[0]
        invariants(ori, m.rows_as_strings())
        n_rev += sum(rev)
    assert n_rev >= 5
    assert timings["collapse_classes"] == sum(len(set(st.oriented(l)[2])) for l in flipped_loci())


def check_leaf_limit(be):
    """More than max_leaves non-empty RECORDS, however few classes: the star MSA, reported."""
    ls = loci()
    recs = [pc.records(l) for l in ls]
    info = []
    msas = sa.star_msas(be, recs, progressive=True, collapse=True, progression=info, max_leaves=3)
    star = sa.star_msas(be, recs)
    fell = 0
    for l, m, s, got in zip(ls, msas, star, info):
        rows, want, _ = cr.progressive(l, max_leaves=3)
        assert m.rows_as_strings() == rows and got == want
        if want[2]:
            fell += 1
            assert sa.msa_fasta(m) == sa.msa_fasta(s)
    assert 3 <= fell < len(ls)
    assert info[4] == (12, 0, True) and n_classes(ls[4])[2] == 1    # one class, twelve records: over the limit all the same
    assert info[5] == (1, 0, False)


def write_inputs(src):
    """A few loci as unaligned FASTA files under src: per file name the MSA text --progressive --collapse-identical writes."""
    want = {}
    for k, l in enumerate(loci()[:2] + loci()[4:7]):
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(l)]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"gene{k}.fa"] = cr.progressive_fasta(recs)
    return want
