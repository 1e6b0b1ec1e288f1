"""What the emulated and the GPU tests of `from_msa --unaligned --free-end-pairs` share (the spec: star_align.py, "Free end
pairs"; its plain-Python statement: tests/freepairs_ref.py): the pairs of the DP check (strip, ring and row-buffer edges, fragments,
overhangs, unrelated pairs, ties between a free run and a match, ambiguity codes, the multi-row profiles of a refine round), the
banded entry, the bounds entry, the two passes of pairs_on_device, the status codes, whole loci with every flag the feature
composes with, the four fragment loci of the finding and the command line's inputs."""
import functools
import random
from collections import Counter

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from make_prg_amd.utils.synthetic import fragment_locus
from tests import align_ref as ar
from tests import band_ref as br
from tests import compare_ref as cmp
from tests import endgap_common as egc
from tests import endgap_ref as eg
from tests import freepairs_ref as fp
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import star_ref as sr
from tests import strand_ref as st

STRIP_N, EDGE_C = (1, 2, 63, 64, 65, 128, 130), (1, 2, 63, 64, 65, 127, 128, 129, 200)
ENTRIES = ("mprg_align_pairs_endgap", "mprg_align_pairs_endgap_banded", "mprg_align_bounds_endgap")


def _dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


class Device:
    """The pairs (leaf rows, sequence), a leaf each, as the entries take them: the profiles written by mprg_align_profiles, the
    sequences' codes in one buffer."""

    def __init__(self, be, pairs):
        self.be, self.n = be, len(pairs)
        leaves = [pc.codes([r.upper() for r in rows]) for rows, _ in pairs]
        seqs = [pa._codes(s, "test") for _, s in pairs]
        shapes = np.array([m.shape for m in leaves], np.int64)
        R, C = shapes[:, 0], shapes[:, 1]
        self.C, self.pn = C, np.array([len(s) for s in seqs], np.int64)
        leaf_tab = np.stack([sa.exclusive_sum(R * C), R, C, sa.exclusive_sum(6 * C)], 1).astype(np.int64)
        work = sa._tile_work(C)
        self.d_leaves, self.d_prof = be.upload(leaf_tab), be.empty(4 * int((6 * C).sum()))
        d_cells, d_work = be.upload(np.concatenate([m.reshape(-1) for m in leaves])), be.upload(work)
        be.call("mprg_align_profiles", be.ptr(d_cells), be.ptr(self.d_leaves), be.ptr(d_work), len(work), be.ptr(self.d_prof), be.stream)
        self.d_seqs = be.upload(np.concatenate(seqs + [np.zeros(1, np.uint8)]).astype(np.uint8))
        self.seq_off, self.ops_off = sa.exclusive_sum(self.pn), sa.exclusive_sum(self.pn + C)

    def run(self, bands=None):
        """One launch of mprg_align_pairs_endgap (bands: of its banded form, a (dlo, dhi) per pair): per pair (status, ops, score)."""
        be, pn, C = self.be, self.pn, self.C
        if bands is None:
            call, words, cols = ENTRIES[0], pa.workspace_words_v(pn, C), ()
        else:
            b = np.array(bands, np.int64).reshape(-1, 2)
            ok = (b[:, 0] <= np.minimum(0, C - pn)) & (b[:, 1] >= np.maximum(0, C - pn))
            words = np.where(ok, pa.band_workspace_words(pn, C, np.maximum(b[:, 0], -pn), np.minimum(b[:, 1], C)), 64)
            call, cols = ENTRIES[1], (b[:, 0], b[:, 1])
        ptab = np.stack([np.arange(self.n), self.seq_off, pn, sa.exclusive_sum(words), self.ops_off, *cols], 1).astype(np.int64)
        ops_bytes = int((pn + C).sum())
        d_ops, d_out, d_ws, d_pairs = be.empty(ops_bytes), be.empty(12 * self.n), be.empty(4 * int(words.sum())), be.upload(ptab)
        be.call(call, be.ptr(self.d_prof), be.ptr(self.d_leaves), self.n, be.ptr(self.d_seqs), be.ptr(d_pairs), self.n, be.ptr(d_ws),
                int(words.sum()), be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
        res = be.download(d_out, np.int32, 3 * self.n).reshape(-1, 3)
        ops = be.download(d_ops, np.uint8, ops_bytes)
        return [(int(s), ops[o:o + k][::-1].tobytes().decode(), int(sc)) for (s, sc, k), o in zip(res.tolist(), self.ops_off.tolist())]

    def bounds(self):
        be = self.be
        d_bounds = be.empty(24 * self.n)
        be.call(ENTRIES[2], be.ptr(self.d_prof), be.ptr(self.d_leaves), self.n, be.ptr(d_bounds), be.stream)
        return be.download(d_bounds, np.int64, 3 * self.n).reshape(-1, 3)


# ---- 2. the DP against the reference
def refine_profile(rng, R, C, gap):
    """The rows a refine round aligns one row against: R rows of C columns, a share `gap` of the cells '-', no all-gap column."""
    return tuple(pr.random_profiles(rng, R, C, gap, amb=0.03))


@functools.lru_cache(maxsize=None)
def dp_pairs():
    """(leaf rows, sequence): every n of the strip edges against every C of the ring and row-buffer edges (the profile one ACGT row,
    or a refine round's R - 1 in {2, 5} rows with gap shares 0.1 and 0.7; the sequence related to it or not); a fragment of the
    centre at its start, in its middle and at its end (n << C); the centre as a fragment of the sequence with overhang at both ends
    (n > C); unrelated pairs; tandem repeats, where a free run ties with a match; ambiguity codes and N on both sides."""
    rng = random.Random(53)
    out = []
    for k, (n, C) in enumerate((n, C) for n in STRIP_N for C in EDGE_C):
        kind = k % 3
        rows = (_dna(rng, C),) if kind == 0 else refine_profile(rng, (2, 5)[k % 2], C, (0.1, 0.7)[(k // 2) % 2])
        root = rows[0].replace("-", "") or "A"
        if k % 4 == 3:
            s = _dna(rng, n)                                                     # unrelated
        else:                                                                    # a piece of the first row, mutated, cut or padded to n
            a = rng.randint(0, max(0, len(root) - n))
            s = (sr.mutate(rng, root[a:a + n], 0.05, 0.03) + _dna(rng, n))[:n]
        out.append((rows, s))
    centre = _dna(rng, 300)
    rel = [sr.mutate(rng, centre, 0.04, 0.02) for _ in range(3)]
    for a, m in ((0, 40), (130, 45), (len(rel[0]) - 50, 50)):                   # a fragment of the centre: start, middle, end
        out.append(((centre,), rel[0][a:a + m]))
        out.append(((centre,), centre[min(a, 250):min(a, 250) + m]))
    out.append(((centre[90:150],), rel[1]))                                      # the centre as a fragment of the sequence
    out.append(((centre[100:165],), _dna(rng, 70) + sr.mutate(rng, centre[100:165], 0.05, 0.02) + _dna(rng, 64)))
    out.append(((centre[:180],), rel[2][120:]))                                  # the end of the centre against the start of the sequence
    out.append(((centre[120:],), rel[2][:180]))
    for n, C in ((40, 70), (70, 40), (130, 129)):                                # unrelated
        out.append(((_dna(rng, C),), _dna(rng, n)))
    for unit, a, b in (("A", 1, 2), ("A", 2, 1), ("AC", 3, 5), ("ACG", 22, 24), ("ACGT", 17, 16), ("AC", 33, 31)):   # ties
        out.append(((unit * b,), unit * a))
        out.append(((unit * b, unit * b, unit * b), unit * a))
    out.append((("ACGTRYKMSWNACGTTTGACCA",), "ACGTNNKMSWNACGTTTGACC"))           # ambiguity codes and N
    out.append((("NNNNNNNN",), "ACGTNNAC"))
    out.append((("ACGTNACGTNNACGTAC", "ACGTAACGTRYACGTAC"), "NNACGTNACG"))
    out.append(((centre[:150].replace("G", "N"),), rel[0][20:90]))
    out.append((refine_profile(rng, 5, 140, 0.7), _dna(rng, 30, "ACGTN")))
    return out


@functools.lru_cache(maxsize=None)
def dp_cases():
    """((rows, sequence), freepairs_ref's (ops, score)) of dp_pairs."""
    return [(p, fp.align_pair_np(*p)) for p in dp_pairs()]


def check_dp(be):
    cases = dp_cases()
    shapes = {(len(s), len(rows[0])) for (rows, s), _ in cases}
    assert {(n, C) for n in STRIP_N for C in EDGE_C} <= shapes
    assert {len(rows) for (rows, _), _ in cases} >= {1, 2, 5}
    off = [ar.align_pair_np(rows, s) for (rows, s), _ in cases]
    assert sum(want != o for (_, want), o in zip(cases, off)) >= 40             # the free ends change results, or nothing is tested
    assert sum(fp.ties_with_a_free_run(rows, s) for (rows, s), _ in cases) >= 6
    assert sum(want[0].startswith("DDDDD") or want[0].startswith("IIIII") for _, want in cases) >= 10
    assert sum(want[0].endswith("DDDDD") or want[0].endswith("IIIII") for _, want in cases) >= 10
    got = Device(be, [p for p, _ in cases]).run()
    for ((rows, s), want), g in zip(cases, got):
        assert g == (0,) + want, (len(s), len(rows), len(rows[0]))
    # the identity of the spec: the profile-profile entry with free end gaps, the sequence as a one-row X
    merged = sa.merge_profiles(be, [(pc.codes([s.upper()]), pc.codes([r.upper() for r in rows])) for (rows, s), _ in cases], free_end_gaps=True)
    for (_, want), (ops, score) in zip(cases, merged):
        assert (ops.decode(), score) == want


# ---- 3. the banded entry
@functools.lru_cache(maxsize=None)
def band_cases():
    """((rows, sequence), (dlo, dhi), the reference's banded (ops, score), the full DP's score): dp_pairs under half-widths 0, 3 and
    9, one-sided bands, the band open to [-n, C] and bands wider than the matrix (clamped)."""
    out = []
    for k, p in enumerate(dp_pairs()):
        n, C = len(p[1]), len(p[0][0])
        lo, hi = min(0, C - n), max(0, C - n)
        for band in ((lo - (0, 3, 9)[k % 3], hi + (0, 3, 9)[(k // 3) % 3]), ((lo - 5, hi), (lo, hi + 5), (-n, C), (-10 ** 6, 10 ** 6))[k % 4]):
            out.append((p, band))
    full = {p: w for p, w in dp_cases()}
    return [(p, b, fp.align_pair_banded_np(*p, *b), full[p][1]) for p, b in out]


def check_banded(be):
    cases = band_cases()
    assert sum(want[1] < whole for _, _, want, whole in cases) >= 20            # the band loses
    assert sum(b == (-len(p[1]), len(p[0][0])) for p, b, _, _ in cases) >= 10 and sum(b[0] == -10 ** 6 for _, b, _, _ in cases) >= 10
    got = Device(be, [p for p, _, _, _ in cases]).run([b for _, b, _, _ in cases])
    full = {p: w for p, w in dp_cases()}
    for (p, b, want, _), g in zip(cases, got):
        assert g == (0,) + want, (len(p[1]), len(p[0]), len(p[0][0]), b)
        if b[0] <= -len(p[1]) and b[1] >= len(p[0][0]):
            assert g[1:] == full[p]
    # a band without (0, 0) or (n, C): C - n = 3: dhi < 3; C - n = -2: dlo > -2; dlo > 0; dhi < 0
    probs = [(("ACGTACGTAC",), s) for s in ("ACGTACG", "ACGTACGTACGG", "ACGTACGTAC", "ACGTACGTAC")]
    assert [g[0] for g in Device(be, probs).run([(-2, 2), (-1, 5), (1, 3), (-3, -1)])] == [3, 3, 3, 3]


# ---- 4. the bounds entry
@functools.lru_cache(maxsize=None)
def bound_profiles():
    """Leaves at C in {1, 63, 64, 65, 200}: one ACGT row (z = 0, m' = 1 280), the same with N cells (z > 0), a refine round's sparse
    rows (columns with one residue in six land in z), and profiles with no column at or above T (m' = 0): N alone, or every column
    with one residue."""
    rng = random.Random(59)
    out = []
    for C in (1, 63, 64, 65, 200):
        row = _dna(rng, C)
        out.append((row,))
        out.append(("".join("N" if rng.random() < 0.2 or j == C // 2 else ch for j, ch in enumerate(row)),))
        out.append(refine_profile(rng, 6, C, 0.7))
        out.append(refine_profile(rng, 3, C, 0.1))
        out.append(("N" * C,))
        out.append(tuple("".join(row[j] if j % 6 == r else "-" for j in range(C)) for r in range(6)))
    return out


def check_bounds(be):
    leaves = bound_profiles()
    want = [fp.bounds(rows) for rows in leaves]
    assert sum(m == 1280 and z == 0 for _, m, z in want) >= 5 and sum(m > 0 and z > 0 for _, m, z in want) >= 8
    assert sum(m == 0 and z == len(rows[0]) for (_, m, z), rows in zip(want, leaves)) >= 10
    assert any(0 < m < 1280 for _, m, _ in want)
    got = Device(be, [(rows, "A") for rows in leaves]).bounds()
    assert [tuple(g) for g in got.tolist()] == want


def check_widths_formula():
    """certified_widths_endgap against the linear search, scalars and arrays, at, one below and one above every threshold."""
    rng = random.Random(61)
    n_checked = 0
    for rows in bound_profiles() + [refine_profile(rng, 4, 90, 0.4) for _ in range(6)]:
        C = len(rows[0])
        SB, m, z = fp.bounds(rows)
        for n in sorted({1, 2, C // 2 + 1, C, C + 7, 3 * C}):
            top = min(n, C)
            scores = {SB + 5000, SB + 1, SB, SB - 1, -10 ** 8, 0}
            for w in sorted({0, 1, 2, top // 2, top - 1, top} & set(range(top + 1))):
                u = fp.U(SB, m, z, n, C, w)
                scores |= {u - 1, u, u + 1}
            us = [fp.U(SB, m, z, n, C, w) for w in range(top + 2)]
            assert all(a >= b for a, b in zip(us, us[1:])) and us[0] <= SB
            assert all(fp.U(SB, m, z, n, C, w) >= fp.U_sorted(rows, n, w) for w in range(top))   # the sorted sum is the sharper bound
            s = np.array(sorted(scores), np.int64)
            want = [fp.wstar(SB, m, z, n, C, int(x)) for x in s]
            f = lambda v: np.full(len(s), v, np.int64)          # noqa: E731
            wm, wp = pa.certified_widths_endgap(f(n), f(C), f(SB), f(m), f(z), s)
            assert wm.tolist() == want == wp.tolist(), (len(rows), n, C)
            n_checked += len(s)
    assert n_checked >= 1000


# ---- 5. two passes
def excursion(rng, centre, k):
    """A relative of the centre with a run of k inserted residues and, further on, k deleted ones: the path leaves the corridor by k."""
    a = len(centre) // 3
    return centre[:a] + _dna(rng, k) + centre[a:2 * a] + centre[2 * a + k:]


@functools.lru_cache(maxsize=None)
def two_pass_cases():
    """(centre rows, sequence) for pairs_on_device with W0 = 8: near-identical sequences, fragments and overhangs (certified in pass 1),
    diverged ones and excursions (a second pass), unrelated ones and short pairs (the full DP), and leave-one-out profiles."""
    rng = random.Random(67)
    c1, c2 = _dna(rng, 400), _dna(rng, 260)
    probs = []
    for c in (c1, c2):
        probs += [((c,), sr.mutate(rng, c, 0.004, 0.0)) for _ in range(3)]
        probs += [((c,), c[60:200]), ((c,), c[len(c) - 90:]), ((c[80:220],), c)]
        probs += [((c,), sr.mutate(rng, c, 0.05, 0.01)) for _ in range(3)]
        probs += [((c,), excursion(rng, c, 20)), ((c,), sr.mutate(rng, c, 0.1, 0.03)[30:])]
        probs += [((c,), _dna(rng, 200)), ((c[:50],), c[:47])]
    msa = fp.star_rows([c2] + [sr.mutate(rng, c2, 0.03, 0.01) for _ in range(4)])[1]
    probs += [(tuple(msa[:a] + msa[a + 1:]), msa[a].replace("-", "")) for a in range(5)]
    return probs


W0 = 8


@functools.lru_cache(maxsize=None)
def two_pass_spec():
    """The reference's two passes per pair of two_pass_cases, which must give the unbanded result; and the counters they add up to."""
    cases = two_pass_cases()
    res = [fp.two_pass(rows, s, W0) for rows, s in cases]
    assert [r for r, _, _, _ in res] == [fp.align_pair_np(rows, s) for rows, s in cases]
    kinds = Counter("second" if second else "full" if full else "first" for _, second, full, _ in res)
    helped = sum(br.band_helps(len(s), len(rows[0]), *br.band(len(s), len(rows[0]), W0, W0)) for rows, s in cases)
    counters = dict(band_pairs=len(cases), band_second_passes=kinds["second"], band_full_pairs=kinds["full"],
                    band_cells=sum(c for _, _, _, c in res), band_full_cells=sum(len(s) * len(rows[0]) for rows, s in cases))
    return [r for r, _, _, _ in res], kinds, helped, counters


def check_two_pass(be):
    cases = two_pass_cases()
    want, kinds, helped, counters = two_pass_spec()
    # the reference alone: a pair certified in pass 1, a second pass, a pair sent to the full DP after pass 1 and one before it
    assert kinds["first"] >= 3 and kinds["second"] >= 3 and kinds["full"] >= 3 and len(cases) - helped >= 1 and helped - kinds["first"] - kinds["second"] >= 1, kinds
    leaves = [pc.codes(list(rows)) for rows, _ in cases]
    seqs = [[pa._codes(s, "test")] for _, s in cases]
    small = 4 * int(max(pa.workspace_words(len(s), len(rows[0])) for rows, s in cases))      # the largest full DP alone: several launches
    plain = pa.align_batch(be, leaves, seqs, free_ends=True)
    assert [(o.decode(), s) for (o, s), in plain] == want
    for budget in (pa.DEFAULT_BUDGET_BYTES, small):
        got_counters = {}
        got = pa.align_batch(be, leaves, seqs, budget_bytes=budget, band=W0, counters=got_counters, free_ends=True)
        assert [(o.decode(), s) for (o, s), in got] == want
        assert got_counters == counters
    assert pa.align_batch(be, leaves, seqs, band=True, free_ends=True) == plain      # the default w0


# ---- 6. status codes
def check_abi_statuses(be):
    """The two pair entries, handed tables that point outside a buffer, report their status code and write nothing else; the bounds
    entry without leaves writes nothing."""
    POISON = 0x5C
    rows, s = ("ACGTA", "AC-TA", "ACGTN"), "ACTA"
    dev = Device(be, [(rows, s)])

    def untouched(buf, n):
        return (be.download(buf, np.uint8, n) == POISON).all()
    full_need, band_need = int(pa.workspace_words(4, 5)), int(pa.band_workspace_words(4, 5, -4, 5))

    def pairs(call, pair, need, n_leaves=1, leaf=None, ws_words=None, ops_bytes=9):
        d_ws, d_ops, d_out = be.full(4 * need, POISON), be.full(9, POISON), be.full(12, POISON)
        d_leaves = dev.d_leaves if leaf is None else be.upload(np.array([leaf], np.int64))
        d_pairs = be.upload(np.array([pair], np.int64))
        be.call(call, be.ptr(dev.d_prof), be.ptr(d_leaves), n_leaves, be.ptr(dev.d_seqs), be.ptr(d_pairs), 1,
                be.ptr(d_ws), need if ws_words is None else ws_words, be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream)
        return be.download(d_out, np.int32, 3).tolist(), untouched(d_ops, 9) and untouched(d_ws, 4 * need), be.download(d_ops, np.uint8, 9)
    want = fp.align_pair(rows, s)
    for call, need, band in ((ENTRIES[0], full_need, []), (ENTRIES[1], band_need, [-4, 5])):
        out, clean, ops = pairs(call, [0, 0, 4, 0, 0] + band, need)
        assert out == [0, want[1], len(want[0])] and ops[:out[2]][::-1].tobytes().decode() == want[0] and not clean
        out, _, ops = pairs(call, [0, 0, 0, 0, 0] + ([0, 5] if band else []), need)              # n = 0: C D ops, score 0
        assert out == [0, 0, 5] and ops[:5].tobytes() == b"DDDDD"
        for pair, kw, code in (([1, 0, 4, 0, 0], {}, 3), ([-1, 0, 4, 0, 0], {}, 3), ([0, 0, -1, 0, 0], {}, 3),
                               ([0, 0, 4, 0, 0], dict(leaf=(0, 0, 5, 0)), 3), ([0, 0, 4, 0, 0], dict(leaf=(0, 3, 0, 0)), 3),
                               ([0, 0, 4, 64, 0], {}, 2), ([0, 0, 4, 1, 0], {}, 2), ([0, 0, 4, -64, 0], {}, 2), ([0, 0, 4, 0, 1], {}, 2),
                               ([0, 0, 4, 0, -1], {}, 2), ([0, 0, 4, 0, 0], dict(ops_bytes=8), 2), ([0, 0, 4, 0, 0], dict(ws_words=need - 1), 2),
                               ([0, 0, 999_996, 0, 0], {}, 1)):
            b = band if 0 <= pair[2] < 10 else [-999_996, 5] if band else []
            assert pairs(call, pair + b, need, **kw)[:2] == ([code, 0, 0], True), (call, pair, kw)
    for band in ([1, 5], [-4, 0], [2, 1]):                                                       # (0, 0) or (n, C) outside the band
        assert pairs(ENTRIES[1], [0, 0, 4, 0, 0] + band, band_need)[:2] == ([3, 0, 0], True)
    ref = fp.align_pair(rows, s, -1, 2)
    out, _, ops = pairs(ENTRIES[1], [0, 0, 4, 0, 0, -1, 2], band_need)
    assert out == [0, ref[1], len(ref[0])] and ops[:out[2]][::-1].tobytes().decode() == ref[0]
    d_bounds = be.full(24, POISON)
    be.call(ENTRIES[2], be.ptr(dev.d_prof), be.ptr(dev.d_leaves), 0, be.ptr(d_bounds), be.stream)
    assert untouched(d_bounds, 24)
    be.call(ENTRIES[2], be.ptr(dev.d_prof), be.ptr(dev.d_leaves), 1, be.ptr(d_bounds), be.stream)
    assert tuple(be.download(d_bounds, np.int64, 3).tolist()) == fp.bounds(rows)


# ---- 7. whole loci
@functools.lru_cache(maxsize=None)
def loci():
    """star_ref's edge loci, a few of its random ones, a small locus with partial records, and one long enough for the band to help."""
    rng = random.Random(71)
    root = _dna(rng, 220)
    long_one = [sr.mutate(rng, root, 0.03, 0.01) for _ in range(4)] + [root[30:120], root[150:]]
    return sr.edge_loci() + sr.random_loci(11, 6) + [fragment_locus(5, 7, 120, 160, share=0.7)[0], long_one]


@functools.lru_cache(maxsize=None)
def star_spec():
    return [fp.star_rows(l)[1] for l in loci()]


def invariants(seqs, rows):
    """What the flag promises of every MSA."""
    norm = [sr.normalise(s) for s in seqs]
    assert [r.replace("-", "") for r in rows] == norm
    assert len({len(r) for r in rows}) == 1
    assert all(any(r[j] != "-" for r in rows) for j in range(len(rows[0])))
    by_seq = {}
    for s, r in zip(norm, rows):
        assert by_seq.setdefault(s, r) == r                     # identical sequences, identical rows


def star(be, ls, **kw):
    return [m.rows_as_strings() for m in sa.star_msas(be, [pc.records(l) for l in ls], free_end_pairs=True, **kw)]


def check_star(be):
    ls, want = loci(), star_spec()
    assert sum(w != sr.star_rows(l)[1] for l, w in zip(ls, want)) >= 5          # the free ends change MSAs
    timings = {}
    assert star(be, ls, timings=timings) == want
    assert timings["free_end_pair_alignments"] == sum(sum(1 for s in l if sr.normalise(s)) - 1 for l in ls)
    for l, rows in zip(ls, want):
        invariants(l, rows)
    for kw in (dict(band=True), dict(band=8), dict(collapse=True), dict(band=8, collapse=True), dict(budget_bytes=1 << 17, chunk_bytes=1 << 12)):
        timings = {}
        assert star(be, ls, timings=timings, **kw) == want, kw
        if "band" in kw:
            assert timings["band_pairs"] > 0
    # adjust_direction: the orientation (unchanged) first, then the star pass with free pairs over the oriented sequences
    rng = random.Random(73)
    flipped = [st.flip(rng, l)[0] for l in ls]
    info = []
    got = star(be, flipped, adjust_direction=True, orientation=info)
    for l, rows, (rev, how) in zip(flipped, got, info):
        w_rev, w_how, ori = st.oriented(l)
        assert (list(rev), how) == (w_rev, w_how) and rows == fp.star_rows(ori)[1]
    assert sum(any(rev) for rev, _ in info) >= 5


@functools.lru_cache(maxsize=None)
def refine_spec():
    return [fp.refine_rows(rows, 2) for rows in star_spec()]


def check_refine(be):
    ls, want = loci(), refine_spec()
    for kw in (dict(), dict(band=8)):
        info, timings = [], {}
        got = star(be, ls, refine=2, refinement=info, timings=timings, **kw)
        for l, rows, rep, (w_rows, acc, trail) in zip(ls, got, info, want):
            assert rows == w_rows and rep == (acc, trail[0], trail[-1]), l
            invariants(l, rows)
        pairs = sum(sum(1 for s in l if sr.normalise(s)) - 1 + fp.refine_pairs(rows, 2) for l, rows in zip(ls, star_spec()))
        assert timings["free_end_pair_alignments"] == pairs
    assert sum(acc > 0 for _, acc, _ in want) >= 3
    assert sum(w[0] != rr.refine_rows(rows, 2)[0] for w, rows in zip(want, star_spec())) >= 3   # not the charged refine's rows


def prog_loci():
    return pr.table_loci()[:3] + [fragment_locus(5, 7, 120, 160, share=0.7)[0]]


def check_progressive(be):
    """progressive with free_end_gaps and refine = 2: endgap_ref's rows, refined with free pairs; a locus over max_leaves gets the
    star MSA with free pairs."""
    ls = prog_loci()
    info = []
    got = star(be, ls, progressive=True, free_end_gaps=True, refine=2, refinement=info)
    accepted = 0
    for l, rows, rep in zip(ls, got, info):
        w_rows, acc, trail = fp.refine_rows(eg.progressive_rows(l), 2)
        assert rows == w_rows and rep == (acc, trail[0], trail[-1]), l
        invariants(l, rows)
        accepted += acc
    assert accepted >= 2
    prog, timings = [], {}
    got = star(be, ls, progressive=True, max_leaves=7, progression=prog, timings=timings)
    fell = [p[2] for p in prog]
    assert any(fell) and not all(fell)
    for l, rows, f in zip(ls, got, fell):
        assert rows == (fp.star_rows(l)[1] if f else pr.progressive_rows(l)), l
    assert timings["free_end_pair_alignments"] == sum(sum(1 for s in l if sr.normalise(s)) - 1 for l, f in zip(ls, fell) if f)


def check_unique_substring(be):
    """A record that is an exact substring of the centre, occurring once, has its residues in place with no internal gap: 1 280 n
    is the most any path scores, and only an occurrence reaches it."""
    rng = random.Random(79)
    n_checked = 0
    for L, cuts in ((150, ((0, 30), (40, 100), (110, 150))), (70, ((0, 64), (5, 70))), (300, ((100, 165), (236, 300)))):
        root = _dna(rng, L)
        base = [root] + [sr.mutate(rng, root, 0.03, 0.02) for _ in range(3)]
        c = sr.centre(base)
        frags = [base[c][a:b] for a, b in cuts]
        seqs = base + frags
        if sr.centre(seqs) != c or any(base[c].count(f) != 1 for f in frags):
            continue
        for rows in (fp.star_rows(seqs)[1], star(be, [seqs])[0], star(be, [seqs], band=8)[0]):
            centre_at = {j: k for k, j in enumerate(j for j, ch in enumerate(rows[c]) if ch != "-")}
            for (a, b), row in zip(cuts, rows[len(base):]):
                assert [centre_at.get(j) for j, ch in enumerate(row) if ch != "-"] == list(range(a, b))
                n_checked += 1
    assert n_checked >= 15


# ---- 8. flag off
def check_flag_off(be):
    """Without the flag, or with False, the bytes are star_ref's and refine_ref's, and no counter of the flag appears."""
    ls = loci()
    want = [sr.star_rows(l)[1] for l in ls]
    for kw in (dict(), dict(free_end_pairs=False)):
        timings = {}
        msas = sa.star_msas(be, [pc.records(l) for l in ls], timings=timings, **kw)
        assert [m.rows_as_strings() for m in msas] == want and "free_end_pair_alignments" not in timings
        msas = sa.star_msas(be, [pc.records(l) for l in ls], refine=2, timings=timings, band=8, **kw)
        assert [m.rows_as_strings() for m in msas] == [rr.refine_rows(rows, 2)[0] for rows in want] and "free_end_pair_alignments" not in timings
    opts = sa.Options(free_end_pairs=True, progressive=True, free_end_gaps=True)
    assert opts.star().free_end_pairs and not opts.star().free_end_gaps and not sa.Options().free_end_pairs


# ---- 9. the finding
# shared pairs with the truth of fragment_locus(seed, 20, 250, 350), seeds 0-3, as the references give them: (the star MSA, with
# free pairs, star + refine 2, free star + free refine 2, progressive with free end gaps, + refine 2, + free refine 2)
FINDING = ((34341, 37546, 34633, 37586, 38008, 36214, 38008), (37882, 38583, 37780, 38943, 39335, 37665, 39335),
           (28501, 30018, 27820, 29772, 29838, 27676, 29860), (40197, 41120, 40707, 41429, 41555, 41083, 41728))


@functools.lru_cache(maxsize=None)
def finding():
    """Per locus: (sequences, true rows, the seven forms' rows)."""
    out = []
    for seqs, truth, forms in egc.finding():
        star_off, star_on, prog = sr.star_rows(seqs)[1], fp.star_rows(seqs)[1], forms[1]
        out.append((seqs, truth, (star_off, star_on, rr.refine_rows(star_off, 2)[0], fp.refine_rows(star_on, 2)[0],
                                  prog, rr.refine_rows(prog, 2)[0], fp.refine_rows(prog, 2)[0])))
    return out


def check_finding_reference():
    got = tuple(tuple(cmp.by_histogram(rows, truth)[0] for rows in forms) for _, truth, forms in finding())
    print("shared pairs (star, free pairs, star + refine, free star + free refine, prog free end gaps, + refine, + free refine):", got)
    assert all(f[1] > f[0] for f in got)                         # free pairs beat the star MSA
    assert all(f[3] > f[2] and f[6] > f[5] for f in got)         # a free refine beats today's, after the free star and after free end gaps
    assert all(f[6] >= f[4] for f in got)                        # and never falls below its input there
    assert got == FINDING


def check_finding(be):
    ls = finding()
    for k, kw in ((1, dict()), (3, dict(refine=2)), (6, dict(progressive=True, free_end_gaps=True, refine=2, device_tree=True))):
        assert star(be, [s for s, _, _ in ls], band=True, **kw) == [forms[k] for _, _, forms in ls], kw


# ---- 10. the command line
def check_parser(capsys):
    """--free-end-pairs without --unaligned is a parser error; with --unaligned alone it parses."""
    import pytest
    from make_prg_amd import __main__ as cli
    with pytest.raises(SystemExit) as exc:
        cli.main(["from_msa", "-i", "x", "-o", "y", "--free-end-pairs"])
    assert exc.value.code == 2 and "--free-end-pairs needs --unaligned" in capsys.readouterr().err


def check_cli(be, tmp_path, caplog):
    """from_msa.run with --unaligned --free-end-pairs --msa-dir (in process): the files are freepairs_ref's and the log has the flag's
    line once; without the flag the files are star_ref's and the line is absent."""
    import logging
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    ls = [sr.random_loci(11, 6)[2], fragment_locus(5, 7, 120, 160, share=0.7)[0]]
    recs = [[(f"s{i} x", s) for i, s in enumerate(l)] for l in ls]
    for k, r in enumerate(recs):
        (src / f"g{k}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in r))
    old = {f"g{k}.fa": sr.star_fasta(r) for k, r in enumerate(recs)}
    pairs = sum(sum(1 for s in l if sr.normalise(s)) - 1 for l in ls)

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None)
        base.update(kw)
        return Namespace(**base)
    for flag in (True, False):
        caplog.clear()
        d = tmp_path / f"msas{flag}"
        with caplog.at_level(logging.INFO):
            from_msa.run(opts(output_prefix=str(tmp_path / f"o{flag}" / "a"), msa_dir=str(d), free_end_pairs=flag), be)
        got = {p.name: p.read_text() for p in d.iterdir()}
        lines = [r.getMessage() for r in caplog.records if "--free-end-pairs:" in r.getMessage()]
        if flag:
            want = {f"g{k}.fa": fp.star_fasta(r) for k, r in enumerate(recs)}
            assert got == want and got != old and len(lines) == 1 and f"--free-end-pairs: {pairs} pair alignments with free ends" in lines[0]
        else:
            assert got == old and not lines
