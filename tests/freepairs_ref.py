"""Test-side statement of "Free end pairs" (make_prg_amd/from_msa/star_align.py) in plain Python on top of
tests/align_ref.py (the profile, the merge), tests/endgap_ref.py (the walk back with free end runs), tests/star_ref.py and
tests/refine_ref.py: the pair DP with its four boundary changes cell by cell (`align_pair`, over a band or the whole matrix) and by
rows in NumPy (`align_pair_np`; the emulated tests pin it to the cell form and to endgap_ref.align_profiles with the sequence as a
one-row X), the star MSA and the refinement built on it, the counted bound {SB', m', z}, U(w), w* by linear search and the two-pass
rule.  Every DP takes endgap (False: the function is align_ref's / band_ref's, which the tests pin)."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import align_ref as ar
from tests import band_ref as br
from tests import endgap_ref as eg
from tests import refine_ref as rr
from tests import star_ref as sr

NEG, OPEN, INS = ar.NEG, ar.OPEN, ar.INS
W0 = br.W0
T = 640                       # the threshold of the counted bound: a design constant, not part of any result


def _prepared(rows, seq):
    return [r.upper() for r in rows], seq.replace("-", "").upper()


# ---- the DP, cell by cell
def cells(rows: Sequence[str], seq: str, dlo: Optional[int] = None, dhi: Optional[int] = None, endgap: bool = True):
    """H, D, I of the spec's recurrence over the cells with dlo <= j - i <= dhi (None: the whole matrix; every other cell NEG), with
    the walk's costs: endgap_ref._walk's arguments."""
    rows, seq = _prepared(rows, seq)
    P, Dc = ar.profile(rows)
    n, C = len(seq), len(Dc)
    dlo, dhi = (-n, C) if dlo is None else br.clamp(n, C, dlo, dhi)
    inside = lambda i, j: dlo <= j - i <= dhi          # noqa: E731
    # what a D op into column j (1-based) costs in row i, to extend and to open; likewise an I op into row i in column j
    d_cost = lambda i, j: (0, 0) if endgap and i in (0, n) else (Dc[j - 1], OPEN + Dc[j - 1])   # noqa: E731
    i_cost = lambda i, j: (0, 0) if endgap and j in (0, C) else (INS, OPEN + INS)               # noqa: E731
    sc = lambda i, j: P[j][seq[i]]                     # noqa: E731
    H = [[NEG] * (C + 1) for _ in range(n + 1)]
    D = [[NEG] * (C + 1) for _ in range(n + 1)]
    I = [[NEG] * (C + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for j in range(1, C + 1):
        if inside(0, j):
            ext, opn = d_cost(0, j)
            D[0][j] = max(D[0][j - 1] + ext, H[0][j - 1] + opn)
            H[0][j] = D[0][j]
    for i in range(1, n + 1):
        if inside(i, 0):
            ext, opn = i_cost(i, 0)
            I[i][0] = max(I[i - 1][0] + ext, H[i - 1][0] + opn)
            H[i][0] = I[i][0]
        for j in range(max(1, i + dlo), min(C, i + dhi) + 1):
            ext, opn = d_cost(i, j)
            D[i][j] = max(D[i][j - 1] + ext, H[i][j - 1] + opn)
            ext, opn = i_cost(i, j)
            I[i][j] = max(I[i - 1][j] + ext, H[i - 1][j] + opn)
            H[i][j] = max(H[i - 1][j - 1] + sc(i - 1, j - 1), D[i][j], I[i][j])
    if endgap:                                           # the boundary the spec states in closed form
        assert all(H[0][J] == D[0][J] == 0 for J in range(1, min(C, dhi) + 1))
        assert all(H[i][0] == I[i][0] == 0 for i in range(1, min(n, -dlo) + 1))
    return H, D, I, sc, d_cost, i_cost, n, C


def align_pair(rows: Sequence[str], seq: str, dlo: Optional[int] = None, dhi: Optional[int] = None, endgap: bool = True) -> Tuple[str, int]:
    """(ops, score) cell by cell over the (clamped) band; None: the whole matrix.  The walk back is endgap_ref's: from (n, C) in
    state H; diagonal, then D, then I; extend before open, also where both are free."""
    got = cells(rows, seq, dlo, dhi, endgap)
    return eg._walk(*got), got[0][got[6]][got[7]]


def ties_with_a_free_run(rows: Sequence[str], seq: str) -> bool:
    """At (n, C) the diagonal ties with the free run of the last row or of the last column."""
    H, D, I, sc, _, _, n, C = cells(rows, seq)
    return n > 0 and H[n - 1][C - 1] + sc(n - 1, C - 1) == H[n][C] and H[n][C] in (D[n][C], I[n][C])


# ---- the DP by rows
def align_pair_np(rows: Sequence[str], seq: str, band: Optional[Tuple[int, int]] = None, endgap: bool = True) -> Tuple[str, int]:
    """align_pair by rows (band_ref.align_pair_banded_np's form): band: (dlo, dhi), the cells outside it FAR below NEG."""
    rows, seq = _prepared(rows, seq)
    Pv, amb, Dc = br._profile_np(rows)
    n, C = len(seq), len(Dc)
    dlo, dhi = (-n, C) if band is None else br.clamp(n, C, *band)
    FAR = -(1 << 60)
    S = np.concatenate([[0], np.cumsum(Dc)])
    cols = np.arange(C + 1)
    H = np.full((n + 1, C + 1), FAR, np.int64)
    D = np.full((n + 1, C + 1), FAR, np.int64)
    I = np.full((n + 1, C + 1), FAR, np.int64)
    D[0, 1:] = np.where(cols[1:] <= dhi, 0 if endgap else OPEN + S[1:], FAR)
    H[0] = D[0]
    H[0, 0] = 0
    sc = [None] * n
    for i in range(1, n + 1):
        inside = (cols - i >= dlo) & (cols - i <= dhi)
        I[i] = np.where(inside, np.maximum(I[i - 1] + INS, H[i - 1] + OPEN + INS), FAR)
        if endgap:                                       # column 0 and column C: free to extend, free to open
            for j in (0, C):
                if inside[j]:
                    I[i, j] = max(I[i - 1, j], H[i - 1, j])
        sc[i - 1] = Pv.get(seq[i - 1], amb)
        diag = np.full(C + 1, FAR, np.int64)
        diag[1:] = H[i - 1, :-1] + sc[i - 1]
        hp = np.where(inside, np.maximum(diag, I[i]), FAR)          # H without D (column 0: H[i][0] = I[i][0])
        if endgap and i == n:                            # row n: D[n][j] = max(D[n][j-1], H[n][j-1])
            D[i, 1:] = np.where(inside[1:], np.maximum.accumulate(hp[:-1]), FAR)
        else:
            D[i, 1:] = np.where(inside[1:], S[1:] + OPEN + np.maximum.accumulate(hp[:-1] - S[:-1]), FAR)
        H[i] = np.maximum(hp, D[i])
    d_cost = lambda i, j: (0,) if endgap and i in (0, n) else (int(Dc[j - 1]),)   # noqa: E731
    i_cost = lambda i, j: (0,) if endgap and j in (0, C) else (INS,)              # noqa: E731
    return eg._walk(H, D, I, lambda i, j: int(sc[i][j]), d_cost, i_cost, n, C), int(H[n, C])


def align_pair_banded_np(rows: Sequence[str], seq: str, dlo: int, dhi: int, endgap: bool = True) -> Tuple[str, int]:
    return align_pair_np(rows, seq, (dlo, dhi), endgap)


# ---- whole loci
def star_rows(seqs: Sequence[str], endgap: bool = True) -> Tuple[int, List[str]]:
    """star_ref.star_rows with every pair an overlap alignment: (centre, the MSA's rows in input order)."""
    seqs = [sr.normalise(s) for s in seqs]
    c = sr.centre(seqs)
    if c < 0:
        raise ValueError("every sequence is empty")
    others = [a for a in range(len(seqs)) if a != c]
    C = len(seqs[c])
    ops = [align_pair_np([seqs[c]], seqs[a], endgap=endgap)[0] if seqs[a] else "D" * C for a in others]
    merged = ar.merge([seqs[c]], [seqs[a] for a in others], ops)
    rows = [None] * len(seqs)
    rows[c] = merged[0]
    for a, r in zip(others, merged[1:]):
        rows[a] = r
    return c, rows


def star_fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --free-end-pairs --msa-dir` writes for a locus."""
    _, rows = star_rows([s for _, s in records])
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))


def one_round(rows: Sequence[str], endgap: bool = True) -> List[str]:
    """refine_ref.one_round with every realignment an overlap alignment."""
    R, W = len(rows), len(rows[0])
    seqs = [r.replace("-", "") for r in rows]
    filled = [a for a in range(R) if seqs[a]]
    ops = [align_pair_np([rows[b] for b in range(R) if b != a], seqs[a], endgap=endgap)[0] for a in filled]
    merged = ar.merge(["-" * W], [seqs[a] for a in filled], ops)[1:]
    width = len(merged[0])
    out = ["-" * width] * R
    for a, r in zip(filled, merged):
        out[a] = r
    return rr.drop_empty_columns(out)


def refine_rows(rows: Sequence[str], n_rounds: int, endgap: bool = True) -> Tuple[List[str], int, List[int]]:
    """refine_ref.refine_rows over one_round above: the objective S and the acceptance rule are refine_ref's, unchanged."""
    rows = list(rows)
    trail = [rr.objective(rows)]
    if not rr.refinable(rows):
        return rows, 0, trail
    for _ in range(n_rounds):
        new = one_round(rows, endgap)
        s = rr.objective(new)
        if s <= trail[-1]:
            break
        rows = new
        trail.append(s)
    return rows, len(trail) - 1, trail


def refine_pairs(rows: Sequence[str], n_rounds: int) -> int:
    """The pair alignments refine_rows runs: per round tried (accepted or not) one per non-empty row."""
    rows = list(rows)
    if not rr.refinable(rows):
        return 0
    filled = sum(1 for r in rows if r.replace("-", ""))
    _, acc, _ = refine_rows(rows, n_rounds)
    return filled * min(n_rounds, acc + 1)


# ---- the certificate
def b_prime(rows: Sequence[str]) -> List[int]:
    """B'_j = max(B_j, 0) per column, B_j = max(max_x P[j][x], Dc[j])."""
    Pv, amb, Dc = br._profile_np([r.upper() for r in rows])
    B = np.maximum(np.maximum.reduce([Pv[x] for x in "ACGT"] + [amb]), Dc)
    return np.maximum(B, 0).tolist()


def bounds(rows: Sequence[str]) -> Tuple[int, int, int]:
    """(SB' = sum_j B'_j, m' = the smallest B'_j >= T or 0 if there is none, z = the columns with B'_j < T)."""
    B = b_prime(rows)
    big = [b for b in B if b >= T]
    return sum(B), min(big) if big else 0, len(B) - len(big)


def U(SB: int, m: int, z: int, n: int, C: int, w: int) -> int:
    """The most a path that touches a diagonal beyond half-width w can score: it skips at least k = max(0, Delta) + w + 1 of the
    profile's columns, at most z of them below T, every other one worth m' or more."""
    return SB - m * max(0, max(0, C - n) + w + 1 - z)


def U_sorted(rows: Sequence[str], n: int, w: int) -> int:
    """endgap_ref.U's sharper form, SB' less the k smallest B'_j: the counted U is never below it."""
    B = sorted(b_prime(rows))
    return sum(B) - sum(B[:max(0, len(B) - n) + w + 1])


def wstar(SB: int, m: int, z: int, n: int, C: int, S0: int) -> int:
    """The smallest w >= 0 with U(w) < S0, by linear search; min(n, C) if none is."""
    for w in range(min(n, C)):
        if U(SB, m, z, n, C, w) < S0:
            return w
    return min(n, C)


def two_pass(rows: Sequence[str], seq: str, w0: int = W0):
    """band_ref.two_pass with the free ends and the counted U: ((ops, score), second pass run, sent to the full DP, cells)."""
    seq = seq.replace("-", "").upper()
    n, C = len(seq), len(rows[0])
    b = bounds(rows)
    b1 = br.band(n, C, w0, w0)
    if not br.band_helps(n, C, *b1):
        return align_pair_np(rows, seq), False, True, n * C
    res = align_pair_banded_np(rows, seq, *b1)
    cells = br.band_cells(n, C, *b1)
    w = wstar(*b, n, C, res[1])
    if w <= w0:
        return res, False, False, cells
    b2 = br.band(n, C, w, w)
    if not br.band_helps(n, C, *b2):
        return align_pair_np(rows, seq), False, True, cells + n * C
    return align_pair_banded_np(rows, seq, *b2), True, False, cells + br.band_cells(n, C, *b2)
