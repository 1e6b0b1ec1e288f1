"""Test-side statement of "Free end gaps" (make_prg_amd/from_msa/star_align.py) in plain Python on top of
tests/prog_ref.py and tests/posgap_ref.py: the merge with its four boundary changes cell by cell (`align_profiles_banded`, over a
band or the whole matrix) and by rows in NumPy (`align_profiles_np`, also over weighted rows; the emulated tests pin it to the cell
form), the overlap optimum by its definition (`overlap_score`), the bound U(w) = SB' - LY'(max(0, Delta) + w + 1), w* by linear
search and the two-pass rule.  Every function takes posgap (the opens by occupancy of "Position gaps" inside the matrix) and endgap
(False: the function is prog_ref's / posgap_ref's, which the tests pin)."""
import contextlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import band_ref as br
from tests import posgap_ref as pg
from tests import prog_ref as pr
from tests import progband_ref as pb

NEG, OPEN = pr.NEG, pr.OPEN
W0 = pb.W0


def _opens(X, Y, posgap):
    """(Oc per column of Y, Ox per column of X) as lists: by occupancy, or -704 everywhere."""
    if posgap:
        return pg.opens(X, Y)
    return [OPEN] * len(Y[0]), [OPEN] * len(X[0])


# ---- the DP, cell by cell
def _cells(X, Y, dlo, dhi, posgap, endgap, zero_borders_only=False):
    """H, D, I of the spec's recurrence over the cells with dlo <= j - i <= dhi (every other cell NEG), with the walk's costs.
    zero_borders_only: rows 0 and columns 0 are free, the last row and column are charged like any other (overlap_score's DP)."""
    P, Dc, cols, Ic = pr.column_tables(X, Y)
    Oc, Ox = _opens(X, Y, posgap)
    RX, n, C = len(X), len(cols), len(Dc)
    inside = lambda i, j: dlo <= j - i <= dhi          # noqa: E731
    sc = lambda i, j: pr.column_score(cols[i], P[j], Dc[j], RX)   # noqa: E731
    last = endgap and not zero_borders_only
    # what a D op into column j (1-based) costs in row i, to extend and to open; likewise an I op into row i in column j
    d_cost = lambda i, j: (0, 0) if (endgap and i == 0) or (last and i == n) else (Dc[j - 1], Oc[j - 1] + Dc[j - 1])   # noqa: E731
    i_cost = lambda i, j: (0, 0) if (endgap and j == 0) or (last and j == C) else (Ic[i - 1], Ox[i - 1] + Ic[i - 1])   # noqa: E731
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


def _walk(H, D, I, sc, d_cost, i_cost, n, C):
    """The walk back from (n, C) in state H: diagonal, then D, then I; extend before open (also where both are free)."""
    ops, i, j, st = [], n, C, "H"
    while i > 0 or j > 0:
        if st == "H":
            if i > 0 and j > 0 and H[i - 1][j - 1] + sc(i - 1, j - 1) == H[i][j]:
                ops.append("M")
                i, j = i - 1, j - 1
            elif D[i][j] == H[i][j]:
                st = "D"
            else:
                st = "I"
        elif st == "D":
            ops.append("D")
            st = "D" if D[i][j - 1] + d_cost(i, j)[0] == D[i][j] else "H"
            j -= 1
        else:
            ops.append("I")
            st = "I" if I[i - 1][j] + i_cost(i, j)[0] == I[i][j] else "H"
            i -= 1
    return "".join(reversed(ops))


def align_profiles_banded(X: Sequence[str], Y: Sequence[str], dlo: Optional[int] = None, dhi: Optional[int] = None, posgap: bool = False,
                          endgap: bool = True) -> Tuple[str, int]:
    """(ops, score) cell by cell over the (clamped) band; None: the whole matrix."""
    n, C = len(X[0]), len(Y[0])
    dlo, dhi = (-n, C) if dlo is None else br.clamp(n, C, dlo, dhi)
    got = _cells(X, Y, dlo, dhi, posgap, endgap)
    return _walk(*got), got[0][n][C]


def align_profiles(X: Sequence[str], Y: Sequence[str], posgap: bool = False, endgap: bool = True) -> Tuple[str, int]:
    return align_profiles_banded(X, Y, None, None, posgap, endgap)


def overlap_score(X: Sequence[str], Y: Sequence[str], posgap: bool = False) -> int:
    """The overlap (semi-global) optimum by its definition: the DP with zero borders and every other cell charged as usual, the
    maximum over its last row and its last column."""
    n, C = len(X[0]), len(Y[0])
    H = _cells(X, Y, -n, C, posgap, True, zero_borders_only=True)[0]
    return max(max(H[n]), max(H[i][C] for i in range(n + 1)))


# ---- the DP by rows
def align_profiles_np(X, Y, wx=None, wy=None, band: Optional[Tuple[int, int]] = None, posgap: bool = False, endgap: bool = True) -> Tuple[str, int]:
    """align_profiles by rows (posgap_ref.align_profiles_np's form).  X and Y: row strings, or R x W matrices of cell codes; wx,
    wy: the rows' weights; band: (dlo, dhi), the cells outside it FAR below NEG."""
    P, Pamb, Dc, Oc, cx, ambx, RX, Ic, Ox = pg.tables(X, Y, wx, wy)
    if not posgap:
        Oc, Ox = np.full_like(Oc, OPEN), np.full_like(Ox, OPEN)
    n, C = len(X[0]), len(Y[0])
    dlo, dhi = (-n, C) if band is None else br.clamp(n, C, *band)
    FAR = -(1 << 60)
    S = np.concatenate([[0], np.cumsum(Dc)])
    cols = np.arange(C + 1)
    H = np.full((n + 1, C + 1), FAR, np.int64)
    D = np.full((n + 1, C + 1), FAR, np.int64)
    I = np.full((n + 1, C + 1), FAR, np.int64)
    if endgap:
        D[0, 1:] = np.where(cols[1:] <= dhi, 0, FAR)
    elif C:
        D[0, 1:] = np.where(cols[1:] <= dhi, int(Oc[0]) + S[1:], FAR)
    H[0] = D[0]
    H[0, 0] = 0
    sc = [None] * n
    for i in range(1, n + 1):
        ins, opn = int(Ic[i - 1]), int(Ox[i - 1])
        inside = (cols - i >= dlo) & (cols - i <= dhi)
        I[i] = np.where(inside, np.maximum(I[i - 1] + ins, H[i - 1] + opn + ins), FAR)
        if endgap:                                       # column 0 and column C: free to extend, free to open
            for j in (0, C):
                if inside[j]:
                    I[i, j] = max(I[i - 1, j], H[i - 1, j])
        sc[i - 1] = pr._tdv(sum(int(cx[x][i - 1]) * P[x] for x in "ACGT") + int(ambx[i - 1]) * Pamb + int(cx["-"][i - 1]) * Dc, RX)
        diag = np.full(C + 1, FAR, np.int64)
        diag[1:] = H[i - 1, :-1] + sc[i - 1]
        hp = np.where(inside, np.maximum(diag, I[i]), FAR)
        if endgap and i == n:                            # row n: D[n][j] = max(D[n][j-1], H[n][j-1])
            D[i, 1:] = np.where(inside[1:], np.maximum.accumulate(hp[:-1]), FAR)
        else:
            # (opening from a cell whose H is its D never beats extending that run: Oc <= 0)
            D[i, 1:] = np.where(inside[1:], S[1:] + np.maximum.accumulate(hp[:-1] + Oc - S[:-1]), FAR)
        H[i] = np.maximum(hp, D[i])
    d_cost = lambda i, j: (0,) if endgap and i in (0, n) else (int(Dc[j - 1]),)   # noqa: E731
    i_cost = lambda i, j: (0,) if endgap and j in (0, C) else (int(Ic[i - 1]),)   # noqa: E731
    return _walk(H, D, I, lambda i, j: sc[i][j], d_cost, i_cost, n, C), int(H[n, C])


def align_profiles_banded_np(X, Y, dlo: int, dhi: int, posgap: bool = False, endgap: bool = True) -> Tuple[str, int]:
    return align_profiles_np(X, Y, band=(dlo, dhi), posgap=posgap, endgap=endgap)


# ---- the certificate
def bounds(X, Y) -> Tuple[int, List[int]]:
    """(SB' = sum_j B'_j, the B'_j = max(B_j, 0) in ascending order): no open and nothing of X enters, so both opens share it."""
    P, Pamb, Dc, _, _ = pb._tables_np(X, Y)
    B = np.maximum(np.maximum(np.maximum.reduce([P[x] for x in "ACGT"] + [Pamb]), Dc), 0)
    return int(B.sum()), sorted(B.tolist())


def U(SB: int, loss: List[int], n: int, C: int, w: int) -> int:
    """The most a path that touches a diagonal beyond half-width w can score: it skips at least max(0, Delta) + w + 1 of Y's
    columns (list slices clamp k to C)."""
    return SB - sum(loss[:max(0, C - n) + w + 1])


def wstar(SB, loss, n, C, S0) -> int:
    """The smallest w >= 0 with U(w) < S0, by linear search; min(n, C) if none is."""
    for w in range(min(n, C)):
        if U(SB, loss, n, C, w) < S0:
            return w
    return min(n, C)


def two_pass(X, Y, w0: int = W0, posgap: bool = False):
    """progband_ref.two_pass with the free ends and the new U: ((ops, score), kind, cells computed)."""
    n, C = len(X[0]), len(Y[0])
    full = lambda: align_profiles_np(X, Y, posgap=posgap)              # noqa: E731
    dp = lambda dlo, dhi: align_profiles_banded_np(X, Y, dlo, dhi, posgap)   # noqa: E731
    b = bounds(X, Y)
    b1 = br.band(n, C, w0, w0)
    if not br.band_helps(n, C, *b1):
        return full(), "full", n * C
    res = dp(*b1)
    cells = br.band_cells(n, C, *b1)
    w = wstar(*b, n, C, res[1])
    if w <= w0:
        return res, "first", cells
    b2 = br.band(n, C, w, w)
    if not br.band_helps(n, C, *b2):
        return full(), "full", cells + n * C
    return dp(*b2), "second", cells + br.band_cells(n, C, *b2)


# ---- whole loci
def dp_for(posgap: bool):
    """The merge as prog_ref.progressive's dp argument (and as what in_compositions puts in prog_ref.align_profiles_np's place)."""
    def dp(X, Y, wx=None, wy=None):
        return align_profiles_np(X, Y, wx, wy, posgap=posgap)
    return dp


def progressive(seqs: Sequence[str], posgap: bool = False):
    """prog_ref.progressive with every merge with free end gaps: (rows, (leaves, rounds, fell back to star))."""
    return pr.progressive(seqs, dp=dp_for(posgap))


def progressive_rows(seqs: Sequence[str], posgap: bool = False) -> List[str]:
    return progressive(seqs, posgap)[0]


def progressive_fasta(records: Sequence[Tuple[str, str]], posgap: bool = False) -> str:
    """The file `from_msa --unaligned --progressive --free-end-gaps --msa-dir` writes for a locus."""
    rows = progressive_rows([s for _, s in records], posgap)
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))


@contextlib.contextmanager
def in_compositions(posgap: bool = False):
    """posgap_ref.in_compositions with this module's merge: inside, the reference compositions built on prog_ref merge with free end
    gaps."""
    from tests import retree_ref as rt
    from tests import weights_ref as wr
    old = pr.align_profiles_np, wr._cached, rt._cached
    pr.align_profiles_np, wr._cached, rt._cached = dp_for(posgap), wr._cached.__wrapped__, rt._cached.__wrapped__
    try:
        yield
    finally:
        pr.align_profiles_np, wr._cached, rt._cached = old
