"""Test-side statement of "Position gaps" (make_prg_amd/from_msa/star_align.py) in plain Python on top of
tests/prog_ref.py: the opens Oc and Ox by occupancy, the profile-profile DP with them cell by cell (`align_profiles`) and by rows
in NumPy (`align_profiles_np`, also over weighted rows; the emulated tests pin it to the cell form), the banded DP cell by cell,
the bound U(w) with oy + ox in place of -1 408, w* by linear search and the two-pass rule, all by their definitions."""
import contextlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import align_ref as ar
from tests import band_ref as br
from tests import prog_ref as pr
from tests import progband_ref as pb

NEG, OPEN = pr.NEG, pr.OPEN
W0 = pb.W0


# ---- the opens
def opens(X: Sequence[str], Y: Sequence[str]) -> Tuple[List[int], List[int]]:
    """(Oc per column of Y, Ox per column of X), from the rows, with C's truncating division."""
    RX, RY = len(X), len(Y)
    Oc = [ar.tdiv(64 * -11 * (RY - sum(r[j] == "-" for r in Y)), RY) for j in range(len(Y[0]))]
    Ox = [ar.tdiv(64 * -11 * (RX - sum(r[i] == "-" for r in X)), RX) for i in range(len(X[0]))]
    return Oc, Ox


def _weighted_counts(rows, w):
    """prog_ref._counts with row r counting w[r] times (None: once)."""
    if w is None:
        return pr._counts(rows)
    w = np.asarray(w, np.int64)
    A = rows if isinstance(rows, np.ndarray) else pr_codes(rows)
    c = {x: ((A == q) * w[:, None]).sum(0).astype(np.int64) for q, x in enumerate("ACGT-")}
    R = int(w.sum())
    return c, R - sum(c.values()), R


def pr_codes(rows) -> np.ndarray:
    """Row strings as a matrix of cell codes (ACGT- = 0..4, everything else 5: only the five counts are taken)."""
    A = np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), -1)
    out = np.full(A.shape, 5, np.uint8)
    for q, x in enumerate("ACGT-"):
        out[A == ord(x)] = q
    return out


def tables(X, Y, wx=None, wy=None):
    """(P per base, Pamb, Dc, Oc of Y; the counts per base, of the ambiguity codes, R_X, Ic and Ox of X), per column; X and Y
    row strings or matrices of cell codes, wx and wy the rows' weights (None: 1)."""
    cy, _, RY = _weighted_counts(Y, wy)
    acgt = sum(cy[x] for x in "ACGT")
    P = {x: pr._tdv(64 * (20 * cy[x] - 9 * (acgt - cy[x]) - 10 * cy["-"]), RY) for x in "ACGT"}
    Pamb = pr._tdv(64 * -10 * cy["-"], RY)
    Dc = pr._tdv(64 * -10 * (RY - cy["-"]), RY)
    Oc = pr._tdv(64 * -11 * (RY - cy["-"]), RY)
    cx, ambx, RX = _weighted_counts(X, wx)
    Ic = pr._tdv(64 * -10 * (RX - cx["-"]), RX)
    Ox = pr._tdv(64 * -11 * (RX - cx["-"]), RX)
    return P, Pamb, Dc, Oc, cx, ambx, RX, Ic, Ox


# ---- the DP
def _walk(H, D, I, sc, Dc, Ic, n, C):
    """The walk back from (n, C) in state H: diagonal, then D, then I; extend before open."""
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
            st = "D" if D[i][j - 1] + Dc[j - 1] == D[i][j] else "H"
            j -= 1
        else:
            ops.append("I")
            st = "I" if I[i - 1][j] + Ic[i - 1] == I[i][j] else "H"
            i -= 1
    return "".join(reversed(ops))


def align_profiles_banded(X: Sequence[str], Y: Sequence[str], dlo: Optional[int] = None, dhi: Optional[int] = None) -> Tuple[str, int]:
    """(ops, score) cell by cell, by the spec's recurrence, over the cells with dlo <= j - i <= dhi (None: all of them); every
    other cell is NEG in all three states."""
    P, Dc, cols, Ic = pr.column_tables(X, Y)
    Oc, Ox = opens(X, Y)
    RX, n, C = len(X), len(cols), len(Dc)
    dlo, dhi = (-n, C) if dlo is None else br.clamp(n, C, dlo, dhi)
    inside = lambda i, j: dlo <= j - i <= dhi          # noqa: E731
    sc = lambda i, j: pr.column_score(cols[i], P[j], Dc[j], RX)   # noqa: E731
    H = [[NEG] * (C + 1) for _ in range(n + 1)]
    D = [[NEG] * (C + 1) for _ in range(n + 1)]
    I = [[NEG] * (C + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for j in range(1, C + 1):
        if inside(0, j):
            D[0][j] = max(D[0][j - 1] + Dc[j - 1], H[0][j - 1] + Oc[j - 1] + Dc[j - 1])
            H[0][j] = D[0][j]
    for i in range(1, n + 1):
        if inside(i, 0):
            I[i][0] = max(I[i - 1][0] + Ic[i - 1], H[i - 1][0] + Ox[i - 1] + Ic[i - 1])
            H[i][0] = I[i][0]
        for j in range(max(1, i + dlo), min(C, i + dhi) + 1):
            D[i][j] = max(D[i][j - 1] + Dc[j - 1], H[i][j - 1] + Oc[j - 1] + Dc[j - 1])
            I[i][j] = max(I[i - 1][j] + Ic[i - 1], H[i - 1][j] + Ox[i - 1] + Ic[i - 1])
            H[i][j] = max(H[i - 1][j - 1] + sc(i - 1, j - 1), D[i][j], I[i][j])
    # the boundary the spec states in closed form
    if dhi == C:
        assert all(H[0][J] == Oc[0] + sum(Dc[:J]) for J in range(1, C + 1))
    if dlo == -n:
        assert all(H[i][0] == Ox[0] + sum(Ic[:i]) for i in range(1, n + 1))
    return _walk(H, D, I, sc, Dc, Ic, n, C), H[n][C]


def align_profiles(X: Sequence[str], Y: Sequence[str]) -> Tuple[str, int]:
    return align_profiles_banded(X, Y)


def align_profiles_np(X, Y, wx=None, wy=None, band: Optional[Tuple[int, int]] = None) -> Tuple[str, int]:
    """align_profiles by rows (prog_ref.align_profiles_np's form): D of a row as a running maximum over H[i][k] + Oc[k] - S[k].
    X and Y: row strings, or R x W matrices of cell codes; wx, wy: the rows' weights; band: (dlo, dhi), the cells outside it FAR
    below NEG (progband_ref.align_profiles_banded_np's form), so that nothing derived from them ties with a real score."""
    P, Pamb, Dc, Oc, cx, ambx, RX, Ic, Ox = tables(X, Y, wx, wy)
    n, C = len(X[0]), len(Y[0])
    dlo, dhi = (-n, C) if band is None else br.clamp(n, C, *band)
    FAR = -(1 << 60)
    S = np.concatenate([[0], np.cumsum(Dc)])
    cols = np.arange(C + 1)
    H = np.full((n + 1, C + 1), FAR, np.int64)
    D = np.full((n + 1, C + 1), FAR, np.int64)
    I = np.full((n + 1, C + 1), FAR, np.int64)
    D[0, 1:] = np.where(cols[1:] <= dhi, int(Oc[0]) + S[1:], FAR)
    H[0] = D[0]
    H[0, 0] = 0
    sc = [None] * n
    for i in range(1, n + 1):
        ins, opn = int(Ic[i - 1]), int(Ox[i - 1])
        inside = (cols - i >= dlo) & (cols - i <= dhi)
        I[i] = np.where(inside, np.maximum(I[i - 1] + ins, H[i - 1] + opn + ins), FAR)
        sc[i - 1] = pr._tdv(sum(int(cx[x][i - 1]) * P[x] for x in "ACGT") + int(ambx[i - 1]) * Pamb + int(cx["-"][i - 1]) * Dc, RX)
        diag = np.full(C + 1, FAR, np.int64)
        diag[1:] = H[i - 1, :-1] + sc[i - 1]
        hp = np.where(inside, np.maximum(diag, I[i]), FAR)
        # (opening from a cell whose H is its D never beats extending that run: Oc <= 0)
        D[i, 1:] = np.where(inside[1:], S[1:] + np.maximum.accumulate(hp[:-1] + Oc - S[:-1]), FAR)
        H[i] = np.maximum(hp, D[i])
    return _walk(H, D, I, lambda i, j: sc[i][j], Dc, Ic, n, C), int(H[n, C])


# ---- the certificate
def bounds(X, Y) -> Tuple[int, List[int], List[int], int, int]:
    """progband_ref.bounds, then (oy, ox): the largest Oc and the largest Ox (0 for an X of no columns)."""
    SB, loss, ins = pb.bounds(X, Y)
    _, _, _, Oc, _, _, _, _, Ox = tables(X, Y)
    return SB, loss, ins, int(Oc.max()), int(Ox.max()) if len(Ox) else 0


def U(SB: int, loss: List[int], ins: List[int], oy: int, ox: int, n: int, C: int, w: int) -> int:
    """The most a path that leaves the band of half-width w can score: its two runs pay at most oy and ox."""
    delta = C - n
    return SB - sum(loss[:max(0, delta) + w + 1]) - sum(ins[:w + 1 - min(0, delta)]) + oy + ox


def closed(SB, loss, ins, oy, ox, n, C, dlo, dhi, S) -> Tuple[bool, bool]:
    """progband_ref.closed with oy + ox."""
    dlo, dhi = br.clamp(n, C, dlo, dhi)
    delta = C - n
    lower = dlo == -n or S > SB - sum(loss[:delta - dlo + 1]) - sum(ins[:1 - dlo]) + oy + ox
    upper = dhi == C or S > SB - sum(loss[:dhi + 1]) - sum(ins[:dhi + 1 - delta]) + oy + ox
    return lower, upper


def wstar(SB, loss, ins, oy, ox, n, C, S0) -> int:
    """The smallest w >= 0 with U(w) < S0, by linear search; min(n, C) if none is."""
    for w in range(min(n, C)):
        if U(SB, loss, ins, oy, ox, n, C, w) < S0:
            return w
    return min(n, C)


def align_profiles_banded_np(X, Y, dlo: int, dhi: int) -> Tuple[str, int]:
    return align_profiles_np(X, Y, band=(dlo, dhi))


def two_pass(X, Y, w0: int = W0, dp=align_profiles_banded_np, full=align_profiles_np):
    """progband_ref.two_pass with the new opens and the new U: ((ops, score), kind, cells computed)."""
    n, C = len(X[0]), len(Y[0])
    b = bounds(X, Y)
    b1 = br.band(n, C, w0, w0)
    if not br.band_helps(n, C, *b1):
        return full(X, Y), "full", n * C
    res = dp(X, Y, *b1)
    cells = br.band_cells(n, C, *b1)
    w = wstar(*b, n, C, res[1])
    if w <= w0:
        assert all(closed(*b, n, C, *b1, res[1]))
        return res, "first", cells
    b2 = br.band(n, C, w, w)
    if not br.band_helps(n, C, *b2):
        return full(X, Y), "full", cells + n * C
    res = dp(X, Y, *b2)
    assert all(closed(*b, n, C, *b2, res[1]))
    return res, "second", cells + br.band_cells(n, C, *b2)


# ---- whole loci
def progressive(seqs: Sequence[str]):
    """prog_ref.progressive with every merge by the new opens: (rows, (leaves, rounds, fell back to star))."""
    return pr.progressive(seqs, dp=align_profiles_np)


def progressive_rows(seqs: Sequence[str]) -> List[str]:
    return progressive(seqs)[0]


def progressive_fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --progressive --position-gaps --msa-dir` writes for a locus."""
    rows = progressive_rows([s for _, s in records])
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))


@contextlib.contextmanager
def in_compositions():
    """Inside: the reference compositions built on prog_ref (collapse_ref, weights_ref, retree_ref, treerefine_ref call
    prog_ref.align_profiles_np for every merge) merge with the new opens."""
    from tests import retree_ref as rt
    from tests import weights_ref as wr
    old = pr.align_profiles_np, wr._cached, rt._cached
    # (the two modules memoise their loci: inside, their uncached forms, so that neither side's results reach the other's)
    pr.align_profiles_np, wr._cached, rt._cached = align_profiles_np, wr._cached.__wrapped__, rt._cached.__wrapped__
    try:
        yield
    finally:
        pr.align_profiles_np, wr._cached, rt._cached = old
