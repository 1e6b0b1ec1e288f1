"""Test-side statement of "Progressive, band" (make_prg_amd/from_msa/star_align.py): the banded profile-profile DP cell by cell
(`align_profiles_banded`) and by rows in NumPy (`align_profiles_banded_np`, the emulated tests pin it to the cell form) on top of
tests/prog_ref.py's column tables and scores, the bounds, U(w), w* by linear search and the two-pass rule with its counters, all
by their definitions (sorted lists and sums), not by the histograms and the bisection the device uses."""
from typing import List, Sequence, Tuple

import numpy as np

from tests import band_ref as br
from tests import prog_ref as pr

NEG, OPEN = pr.NEG, pr.OPEN
W0 = 64                       # make_prg_amd.from_msa.star_align.PROG_BAND_W0


def align_profiles_banded(X: Sequence[str], Y: Sequence[str], dlo: int, dhi: int) -> Tuple[str, int]:
    """prog_ref.align_profiles over the cells with dlo <= j - i <= dhi: every other cell is NEG in all three states."""
    P, Dc, cols, Ic = pr.column_tables(X, Y)
    RX, n, C = len(X), len(cols), len(Dc)
    dlo, dhi = br.clamp(n, C, dlo, dhi)
    inside = lambda i, j: dlo <= j - i <= dhi          # noqa: E731
    sc = lambda i, j: pr.column_score(cols[i], P[j], Dc[j], RX)   # noqa: E731
    H = [[NEG] * (C + 1) for _ in range(n + 1)]
    D = [[NEG] * (C + 1) for _ in range(n + 1)]
    I = [[NEG] * (C + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for j in range(1, C + 1):
        if inside(0, j):
            D[0][j] = max(D[0][j - 1] + Dc[j - 1], H[0][j - 1] + OPEN + Dc[j - 1])
            H[0][j] = D[0][j]
    for i in range(1, n + 1):
        if inside(i, 0):
            I[i][0] = max(I[i - 1][0] + Ic[i - 1], H[i - 1][0] + OPEN + Ic[i - 1])
            H[i][0] = I[i][0]
        for j in range(max(1, i + dlo), min(C, i + dhi) + 1):
            D[i][j] = max(D[i][j - 1] + Dc[j - 1], H[i][j - 1] + OPEN + Dc[j - 1])
            I[i][j] = max(I[i - 1][j] + Ic[i - 1], H[i - 1][j] + OPEN + Ic[i - 1])
            H[i][j] = max(H[i - 1][j - 1] + sc(i - 1, j - 1), D[i][j], I[i][j])
    ops, i, j, state = [], n, C, "H"
    while i > 0 or j > 0:
        assert inside(i, j)
        if state == "H":
            if i > 0 and j > 0 and H[i - 1][j - 1] + sc(i - 1, j - 1) == H[i][j]:
                ops.append("M")
                i, j = i - 1, j - 1
            elif D[i][j] == H[i][j]:
                state = "D"
            else:
                state = "I"
        elif state == "D":
            ops.append("D")
            state = "D" if D[i][j - 1] + Dc[j - 1] == D[i][j] else "H"
            j -= 1
        else:
            ops.append("I")
            state = "I" if I[i - 1][j] + Ic[i - 1] == I[i][j] else "H"
            i -= 1
    return "".join(reversed(ops)), H[n][C]


def _tables_np(X, Y):
    cy, _, RY = pr._counts(Y)
    acgt = sum(cy[x] for x in "ACGT")
    P = {x: pr._tdv(64 * (20 * cy[x] - 9 * (acgt - cy[x]) - 10 * cy["-"]), RY) for x in "ACGT"}
    Pamb = pr._tdv(64 * -10 * cy["-"], RY)
    Dc = pr._tdv(64 * -10 * (RY - cy["-"]), RY)
    cx, ambx, RX = pr._counts(X)
    Ic = pr._tdv(64 * -10 * (RX - cx["-"]), RX)

    def srow(i):
        return pr._tdv(sum(int(cx[x][i]) * P[x] for x in "ACGT") + int(ambx[i]) * Pamb + int(cx["-"][i]) * Dc, RX)
    return P, Pamb, Dc, Ic, srow


def align_profiles_banded_np(X: Sequence[str], Y: Sequence[str], dlo: int, dhi: int) -> Tuple[str, int]:
    """align_profiles_banded by rows (band_ref.align_pair_banded_np's form: FAR outside the band, far below NEG, so that nothing
    derived from it ties with a real score; H inside, and D and I wherever they descend from a real cell, are the cell form's)."""
    _, _, Dc, Ic, srow = _tables_np(X, Y)
    n, C = len(X[0]), len(Y[0])
    dlo, dhi = br.clamp(n, C, dlo, dhi)
    FAR = -(1 << 60)
    S = np.concatenate([[0], np.cumsum(Dc)])
    cols = np.arange(C + 1)
    H = np.full((n + 1, C + 1), FAR, np.int64)
    D = np.full((n + 1, C + 1), FAR, np.int64)
    I = np.full((n + 1, C + 1), FAR, np.int64)
    D[0, 1:] = np.where(cols[1:] <= dhi, OPEN + S[1:], FAR)
    H[0] = D[0]
    H[0, 0] = 0
    sc = [None] * n
    for i in range(1, n + 1):
        ins = int(Ic[i - 1])
        inside = (cols - i >= dlo) & (cols - i <= dhi)
        I[i] = np.where(inside, np.maximum(I[i - 1] + ins, H[i - 1] + OPEN + ins), FAR)
        sc[i - 1] = srow(i - 1)
        diag = np.full(C + 1, FAR, np.int64)
        diag[1:] = H[i - 1, :-1] + sc[i - 1]
        hp = np.where(inside, np.maximum(diag, I[i]), FAR)
        run = np.maximum.accumulate(hp[:-1] - S[:-1])
        D[i, 1:] = np.where(inside[1:], S[1:] + OPEN + run, FAR)
        H[i] = np.maximum(hp, D[i])
    ops, i, j, st = [], n, C, "H"
    while i > 0 or j > 0:
        if st == "H":
            if i > 0 and j > 0 and H[i - 1, j - 1] + sc[i - 1][j - 1] == H[i, j]:
                ops.append("M")
                i, j = i - 1, j - 1
            elif D[i, j] == H[i, j]:
                st = "D"
            else:
                st = "I"
        elif st == "D":
            ops.append("D")
            st = "D" if D[i, j - 1] + Dc[j - 1] == D[i, j] else "H"
            j -= 1
        else:
            ops.append("I")
            st = "I" if I[i - 1, j] + Ic[i - 1] == I[i, j] else "H"
            i -= 1
    return "".join(reversed(ops)), int(H[n, C])


# ---- the certificate
def bounds(X: Sequence[str], Y: Sequence[str]) -> Tuple[int, List[int], List[int]]:
    """(SB, the loss_j in ascending order, the ins_i in ascending order)."""
    P, Pamb, Dc, Ic, _ = _tables_np(X, Y)
    B = np.maximum(np.maximum.reduce([P[x] for x in "ACGT"] + [Pamb]), Dc)
    return int(B.sum()), sorted((B - Dc).tolist()), sorted((-Ic).tolist())


def U(SB: int, loss: List[int], ins: List[int], n: int, C: int, w: int) -> int:
    """The most a path that leaves the band of half-width w (on either side) can score; list slices clamp k."""
    delta = C - n
    return SB - sum(loss[:max(0, delta) + w + 1]) - sum(ins[:w + 1 - min(0, delta)]) + 2 * OPEN


def closed(SB, loss, ins, n, C, dlo, dhi, S) -> Tuple[bool, bool]:
    """(the lower side, the upper side) of the (clamped) band, each by its own count of ops: a path that touches dlo - 1 has at
    least (C - n) - (dlo - 1) D ops and -(dlo - 1) I ops; one that touches dhi + 1 at least dhi + 1 and dhi + 1 - (C - n)."""
    dlo, dhi = br.clamp(n, C, dlo, dhi)
    delta = C - n
    lower = dlo == -n or S > SB - sum(loss[:delta - dlo + 1]) - sum(ins[:1 - dlo]) + 2 * OPEN
    upper = dhi == C or S > SB - sum(loss[:dhi + 1]) - sum(ins[:dhi + 1 - delta]) + 2 * OPEN
    return lower, upper


def wstar(SB, loss, ins, n, C, S0) -> int:
    """The smallest w >= 0 with U(w) < S0, by linear search; min(n, C), where both sides reach the matrix's edge, if none is."""
    for w in range(min(n, C)):
        if U(SB, loss, ins, n, C, w) < S0:
            return w
    return min(n, C)


def two_pass(X: Sequence[str], Y: Sequence[str], w0: int = W0, dp=align_profiles_banded_np, full=pr.align_profiles_np):
    """The spec's two-pass rule for one merge: ((ops, score), kind, cells computed); kind: "first" (certified in pass 1),
    "second" (a second pass ran) or "full" (sent to the full DP, before or after pass 1)."""
    n, C = len(X[0]), len(Y[0])
    SB, loss, ins = bounds(X, Y)
    b1 = br.band(n, C, w0, w0)
    if not br.band_helps(n, C, *b1):
        return full(X, Y), "full", n * C
    res = dp(X, Y, *b1)
    cells = br.band_cells(n, C, *b1)
    w = wstar(SB, loss, ins, n, C, res[1])
    if w <= w0:
        assert all(closed(SB, loss, ins, n, C, *b1, res[1]))
        return res, "first", cells
    b2 = br.band(n, C, w, w)
    if not br.band_helps(n, C, *b2):
        return full(X, Y), "full", cells + n * C
    res = dp(X, Y, *b2)
    assert all(closed(SB, loss, ins, n, C, *b2, res[1]))
    return res, "second", cells + br.band_cells(n, C, *b2)


def counters(kinds_cells, sizes) -> dict:
    """star_align's prog_band_* counters of a set of merges from two_pass's (kind, cells) and the (n, C) of each."""
    kinds = [k for k, _ in kinds_cells]
    return dict(prog_band_merges=len(kinds), prog_band_second_passes=kinds.count("second"), prog_band_full_merges=kinds.count("full"),
                prog_band_cells=sum(c for _, c in kinds_cells), prog_band_full_cells=sum(n * C for n, C in sizes))


def progressive(seqs: Sequence[str], w0: int = W0):
    """prog_ref.progressive with every merge through two_pass: (rows, info, [(kind, cells)], [(n, C)]) of the locus."""
    log, sizes = [], []

    def dp(X, Y):
        res, kind, cells = two_pass(X, Y, w0)
        log.append((kind, cells))
        sizes.append((len(X[0]), len(Y[0])))
        return res
    rows, info = pr.progressive(seqs, dp=dp)
    return rows, info, log, sizes
