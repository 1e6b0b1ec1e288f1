"""Test-side statement of the banded pair DP and of its certificate (the spec: make_prg_amd/update/profile_align.py, "Band"):
plain Python, cell by cell, on top of tests/align_ref.py's profile, scores and tie order; `align_pair_banded_np` is the same by
rows in NumPy (align_ref.align_pair_np with everything outside the band masked) for the large pairs; the emulated tests pin it to
the cell form.  The certificate, the two-pass rule and the cell counts are stated by their definitions (sums and linear searches),
not by the closed forms the host uses."""
from typing import List, Sequence, Tuple

import numpy as np

from tests.align_ref import INS, NEG, OPEN, MATCH, MISMATCH, VS_GAP, profile

W0 = 64                       # make_prg_amd.update.profile_align.BAND_W0


def band(n: int, C: int, w_minus: int, w_plus: int) -> Tuple[int, int]:
    """(dlo, dhi) of the half-widths, clamped to the matrix's diagonals [-n, C]."""
    delta = C - n
    return max(min(0, delta) - w_minus, -n), min(max(0, delta) + w_plus, C)


def clamp(n: int, C: int, dlo: int, dhi: int) -> Tuple[int, int]:
    assert dlo <= min(0, C - n) and dhi >= max(0, C - n), "the band must hold (0, 0) and (n, C)"
    return max(dlo, -n), min(dhi, C)


def align_pair_banded(rows: Sequence[str], seq: str, dlo: int, dhi: int) -> Tuple[str, int]:
    """align_ref.align_pair over the cells with dlo <= j - i <= dhi: every other cell is NEG in all three states."""
    seq = seq.replace("-", "").upper()
    P, Dc = profile([r.upper() for r in rows])
    n, C = len(seq), len(Dc)
    dlo, dhi = clamp(n, C, dlo, dhi)
    inside = lambda i, j: dlo <= j - i <= dhi          # noqa: E731
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
            I[i][0] = max(I[i - 1][0] + INS, H[i - 1][0] + OPEN + INS)
            H[i][0] = I[i][0]
        for j in range(1, C + 1):
            if inside(i, j):
                D[i][j] = max(D[i][j - 1] + Dc[j - 1], H[i][j - 1] + OPEN + Dc[j - 1])
                I[i][j] = max(I[i - 1][j] + INS, H[i - 1][j] + OPEN + INS)
                H[i][j] = max(H[i - 1][j - 1] + P[j - 1][seq[i - 1]], D[i][j], I[i][j])
    ops, i, j, state = [], n, C, "H"
    while i > 0 or j > 0:
        assert inside(i, j)
        if state == "H":
            if i > 0 and j > 0 and H[i - 1][j - 1] + P[j - 1][seq[i - 1]] == H[i][j]:
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
            state = "I" if I[i - 1][j] + INS == I[i][j] else "H"
            i -= 1
    return "".join(reversed(ops)), H[n][C]


def _profile_np(rows: Sequence[str]):
    A = np.frombuffer("".join(r.upper() for r in rows).encode(), np.uint8).reshape(len(rows), -1)
    R = A.shape[0]
    cnt = {x: (A == ord(x)).sum(0).astype(np.int64) for x in "ACGT-"}
    acgt = cnt["A"] + cnt["C"] + cnt["G"] + cnt["T"]

    def tdiv_v(a):
        return np.sign(a) * (np.abs(a) // R)
    Pv = {x: tdiv_v(64 * (MATCH * cnt[x] + MISMATCH * (acgt - cnt[x]) + VS_GAP * cnt["-"])) for x in "ACGT"}
    return Pv, tdiv_v(64 * VS_GAP * cnt["-"]), tdiv_v(64 * VS_GAP * (R - cnt["-"]))


def align_pair_banded_np(rows: Sequence[str], seq: str, dlo: int, dhi: int) -> Tuple[str, int]:
    """align_pair_banded by rows.  Outside the band everything is FAR (far below NEG, so that nothing derived from it can tie with
    a real score); inside, H, and D and I wherever they descend from a real cell, are the cell form's values: those are the only
    ones the maxima and the traceback ever select."""
    seq = seq.replace("-", "").upper()
    Pv, amb, Dc = _profile_np(rows)
    n, C = len(seq), len(Dc)
    dlo, dhi = clamp(n, C, dlo, dhi)
    FAR = -(1 << 60)
    S = np.concatenate([[0], np.cumsum(Dc)])
    cols = np.arange(C + 1)
    H = np.full((n + 1, C + 1), FAR, np.int64)
    D = np.full((n + 1, C + 1), FAR, np.int64)
    I = np.full((n + 1, C + 1), FAR, np.int64)
    in0 = cols <= dhi
    D[0, 1:] = np.where(in0[1:], OPEN + S[1:], FAR)
    H[0] = D[0]
    H[0, 0] = 0
    for i in range(1, n + 1):
        inside = (cols - i >= dlo) & (cols - i <= dhi)
        I[i] = np.where(inside, np.maximum(I[i - 1] + INS, H[i - 1] + OPEN + INS), FAR)
        diag = np.full(C + 1, FAR, np.int64)
        diag[1:] = H[i - 1, :-1] + Pv.get(seq[i - 1], amb)
        hp = np.where(inside, np.maximum(diag, I[i]), FAR)          # H without D (column 0: H[i][0] = I[i][0])
        run = np.maximum.accumulate(hp[:-1] - S[:-1])
        D[i, 1:] = np.where(inside[1:], S[1:] + OPEN + run, FAR)
        H[i] = np.maximum(hp, D[i])
    ops, i, j, state = [], n, C, "H"
    Pj = lambda j, x: int(Pv[x][j]) if x in Pv else int(amb[j])   # noqa: E731
    while i > 0 or j > 0:
        if state == "H":
            if i > 0 and j > 0 and H[i - 1, j - 1] + Pj(j - 1, seq[i - 1]) == H[i, j]:
                ops.append("M")
                i, j = i - 1, j - 1
            elif D[i, j] == H[i, j]:
                state = "D"
            else:
                state = "I"
        elif state == "D":
            ops.append("D")
            state = "D" if D[i, j - 1] + Dc[j - 1] == D[i, j] else "H"
            j -= 1
        else:
            ops.append("I")
            state = "I" if I[i - 1, j] + INS == I[i, j] else "H"
            i -= 1
    return "".join(reversed(ops)), int(H[n, C])


# ---- the certificate
def bounds(rows: Sequence[str]) -> Tuple[int, List[int]]:
    """(SB, the loss_j in ascending order) of a leaf: B_j = max(max_x P[j][x], Dc[j]), loss_j = B_j - Dc[j]."""
    Pv, amb, Dc = _profile_np(rows)
    B = np.maximum(np.maximum.reduce([Pv[x] for x in "ACGT"] + [amb]), Dc)
    return int(B.sum()), sorted((B - Dc).tolist())


def ub_plus(SB: int, loss: List[int], n: int, C: int, d: int, sorted_sum: bool = False) -> int:
    """The most a path that touches diagonal d > max(0, C - n) can score: >= d deletions, >= d - (C - n) insertions, a run of each."""
    assert d > max(0, C - n)
    lost = sum(loss[:d]) if sorted_sum else d * loss[0]
    return SB - lost + INS * (d - (C - n)) + 2 * OPEN


def ub_minus(SB: int, loss: List[int], n: int, C: int, d: int, sorted_sum: bool = False) -> int:
    """... that touches diagonal d < min(0, C - n): >= -d insertions, >= (C - n) - d deletions."""
    assert d < min(0, C - n)
    k = (C - n) - d
    lost = sum(loss[:k]) if sorted_sum else k * loss[0]
    return SB - lost + INS * (-d) + 2 * OPEN


def closed(SB, loss, n, C, dlo, dhi, S, sorted_sum=False) -> Tuple[bool, bool]:
    """(the lower side, the upper side): no path that leaves the (clamped) band there can reach S."""
    dlo, dhi = clamp(n, C, dlo, dhi)
    return (dlo == -n or S > ub_minus(SB, loss, n, C, dlo - 1, sorted_sum),
            dhi == C or S > ub_plus(SB, loss, n, C, dhi + 1, sorted_sum))


def certified(rows, seq, dlo, dhi, S, sorted_sum=False) -> bool:
    seq = seq.replace("-", "").upper()
    SB, loss = bounds(rows)
    return all(closed(SB, loss, len(seq), len(rows[0]), dlo, dhi, S, sorted_sum))


def certified_widths(SB, loss, n, C, S0) -> Tuple[int, int]:
    """(w*-, w*+): per side the smallest half-width whose band is closed against S0, by linear search."""
    w_minus = w_plus = 0
    while not closed(SB, loss, n, C, *band(n, C, w_minus, 0), S0)[0]:
        w_minus += 1
    while not closed(SB, loss, n, C, *band(n, C, 0, w_plus), S0)[1]:
        w_plus += 1
    return w_minus, w_plus


# ---- sizes
def full_words(n: int, C: int) -> int:
    return -(-2 * (C + 1) // 64) * 64 + -(-n // 64) * -(-(C + 63) // 8) * 64


def band_words(n: int, C: int, dlo: int, dhi: int) -> int:
    W = dhi - dlo + 1
    return -(-2 * W // 64) * 64 + -(-n // 64) * -(-(min(C, W + 63) + 63) // 8) * 64


def band_helps(n: int, C: int, dlo: int, dhi: int) -> bool:
    """Else the pair goes to the full DP: the band needs less workspace than the full matrix, in total and in its traceback (whose
    rows are min(C, W + 63) + 63 steps long against C + 63)."""
    return band_words(n, C, dlo, dhi) < full_words(n, C) and dhi - dlo + 1 + 63 < C


def band_cells(n: int, C: int, dlo: int, dhi: int) -> int:
    return sum(max(0, min(C, i + dhi) - max(1, i + dlo) + 1) for i in range(1, n + 1))


def two_pass(rows: Sequence[str], seq: str, w0: int = W0, dp=align_pair_banded_np, full=None):
    """The spec's two-pass rule for one pair: ((ops, score), second pass run, sent to the full DP, cells computed)."""
    from tests.align_ref import align_pair_np
    full = full or align_pair_np
    seq = seq.replace("-", "").upper()
    n, C = len(seq), len(rows[0])
    SB, loss = bounds(rows)
    b1 = band(n, C, w0, w0)
    if not band_helps(n, C, *b1):
        return full(rows, seq), False, True, n * C
    res = dp(rows, seq, *b1)
    cells = band_cells(n, C, *b1)
    w_minus, w_plus = certified_widths(SB, loss, n, C, res[1])
    if w_minus <= w0 and w_plus <= w0:
        return res, False, False, cells
    b2 = band(n, C, w_minus, w_plus)
    if not band_helps(n, C, *b2):
        return full(rows, seq), False, True, cells + n * C
    res = dp(rows, seq, *b2)
    assert all(closed(SB, loss, n, C, *b2, res[1]))
    return res, True, False, cells + band_cells(n, C, *b2)
