"""Test-side statement of the Progressive spec of `from_msa --unaligned --progressive` (make_prg_amd/from_msa/star_align.py, DESIGN.md
§3b) in plain Python on top of tests/align_ref.py, tests/star_ref.py and tests/refine_ref.py: the 6-mer distances, the exact UPGMA
tree with its tie rule, the profile-profile DP cell by cell (`align_profiles`) and by rows in NumPy (`align_profiles_np`, exact
integers, over row strings or matrices of cell codes; the emulated tests pin it to the cell form), the merge of a node's two
children and the rows in input order."""
import random
from typing import List, Sequence, Tuple

import numpy as np

from tests import align_ref as ar
from tests import star_ref as sr

NEG, OPEN = ar.NEG, ar.OPEN
SCALE = 1 << 16
MAX_LEAVES = 4096


# ---- distances and tree
def distances(seqs: Sequence[str]) -> Tuple[List[List[int]], List[List[int]], List[int]]:
    """(D, s, nw) over all records of a locus (normalised sequences): D[a][b] of the spec, s[a][b] the shared 6-mers, nw[a]."""
    cs = [sr.kmer_counts(s) for s in seqs]
    nw = [int(c.sum()) for c in cs]
    R = len(seqs)
    D = [[0] * R for _ in range(R)]
    S = [[0] * R for _ in range(R)]
    for a in range(R):
        for b in range(a + 1, R):
            s = int(np.minimum(cs[a], cs[b]).sum())
            m = min(nw[a], nw[b])
            S[a][b] = S[b][a] = s
            D[a][b] = D[b][a] = SCALE if m == 0 else SCALE - (SCALE * s) // m
    return D, S, nw


def upgma(D: Sequence[Sequence[int]], leaves: Sequence[int]):
    """The tree over the leaves (indices into D) as nested pairs (an int is a leaf): average linkage, fractions compared by
    cross-multiplication, ties to the smallest key(U), then the smallest key(V), key = the lowest member, key(U) < key(V)."""
    members = {i: [i] for i in leaves}
    tree = {i: i for i in leaves}
    while len(members) > 1:
        keys = sorted(members)
        best = None
        for x, u in enumerate(keys):
            for v in keys[x + 1:]:
                s = sum(D[a][b] for a in members[u] for b in members[v])
                w = len(members[u]) * len(members[v])
                if best is None or s * best[1] < best[0] * w:       # strictly smaller only: the first (u, v) in key order keeps a tie
                    best = (s, w, u, v)
        _, _, u, v = best
        members[u] += members.pop(v)
        tree[u] = (tree[u], tree.pop(v))
    return tree[min(tree)]


# ---- profile-profile DP
def column_tables(X: Sequence[str], Y: Sequence[str]):
    """(P, Dc of Y as align_ref.profile gives them; per X column its counts {A, C, G, T, amb, '-'}; Ic)."""
    P, Dc = ar.profile(Y)
    RX = len(X)
    cols = []
    for i in range(len(X[0])):
        col = [r[i] for r in X]
        c = {x: col.count(x) for x in "ACGT-"}
        c["amb"] = RX - sum(c.values())
        cols.append(c)
    Ic = [ar.tdiv(64 * -10 * (RX - c["-"]), RX) for c in cols]
    return P, Dc, cols, Ic


def column_score(c, Pj, Dcj, RX: int) -> int:
    return ar.tdiv(sum(c[x] * Pj[x] for x in "ACGT") + c["amb"] * Pj["N"] + c["-"] * Dcj, RX)


def align_profiles(X: Sequence[str], Y: Sequence[str]) -> Tuple[str, int]:
    """(ops, score) cell by cell: M X's column with Y's column, I X's column alone, D Y's column alone."""
    P, Dc, cols, Ic = column_tables(X, Y)
    RX, n, C = len(X), len(cols), len(Dc)
    sc = [[column_score(cols[i], P[j], Dc[j], RX) for j in range(C)] for i in range(n)]
    H = [[0] * (C + 1) for _ in range(n + 1)]
    D = [[NEG] * (C + 1) for _ in range(n + 1)]
    I = [[NEG] * (C + 1) for _ in range(n + 1)]
    for j in range(1, C + 1):
        D[0][j] = max(D[0][j - 1] + Dc[j - 1], H[0][j - 1] + OPEN + Dc[j - 1])
        H[0][j] = D[0][j]
    for i in range(1, n + 1):
        I[i][0] = max(I[i - 1][0] + Ic[i - 1], H[i - 1][0] + OPEN + Ic[i - 1])
        H[i][0] = I[i][0]
        for j in range(1, C + 1):
            D[i][j] = max(D[i][j - 1] + Dc[j - 1], H[i][j - 1] + OPEN + Dc[j - 1])
            I[i][j] = max(I[i - 1][j] + Ic[i - 1], H[i - 1][j] + OPEN + Ic[i - 1])
            H[i][j] = max(H[i - 1][j - 1] + sc[i - 1][j - 1], D[i][j], I[i][j])
    ops, i, j, state = [], n, C, "H"
    while i > 0 or j > 0:
        if state == "H":
            if i > 0 and j > 0 and H[i - 1][j - 1] + sc[i - 1][j - 1] == H[i][j]:
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


def _counts(rows):
    """Per column the counts of A C G T '-', of the ambiguity codes together, and R: of row strings, or of an R x W matrix of cell
    codes (uint8; tall profiles, whose rows nobody wants as Python strings)."""
    if isinstance(rows, np.ndarray):
        c = {x: (rows == q).sum(0).astype(np.int64) for q, x in enumerate("ACGT-")}
    else:
        A = np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), -1)
        c = {x: (A == ord(x)).sum(0).astype(np.int64) for x in "ACGT-"}
    return c, len(rows) - sum(c.values()), len(rows)


def _tdv(a, R):
    return np.sign(a) * (np.abs(a) // R)


def _column_tables(X, Y):
    """(P per base, Pamb, Dc of Y; the counts per base, of the ambiguity codes, R_X and Ic of X), all per column."""
    cy, _, RY = _counts(Y)
    acgt = sum(cy[x] for x in "ACGT")
    P = {x: _tdv(64 * (20 * cy[x] - 9 * (acgt - cy[x]) - 10 * cy["-"]), RY) for x in "ACGT"}
    Pamb = _tdv(64 * -10 * cy["-"], RY)
    Dc = _tdv(64 * -10 * (RY - cy["-"]), RY)
    cx, ambx, RX = _counts(X)
    return P, Pamb, Dc, cx, ambx, RX, _tdv(64 * -10 * (RX - cx["-"]), RX)


def numerators(X, Y) -> np.ndarray:
    """The W_X x W_Y numerators of the column scores, before the truncating division by R_X (int64)."""
    P, Pamb, Dc, cx, ambx, _, _ = _column_tables(X, Y)
    return sum(cx[x][:, None] * P[x][None] for x in "ACGT") + ambx[:, None] * Pamb[None] + cx["-"][:, None] * Dc[None]


def align_profiles_np(X: Sequence[str], Y: Sequence[str]) -> Tuple[str, int]:
    """align_profiles by rows: D of a row as a running maximum over the row's other values (as align_ref.align_pair_np).  X and Y:
    row strings, or R x W matrices of cell codes."""
    P, Pamb, Dc, cx, ambx, RX, Ic = _column_tables(X, Y)
    n, C = len(X[0]), len(Y[0])

    def srow(i):
        return _tdv(sum(int(cx[x][i]) * P[x] for x in "ACGT") + int(ambx[i]) * Pamb + int(cx["-"][i]) * Dc, RX)
    S = np.concatenate([[0], np.cumsum(Dc)])
    H = np.empty((n + 1, C + 1), np.int64)
    D = np.full((n + 1, C + 1), NEG, np.int64)
    I = np.full((n + 1, C + 1), NEG, np.int64)
    D[0, 1:] = OPEN + S[1:]
    H[0] = D[0]
    H[0, 0] = 0
    sc = [None] * n
    for i in range(1, n + 1):
        ins = int(Ic[i - 1])
        I[i] = np.maximum(I[i - 1] + ins, H[i - 1] + OPEN + ins)
        sc[i - 1] = srow(i - 1)
        diag = np.full(C + 1, NEG, np.int64)
        diag[1:] = H[i - 1, :-1] + sc[i - 1]
        hp = np.maximum(diag, I[i])
        run = np.maximum.accumulate(hp[:-1] - S[:-1])
        D[i, 1:] = S[1:] + OPEN + run
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


def merge_rows(X: Sequence[str], Y: Sequence[str], ops: str) -> Tuple[List[str], List[str]]:
    """(X's rows, Y's rows) over the merged columns, one per op."""
    ox, oy, i, j = [[] for _ in X], [[] for _ in Y], 0, 0
    for op in ops:
        for r, o in zip(X, ox):
            o.append(r[i] if op != "D" else "-")
        for r, o in zip(Y, oy):
            o.append(r[j] if op != "I" else "-")
        i += op != "D"
        j += op != "I"
    assert i == len(X[0]) and j == len(Y[0])
    return ["".join(o) for o in ox], ["".join(o) for o in oy]


# ---- the whole locus
def build(tree, seqs: Sequence[str], dp=align_profiles_np):
    """(leaf indices in row order, rows, rounds) of a tree node: Y (more rows; on equal rows the lower key) first, then X."""
    if isinstance(tree, int):
        return [tree], [seqs[tree]], 0
    ia, ra, da = build(tree[0], seqs, dp)
    ib, rb, db = build(tree[1], seqs, dp)
    if (len(ia), -min(ia)) >= (len(ib), -min(ib)):
        iy, Y, ix, X = ia, ra, ib, rb
    else:
        iy, Y, ix, X = ib, rb, ia, ra
    ops, _ = dp(X, Y)
    nx, ny = merge_rows(X, Y, ops)
    return iy + ix, ny + nx, 1 + max(da, db)


def progressive_rows(seqs: Sequence[str], max_leaves: int = MAX_LEAVES, dp=align_profiles_np) -> List[str]:
    """The MSA's rows in input order of one locus's raw sequences; a locus with more than max_leaves non-empty records: star's."""
    return progressive(seqs, max_leaves, dp)[0]


def progressive(seqs: Sequence[str], max_leaves: int = MAX_LEAVES, dp=align_profiles_np) -> Tuple[List[str], Tuple[int, int, bool]]:
    """(rows, (leaves, rounds, fell back to star))."""
    seqs = [sr.normalise(s) for s in seqs]
    leaves = [i for i, s in enumerate(seqs) if s]
    if not leaves:
        raise ValueError("every sequence is empty")
    if len(leaves) > max_leaves:
        return sr.star_rows(seqs)[1], (len(leaves), 0, True)
    tree = upgma(distances(seqs)[0], leaves)
    idx, rows, rounds = build(tree, seqs, dp)
    out = ["-" * len(rows[0])] * len(seqs)
    for i, r in zip(idx, rows):
        out[i] = r
    return out, (len(leaves), rounds, False)


def progressive_fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --progressive --msa-dir` writes for a locus."""
    rows = progressive_rows([s for _, s in records])
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))


# ---- loci
def clade_locus(seed: int, n: int = 12, clades: int = 2, L=(150, 300), deep=(0.10, 0.05), shallow=(0.04, 0.02)) -> List[str]:
    """n sequences in `clades` sub-families: a random root of 150-300 nt -> one ancestor per clade by star_ref.mutate(0.10, 0.05)
    -> the members by mutate(0.04, 0.02) of the ancestors in turn, shuffled."""
    rng = random.Random(seed)
    root = "".join(rng.choice("ACGT") for _ in range(rng.randint(*L)))
    anc = [sr.mutate(rng, root, *deep) for _ in range(clades)]
    seqs = [sr.mutate(rng, anc[k % clades], *shallow) for k in range(n)]
    rng.shuffle(seqs)
    return seqs


def table_loci() -> List[List[str]]:
    """The 18 loci of the issue's table: six diverged, six of two clades (12 rows), six of three clades (18 rows)."""
    from tests import refine_ref as rr
    return ([rr.diverged_locus(s) for s in range(6)] + [clade_locus(s) for s in range(6)] +
            [clade_locus(s, 18, clades=3) for s in range(6)])


def random_profiles(rng: random.Random, R: int, W: int, gap: float = 0.2, amb: float = 0.05) -> List[str]:
    """R rows of W cells: '-' with probability gap, an ambiguity code with probability amb, else ACGT; no all-gap column
    and (R > 1) columns that share a letter often enough for the DP to have real choices."""
    base = [rng.choice("ACGT") for _ in range(W)]
    rows = []
    for _ in range(R):
        row = []
        for j in range(W):
            u = rng.random()
            row.append("-" if u < gap else rng.choice("RYKMSWN") if u < gap + amb else base[j] if u < 0.9 else rng.choice("ACGT"))
        rows.append(row)
    for j in range(W):
        if all(r[j] == "-" for r in rows):
            rows[rng.randrange(R)][j] = base[j]
    return ["".join(r) for r in rows]
