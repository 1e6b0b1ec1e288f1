"""Test-side statement of the Tree refinement spec of `from_msa --unaligned --progressive --refine-tree`
(make_prg_amd/from_msa/star_align.py, "Tree refinement") in plain Python on top of tests/prog_ref.py,
tests/collapse_ref.py and tests/refine_ref.py, none of which it changes: the merges in the order UPGMA made them, the step list, the
split of an MSA into two sub-alignments, one step (prog_ref's DP on the two sides' rows written w times, as collapse_ref does), the
weighted objective and the passes.  Without classes every weight is 1."""
from typing import List, Optional, Sequence, Tuple

from tests import collapse_ref as cr
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import star_ref as sr

MAX_LEAVES = 512                               # TREE_REFINE_MAX_LEAVES
MIN_LEAVES = 4


# ---- the tree's merges and the steps
def merge_order(D: Sequence[Sequence[int]], leaves: Sequence[int], w: Optional[Sequence[int]] = None):
    """(the merges (key(U), key(V)) in the order UPGMA makes them, the nested tree): collapse_ref.upgma's loop (prog_ref.upgma's
    with every weight 1), keeping the order."""
    w = [1] * (max(leaves) + 1) if w is None else w
    members = {i: [i] for i in leaves}
    tree = {i: i for i in leaves}
    merges = []
    while len(members) > 1:
        keys = sorted(members)
        best = None
        for x, u in enumerate(keys):
            for v in keys[x + 1:]:
                s = sum(w[a] * w[b] * D[a][b] for a in members[u] for b in members[v])
                n = sum(w[a] for a in members[u]) * sum(w[b] for b in members[v])
                if best is None or s * best[1] < best[0] * n:
                    best = (s, n, u, v)
        _, _, u, v = best
        merges.append((u, v))
        members[u] += members.pop(v)
        tree[u] = (tree[u], tree.pop(v))
    return merges, tree[min(tree)]


def node_leaves(merges: Sequence[Tuple[int, int]]) -> Tuple[List[List[int]], List[Tuple[int, int]]]:
    """(L_t per merge t: the leaves under node t, sorted; per merge its two children as node numbers, -1 - a for leaf a)."""
    at, under, kids = {}, [], []
    for t, (u, v) in enumerate(merges):
        a, b = at.get(u, -1 - u), at.get(v, -1 - v)
        kids.append((a, b))
        under.append(sorted((under[a] if a >= 0 else [u]) + (under[b] if b >= 0 else [v])))
        at[u] = t
    return under, kids


def steps(merges: Sequence[Tuple[int, int]]) -> List[List[int]]:
    """The spec's Steps: G = L_t of the nodes t = 0 .. m - 3, ascending, that leave two leaves or more outside; of two inner
    children of the root (the same split) the one with the smaller t is left out."""
    m = len(merges) + 1
    under, kids = node_leaves(merges)
    skip = min(kids[-1]) if m >= 3 and min(kids[-1]) >= 0 else -1
    return [under[t] for t in range(m - 2) if m - len(under[t]) >= 2 and t != skip]


# ---- the objective
def objective(rows: Sequence[str], w: Optional[Sequence[int]] = None, empty: int = 0) -> int:
    """The spec's Objective: Refinement's S with row r counted w_r times and `empty` all-gap rows more; no column may be all gaps."""
    w = [1] * len(rows) if w is None else w
    R = sum(w) + empty
    sp = 0
    for j in range(len(rows[0])):
        c = {x: 0 for x in "ACGT-"}
        for r, n in zip(rows, w):
            if r[j] in c:
                c[r[j]] += n
        v = [c[x] for x in "ACGT"]
        g = c["-"] + empty
        sp += 20 * sum(a * (a - 1) // 2 for a in v) - 9 * sum(v[x] * v[y] for x in range(4) for y in range(x + 1, 4)) - 10 * g * (R - g)
    runs = sum(n * rr.runs([r]) for r, n in zip(rows, w)) + empty
    return 2 * sp - 11 * (R - 1) * runs


# ---- a step
def split(rows: Sequence[str], side: Sequence[int]) -> Tuple[List[str], List[str]]:
    """(the rows with side 0, the rows with side 1), each over the columns in which one of its rows is not '-'; order kept."""
    out = []
    for s in (0, 1):
        part = [r for r, q in zip(rows, side) if q == s]
        keep = [j for j in range(len(rows[0])) if any(r[j] != "-" for r in part)]
        out.append(["".join(r[j] for j in keep) for r in part])
    return out[0], out[1]


def step(idx: Sequence[int], rows: Sequence[str], G: Sequence[int], w: Sequence[int]) -> Tuple[List[int], List[str]]:
    """The spec's step on the MSA `rows` of the leaves `idx` (row order): (leaves in the new row order: Y's, then X's; A')."""
    in_g = [a in G for a in idx]
    wg, wo = sum(w[a] for a, q in zip(idx, in_g) if q), sum(w[a] for a, q in zip(idx, in_g) if not q)
    g_is_y = wg > wo or (wg == wo and min(idx) in G)
    side = [int(q != g_is_y) for q in in_g]                         # 0: Y, 1: X
    Y, X = split(rows, side)
    iy, ix = [a for a, s in zip(idx, side) if s == 0], [a for a, s in zip(idx, side) if s == 1]
    ops, _ = pr.align_profiles_np(cr.expanded(X, [w[a] for a in ix]), cr.expanded(Y, [w[a] for a in iy]))
    nx, ny = pr.merge_rows(X, Y, ops)
    return iy + ix, ny + nx


def refine_tree(idx: Sequence[int], rows: Sequence[str], merges: Sequence[Tuple[int, int]], w: Sequence[int], empty: int, passes: int,
                max_leaves: int = MAX_LEAVES):
    """The spec's passes on a locus's root MSA: (leaves in row order, rows, (steps tried, accepted, skipped, S before, S after)).
    Nothing is ever skipped here: the limits are the device's."""
    wr = lambda ix: [w[a] for a in ix]
    s0 = s = objective(rows, wr(idx), empty)
    tried = accepted = 0
    if MIN_LEAVES <= len(idx) <= max_leaves:
        todo = steps(merges)
        for _ in range(passes):
            moved = False
            for G in todo:
                tried += 1
                idx2, rows2 = step(idx, rows, G, w)
                s2 = objective(rows2, wr(idx2), empty)
                if s2 > s:
                    idx, rows, s, moved, accepted = idx2, rows2, s2, True, accepted + 1
            if not moved:
                break
    return list(idx), list(rows), (tried, accepted, 0, s0, s)


# ---- the whole locus
def progressive(seqs: Sequence[str], passes: int, collapse: bool = False, max_leaves: int = MAX_LEAVES):
    """(rows in input order, the tree_refinement tuple) of one locus's raw sequences: prog_ref's (collapse: collapse_ref's)
    progressive MSA, then the passes.  passes = 0: the progressive rows."""
    seqs = [sr.normalise(s) for s in seqs]
    if not any(seqs):
        raise ValueError("every sequence is empty")
    rep = cr.classes(seqs) if collapse else list(range(len(seqs)))
    w = cr.weights(rep)
    leaves = [a for a, s in enumerate(seqs) if s and rep[a] == a]
    merges, tree = merge_order(pr.distances(seqs)[0], leaves, w)
    idx, rows, _, _ = cr.build(tree, seqs, w)
    empty = sum(1 for s in seqs if not s)
    idx, rows, info = refine_tree(idx, rows, merges, w, empty, passes, max_leaves)
    at = dict(zip(idx, rows))
    return [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(seqs)], info


def fasta(records: Sequence[Tuple[str, str]], passes: int) -> str:
    """The file `from_msa --unaligned --progressive --refine-tree N --msa-dir` writes for a locus."""
    rows = progressive([s for _, s in records], passes)[0]
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))
