"""Test-side statement of the Collapse spec of `from_msa --unaligned --collapse-identical` (make_prg_amd/from_msa/star_align.py,
"Collapse") in plain Python on top of tests/prog_ref.py and tests/star_ref.py, neither of which it changes: the
classes by string equality, the weighted UPGMA in Python integers, and a node's merge by prog_ref's unweighted DP on the rows
written w times each, so what stands for the weights is the unweighted code the progressive tests pin."""
from typing import List, Sequence, Tuple

from tests import prog_ref as pr
from tests import star_ref as sr


def classes(seqs: Sequence[str]) -> List[int]:
    """rep per record of normalised sequences: the smallest index of an equal sequence; an empty record is its own."""
    first, rep = {}, []
    for a, s in enumerate(seqs):
        rep.append(first.setdefault(s, a) if s else a)
    return rep


def weights(rep: Sequence[int]) -> List[int]:
    """The size of the class at every representative, 0 elsewhere."""
    w = [0] * len(rep)
    for r in rep:
        w[r] += 1
    return w


def upgma(D: Sequence[Sequence[int]], leaves: Sequence[int], w: Sequence[int]):
    """prog_ref.upgma with leaf a counting w[a] times: dist(U, V) = sum w_a w_b D[a][b] / (|U| |V|), |U| the weight sum."""
    members = {i: [i] for i in leaves}
    tree = {i: i for i in leaves}
    while len(members) > 1:
        keys = sorted(members)
        best = None
        for x, u in enumerate(keys):
            for v in keys[x + 1:]:
                s = sum(w[a] * w[b] * D[a][b] for a in members[u] for b in members[v])
                n = sum(w[a] for a in members[u]) * sum(w[b] for b in members[v])
                if best is None or s * best[1] < best[0] * n:       # strictly smaller only: the first (u, v) in key order keeps a tie
                    best = (s, n, u, v)
        _, _, u, v = best
        members[u] += members.pop(v)
        tree[u] = (tree[u], tree.pop(v))
    return tree[min(tree)]


def expanded(rows: Sequence[str], ws: Sequence[int]) -> List[str]:
    return [r for r, n in zip(rows, ws) for _ in range(n)]


def build(tree, seqs: Sequence[str], w: Sequence[int]):
    """(representatives in row order, one row per class, rounds, merges) of a tree node: Y (the larger weight sum; on equal sums
    the lower key) first, then X; the ops from prog_ref's DP on both sides' rows written w times."""
    if isinstance(tree, int):
        return [tree], [seqs[tree]], 0, 0
    ia, ra, da, ma = build(tree[0], seqs, w)
    ib, rb, db, mb = build(tree[1], seqs, w)
    if (sum(w[i] for i in ia), -min(ia)) >= (sum(w[i] for i in ib), -min(ib)):
        iy, Y, ix, X = ia, ra, ib, rb
    else:
        iy, Y, ix, X = ib, rb, ia, ra
    ops, _ = pr.align_profiles_np(expanded(X, [w[i] for i in ix]), expanded(Y, [w[i] for i in iy]))
    nx, ny = pr.merge_rows(X, Y, ops)
    return iy + ix, ny + nx, 1 + max(da, db), ma + mb + 1


def progressive(seqs: Sequence[str], max_leaves: int = pr.MAX_LEAVES) -> Tuple[List[str], Tuple[int, int, bool], int]:
    """(rows in input order, (classes of non-empty records, rounds, fell back to star), merges) of one locus's raw sequences."""
    seqs = [sr.normalise(s) for s in seqs]
    if not any(seqs):
        raise ValueError("every sequence is empty")
    n_records = sum(1 for s in seqs if s)
    if n_records > max_leaves:                                      # (by RECORDS, not classes)
        return sr.star_rows(seqs)[1], (n_records, 0, True), 0
    rep = classes(seqs)
    w = weights(rep)
    leaves = [a for a, s in enumerate(seqs) if s and rep[a] == a]
    idx, rows, rounds, merges = build(upgma(pr.distances(seqs)[0], leaves, w), seqs, w)
    at = {a: r for a, r in zip(idx, rows)}
    return [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(seqs)], (len(leaves), rounds, False), merges


def progressive_fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --progressive --collapse-identical --msa-dir` writes for a locus."""
    rows = progressive([s for _, s in records])[0]
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))
