"""Test-side statement of the Sequence weights spec of `from_msa --unaligned --progressive --seq-weights`
(make_prg_amd/from_msa/star_align.py, "Sequence weights") in plain Python on top of tests/prog_ref.py,
tests/collapse_ref.py, tests/treerefine_ref.py and tests/retree_ref.py, none of which it changes: the heights, the edges, the raw
weights and q in Python integers from a distance table and a merge list, and a weighted merge as prog_ref's unweighted DP on the
rows written q times each (as collapse_ref does for the multiplicities).  Without classes every multiplicity is 1."""
import functools
from typing import Dict, List, Optional, Sequence, Tuple

from tests import collapse_ref as cr
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import retree_ref as rt
from tests import star_ref as sr
from tests import treerefine_ref as tf

UNIT = 256


# ---- the weights
def heights(D, merges: Sequence[Tuple[int, int]], w: Dict[int, int]):
    """Per merge t: (H_t, the leaves below node t as a set, their multiplicity sum)."""
    members = {}
    out = []
    for u, v in merges:
        U, V = members.get(u, [u]), members.pop(v, [v])
        n = sum(w[a] * w[b] * D[a][b] for a in U for b in V)
        su, sv = sum(w[a] for a in U), sum(w[b] for b in V)
        out.append((n // (su * sv), set(U + V), su + sv))
        members[u] = U + V
    return out


def leaf_weights(D, leaves: Sequence[int], merges: Sequence[Tuple[int, int]], w: Optional[Sequence[int]] = None):
    """(H per merge, c per leaf, q per leaf; the last two as dicts by record index).  w: per RECORD its multiplicity.
    Stated from the leaf's side: for every node t above leaf a, the child c of t that holds a has the edge
    len(c) = max(H_t - H_c, 0), shared by the n_c multiplicities below c."""
    mult = {a: 1 if w is None else w[a] for a in leaves}
    nodes = heights(D, merges, mult)
    raw = {}
    for a in leaves:
        c, below, n = 0, 0, mult[a]                                # the child that holds a: its height, its multiplicity sum
        for h, under, size in nodes:                               # (in merge order: a's ancestors from the bottom up)
            if a in under:
                c += (UNIT * max(h - below, 0) * mult[a]) // n
                below, n = h, size
        raw[a] = c
    top = max(raw.values(), default=0)
    return [h for h, _, _ in nodes], raw, {a: 1 if top == 0 else 1 + ((UNIT - 1) * c) // top for a, c in raw.items()}


# ---- the weighted build
def build(tree, seqs: Sequence[str], w: Sequence[int], q: Dict[int, int]):
    """collapse_ref.build with the rows counting q times in a merge; Y and X by the multiplicities w, as there."""
    if isinstance(tree, int):
        return [tree], [seqs[tree]], 0
    ia, ra, da = build(tree[0], seqs, w, q)
    ib, rb, db = build(tree[1], seqs, w, q)
    if (sum(w[i] for i in ia), -min(ia)) >= (sum(w[i] for i in ib), -min(ib)):
        iy, Y, ix, X = ia, ra, ib, rb
    else:
        iy, Y, ix, X = ib, rb, ia, ra
    ops, _ = pr.align_profiles_np(cr.expanded(X, [q[i] for i in ix]), cr.expanded(Y, [q[i] for i in iy]))
    nx, ny = pr.merge_rows(X, Y, ops)
    return iy + ix, ny + nx, 1 + max(da, db)


def step(idx, rows, G, w, q):
    """treerefine_ref.step with the rows counting q times in the realignment; the sides by the multiplicities w, as there."""
    in_g = [a in G for a in idx]
    wg, wo = sum(w[a] for a, g in zip(idx, in_g) if g), sum(w[a] for a, g in zip(idx, in_g) if not g)
    g_is_y = wg > wo or (wg == wo and min(idx) in G)
    side = [int(g != g_is_y) for g in in_g]
    Y, X = tf.split(rows, side)
    iy, ix = [a for a, s in zip(idx, side) if s == 0], [a for a, s in zip(idx, side) if s == 1]
    ops, _ = pr.align_profiles_np(cr.expanded(X, [q[a] for a in ix]), cr.expanded(Y, [q[a] for a in iy]))
    nx, ny = pr.merge_rows(X, Y, ops)
    return iy + ix, ny + nx


def locus(seqs: Sequence[str], collapse: bool = False, retree: int = 0, refine_tree: int = 0):
    """One locus's raw sequences through the weighted Progressive: (leaves in row order, rows, q by leaf, multiplicities per
    record, representatives, empty records, the retreeing tuple or None, the tree_refinement tuple or None)."""
    seqs = [sr.normalise(s) for s in seqs]
    if not any(seqs):
        raise ValueError("every sequence is empty")
    rep = cr.classes(seqs) if collapse else list(range(len(seqs)))
    w = cr.weights(rep)
    leaves = [a for a, s in enumerate(seqs) if s and rep[a] == a]
    empty = sum(1 for s in seqs if not s)
    D = rt.kmer_distances(seqs, leaves)
    merges, tree = tf.merge_order(D, leaves, w)
    q = leaf_weights(D, leaves, merges, w)[2]
    idx, rows, _ = build(tree, seqs, w, q)
    wr = lambda ix: [w[a] for a in ix]
    re_info = tree_info = None
    if retree:
        s0 = s = tf.objective(rows, wr(idx), empty)
        runs = accepted = 0
        why = None
        if len(leaves) >= 3:
            for _ in range(retree):
                runs += 1
                D2 = rt.distances(idx, rows)
                merges2, tree2 = tf.merge_order(D2, leaves, w)
                if merges2 == merges:
                    why = "same"
                    break
                q2 = leaf_weights(D2, leaves, merges2, w)[2]
                idx2, rows2, _ = build(tree2, seqs, w, q2)
                s2 = tf.objective(rows2, wr(idx2), empty)
                if s2 <= s:
                    why = "refused"
                    break
                idx, rows, merges, q, s, accepted = idx2, rows2, merges2, q2, s2, accepted + 1
        re_info = (runs, accepted, why, s0, s)
    if refine_tree:
        s0 = s = tf.objective(rows, wr(idx), empty)
        tried = accepted = 0
        if tf.MIN_LEAVES <= len(idx) <= tf.MAX_LEAVES:
            todo = tf.steps(merges)
            for _ in range(refine_tree):
                moved = False
                for G in todo:
                    tried += 1
                    idx2, rows2 = step(idx, rows, G, w, q)
                    s2 = tf.objective(rows2, wr(idx2), empty)
                    if s2 > s:
                        idx, rows, s, moved, accepted = idx2, rows2, s2, True, accepted + 1
                if not moved:
                    break
        tree_info = (tried, accepted, 0, s0, s)
    return idx, rows, q, w, rep, empty, re_info, tree_info


@functools.lru_cache(maxsize=None)
def _cached(seqs: Tuple[str, ...], collapse: bool, retree: int, refine_tree: int):
    return locus(seqs, collapse, retree, refine_tree)


def progressive(seqs: Sequence[str], collapse: bool = False, retree: int = 0, refine_tree: int = 0, refine: int = 0):
    """(rows in input order, q by leaf, the retreeing tuple, the tree_refinement tuple, the refinement tuple) of one locus's raw
    sequences; refine: refine_ref's rounds afterwards, on the rows in input order, unweighted."""
    idx, rows, q, _, rep, _, re_info, tree_info = _cached(tuple(seqs), collapse, retree, refine_tree)
    norm = [sr.normalise(s) for s in seqs]
    at = dict(zip(idx, rows))
    out = [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(norm)]
    refine_info = None
    if refine:
        out, acc, trail = rr.refine_rows(out, refine)
        refine_info = (acc, trail[0], trail[-1])
    return out, q, re_info, tree_info, refine_info


def fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --progressive --seq-weights --msa-dir` writes for a locus."""
    rows = progressive([s for _, s in records])[0]
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))
