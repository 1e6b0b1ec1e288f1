"""Test-side statement of the Retree spec of `from_msa --unaligned --progressive --retree` (make_prg_amd/from_msa/star_align.py,
"Retree") in plain Python on top of tests/prog_ref.py, tests/collapse_ref.py and tests/treerefine_ref.py, none of which
it changes: s', nw' and D' from row strings, the tree on D' (treerefine_ref.merge_order: collapse_ref's weighted UPGMA, keeping the
order of the merges), the rebuild (collapse_ref.build, which with every weight 1 is prog_ref.build) and the iteration with its stop
reasons.  Without classes every weight is 1.  Nothing is ever beyond a limit here: the limits are the device's."""
import functools
from typing import List, Sequence, Tuple

from tests import collapse_ref as cr
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import star_ref as sr
from tests import treerefine_ref as tf

SCALE = 1 << 16
MAX_REBUILDS = 4                               # RETREE_MAX


# ---- the distance
def valid_cells(row: str) -> int:
    """nw': the cells of a row that are A, C, G or T."""
    return sum(1 for ch in row if ch in "ACGT")


def identical_cells(x: str, y: str) -> int:
    """s': the columns in which both rows hold the same letter and that letter is A, C, G or T."""
    return sum(1 for p, q in zip(x, y) if p == q and p in "ACGT")


def identities(rows: Sequence[str]) -> Tuple[List[List[int]], List[int]]:
    """(s' as a full symmetric table over the rows with a zero diagonal, nw' per row)."""
    n = len(rows)
    s = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            s[a][b] = s[b][a] = identical_cells(rows[a], rows[b])
    return s, [valid_cells(r) for r in rows]


def distances(idx: Sequence[int], rows: Sequence[str]):
    """D' between a locus's leaves from its MSA, as D[a][b] by record index: row k is record idx[k]."""
    s, nw = identities(rows)
    D = {a: {} for a in idx}
    for x, a in enumerate(idx):
        for y, b in enumerate(idx):
            m = min(nw[x], nw[y])
            D[a][b] = 0 if a == b else SCALE if m == 0 else SCALE - (SCALE * s[x][y]) // m
    return D


def kmer_distances(seqs: Sequence[str], leaves: Sequence[int]):
    """Progressive's D between the leaves (prog_ref.distances is quadratic in what it is given), as D[a][b] by record index."""
    small = pr.distances([seqs[a] for a in leaves])[0]
    return {a: {b: small[i][j] for j, b in enumerate(leaves)} for i, a in enumerate(leaves)}


# ---- the iteration
def retree(seqs: Sequence[str], rebuilds: int, collapse: bool = False):
    """One locus's raw sequences through Progressive (collapse: Collapse's) and up to `rebuilds` iterations of the spec: (leaves
    in row order, one row per leaf, the merges of the tree that built them, weights per record, empty records, rounds of that tree,
    (iterations run, accepted, why it stopped, S before, S after))."""
    seqs = [sr.normalise(s) for s in seqs]
    if not any(seqs):
        raise ValueError("every sequence is empty")
    rep = cr.classes(seqs) if collapse else list(range(len(seqs)))
    w = cr.weights(rep)
    leaves = [a for a, s in enumerate(seqs) if s and rep[a] == a]
    empty = sum(1 for s in seqs if not s)
    merges, tree = tf.merge_order(kmer_distances(seqs, leaves), leaves, w)
    idx, rows, rounds, _ = cr.build(tree, seqs, w)
    s0 = s = tf.objective(rows, [w[a] for a in idx], empty)
    runs = accepted = 0
    why = None
    if len(leaves) >= 3:
        for _ in range(rebuilds):
            runs += 1
            merges2, tree2 = tf.merge_order(distances(idx, rows), leaves, w)
            if merges2 == merges:
                why = "same"
                break
            idx2, rows2, rounds2, _ = cr.build(tree2, seqs, w)
            s2 = tf.objective(rows2, [w[a] for a in idx2], empty)
            if s2 <= s:
                why = "refused"
                break
            idx, rows, merges, rounds, s, accepted = idx2, rows2, merges2, rounds2, s2, accepted + 1
    return idx, rows, merges, w, empty, rounds, (runs, accepted, why, s0, s)


@functools.lru_cache(maxsize=None)
def _cached(seqs: Tuple[str, ...], rebuilds: int, collapse: bool):
    return retree(seqs, rebuilds, collapse)


def progressive(seqs: Sequence[str], rebuilds: int, collapse: bool = False, refine_tree: int = 0, refine: int = 0):
    """(rows in input order, the retreeing tuple, the progression tuple, the tree_refinement tuple or None, the refinement tuple or
    None) of one locus's raw sequences: the iteration, then treerefine_ref's passes on the accepted MSA with the accepted tree,
    then refine_ref's rounds on the rows in input order.  rebuilds = 0: the progressive rows."""
    idx, rows, merges, w, empty, rounds, info = _cached(tuple(seqs), rebuilds, collapse)
    norm = [sr.normalise(s) for s in seqs]
    rep = cr.classes(norm) if collapse else list(range(len(norm)))
    tree_info = refine_info = None
    if refine_tree:
        idx, rows, tree_info = tf.refine_tree(idx, rows, merges, w, empty, refine_tree)
    at = dict(zip(idx, rows))
    out = [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(norm)]
    if refine:
        out, acc, trail = rr.refine_rows(out, refine)
        refine_info = (acc, trail[0], trail[-1])
    return out, info, (len(idx), rounds, False), tree_info, refine_info


def fasta(records: Sequence[Tuple[str, str]], rebuilds: int) -> str:
    """The file `from_msa --unaligned --progressive --retree N --msa-dir` writes for a locus."""
    rows = progressive([s for _, s in records], rebuilds)[0]
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))
