"""Test-side statement of "Free end distances" (make_prg_amd/from_msa/star_align.py) in plain Python on top of
tests/freepairs_ref.py (the pair DP with free ends, its counted bound and its two passes), tests/pairdist_ref.py (s'', nw'', D'',
the tree and the build, none of which it changes) and tests/prog_ref.py: the overlap score of two sequences, the tables and D''
from it, the locus built on that tree, the stages behind it, and each fragment's distance to its nearest full-length record.
Every function takes free (False: the charged score of "Pair distances", which the tests pin to pairdist_ref's)."""
import contextlib
import functools
from typing import List, Sequence, Tuple

from tests import collapse_ref as cr
from tests import endgap_ref as eg
from tests import freepairs_ref as fp
from tests import pairdist_ref as pd
from tests import star_ref as sr
from tests import treerefine_ref as tf

SCALE, MATCH, UNIT, MAX_LEAVES = pd.SCALE, pd.MATCH, pd.UNIT, pd.MAX_LEAVES


# ---- the distance
@functools.lru_cache(maxsize=None)
def score(a: str, b: str, free: bool = True) -> int:
    """The score of "Free end pairs"' DP of sequence a against sequence b as a one-row leaf; free=False: profile_align's."""
    return fp.align_pair_np([b], a)[1] if free else pd.score(a, b)


def shared(a: str, b: str, free: bool = True) -> int:
    """s''."""
    return max(score(a, b, free), 0) // UNIT


def tables(seqs: Sequence[str], free: bool = True) -> Tuple[List[List[int]], List[int]]:
    """pairdist_ref.tables with the overlap score: (s'' as a full symmetric table, nw'' per record)."""
    n = len(seqs)
    s = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            if seqs[a] and seqs[b]:
                s[a][b] = s[b][a] = shared(seqs[a], seqs[b], free)
    return s, [MATCH * pd.acgt(x) for x in seqs]


def distances(seqs: Sequence[str], leaves: Sequence[int], free: bool = True):
    """D'' between the leaves, as D[a][b] by record index."""
    return {a: {b: 0 if a == b else pd.distance(shared(seqs[min(a, b)], seqs[max(a, b)], free), MATCH * pd.acgt(seqs[a]), MATCH * pd.acgt(seqs[b]))
                for b in leaves} for a in leaves}


def two_pass(a: str, b: str, w0: int):
    """freepairs_ref.two_pass of sequence a against b as a one-row leaf: ((ops, score), second pass run, sent to the full DP, cells)."""
    return fp.two_pass([b], a, w0)


# ---- the whole locus
def _merges(free_end_gaps: bool):
    """Inside, the builds of the references merge with free end gaps (endgap_ref.in_compositions), or as they are."""
    return eg.in_compositions() if free_end_gaps else contextlib.nullcontext()


@functools.lru_cache(maxsize=None)
def _locus(seqs: Tuple[str, ...], collapse: bool, cap: int, free: bool, free_end_gaps: bool):
    seqs = [sr.normalise(s) for s in seqs]
    if not any(seqs):
        raise ValueError("every sequence is empty")
    rep = cr.classes(seqs) if collapse else list(range(len(seqs)))
    w = cr.weights(rep)
    leaves = [a for a, s in enumerate(seqs) if s and rep[a] == a]
    h = pd.how(len(leaves), cap)
    D = distances(seqs, leaves, free) if h == "pairs" else pd.kmer_distances(seqs, leaves)
    merges, tree = tf.merge_order(D, leaves, w)
    with _merges(free_end_gaps):
        idx, rows, rounds, _ = cr.build(tree, seqs, w)
    pairs = len(leaves) * (len(leaves) - 1) // 2 if h == "pairs" else 0
    return idx, rows, merges, tree, w, rep, sum(1 for s in seqs if not s), rounds, D, (len(leaves), pairs, h)


def locus(seqs: Sequence[str], collapse: bool = False, cap: int = MAX_LEAVES, free: bool = True, free_end_gaps: bool = False):
    """pairdist_ref.locus with the tree from the overlap scores' D'' (free_end_gaps: every merge of the build as endgap_ref's)."""
    return _locus(tuple(seqs), collapse, cap, free, free_end_gaps)


def merges(seqs: Sequence[str], free: bool = True):
    """The UPGMA merge list of the locus."""
    return locus(seqs, free=free)[2]


def progressive(seqs: Sequence[str], collapse: bool = False, cap: int = MAX_LEAVES, free: bool = True, free_end_gaps: bool = False):
    """(rows in input order, the pair_distancing tuple, the progression tuple) of one locus's raw sequences."""
    idx, rows, _, _, _, rep, _, rounds, _, info = locus(seqs, collapse, cap, free, free_end_gaps)
    norm = [sr.normalise(s) for s in seqs]
    at = dict(zip(idx, rows))
    return [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(norm)], info, (len(idx), rounds, False)


def composed(seqs: Sequence[str], collapse: bool = False, seq_weights: bool = False, retree: int = 0, refine_tree: int = 0, refine: int = 0,
             free_end_gaps: bool = False, free_end_pairs: bool = False, free: bool = True):
    """pairdist_ref.composed on the overlap scores' tree: (rows in input order, the retreeing tuple or None, the tree_refinement tuple
    or None, the refinement tuple or None).  free_end_gaps: every merge of every stage as endgap_ref's; free_end_pairs: refine's
    realignments as freepairs_ref's."""
    from tests import refine_ref as rr
    from tests import retree_ref as rt
    from tests import weights_ref as wr
    idx, rows, mg, tree, w, rep, empty, _, D, _ = locus(seqs, collapse, MAX_LEAVES, free, free_end_gaps)
    norm = [sr.normalise(s) for s in seqs]
    leaves = sorted(idx)
    re_info = tree_info = refine_info = None
    with _merges(free_end_gaps):
        if seq_weights:
            assert not (retree or refine_tree)
            idx, rows, _ = wr.build(tree, norm, w, wr.leaf_weights(D, leaves, mg, w)[2])
        if retree:
            s0 = s = tf.objective(rows, [w[a] for a in idx], empty)
            runs = accepted = 0
            why = None
            if len(leaves) >= pd.MIN_LEAVES:
                for _ in range(retree):
                    runs += 1
                    mg2, tree2 = tf.merge_order(rt.distances(idx, rows), leaves, w)
                    if mg2 == mg:
                        why = "same"
                        break
                    idx2, rows2, _, _ = cr.build(tree2, norm, w)
                    s2 = tf.objective(rows2, [w[a] for a in idx2], empty)
                    if s2 <= s:
                        why = "refused"
                        break
                    idx, rows, mg, s, accepted = idx2, rows2, mg2, s2, accepted + 1
            re_info = (runs, accepted, why, s0, s)
        if refine_tree:
            idx, rows, tree_info = tf.refine_tree(idx, rows, mg, w, empty, refine_tree)
    at = dict(zip(idx, rows))
    out = [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(norm)]
    if refine:
        out, acc, trail = (fp if free_end_pairs else rr).refine_rows(out, refine)
        refine_info = (acc, trail[0], trail[-1])
    return out, re_info, tree_info, refine_info


def fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --progressive --pair-distances --free-end-distances --msa-dir` writes for a locus."""
    rows = progressive([s for _, s in records])[0]
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))


# ---- the finding
def nearest_full(seqs: Sequence[str], free: bool, short: int = 240):
    """Per record shorter than `short` its D'' to its nearest record of `short` or more, in record order; and the median D'' between
    two such records (of an even count the mean of the middle two, rounded down)."""
    full = [a for a, s in enumerate(seqs) if len(s) >= short]
    D = distances(seqs, range(len(seqs)), free)
    near = [min(D[a][b] for b in full) for a, s in enumerate(seqs) if len(s) < short]
    between = sorted(D[a][b] for i, a in enumerate(full) for b in full[i + 1:])
    return near, (between[(len(between) - 1) // 2] + between[len(between) // 2]) // 2
