"""Test-side statement of the Pair distances spec of `from_msa --unaligned --progressive --pair-distances`
(make_prg_amd/from_msa/star_align.py, "Pair distances") in plain Python on top of tests/align_ref.py (the pair DP),
tests/prog_ref.py, tests/collapse_ref.py and tests/treerefine_ref.py, none of which it changes: score, s'', nw'' and D'' from
sequences, the tree on D'' (treerefine_ref.merge_order: collapse_ref's weighted UPGMA, keeping the order of the merges) and the
build up that tree (collapse_ref.build, which with every weight 1 is prog_ref.build).  Nothing is ever beyond the DP's limit here."""
import functools
import random
from typing import List, Optional, Sequence, Tuple

from tests import align_ref as ar
from tests import collapse_ref as cr
from tests import prog_ref as pr
from tests import star_ref as sr
from tests import treerefine_ref as tf

SCALE = 1 << 16
MAX_LEAVES = 512                               # PAIR_DIST_MAX_LEAVES
MIN_LEAVES = 3
UNIT = 64                                      # the DP's scores are in 1/64 row
MATCH = 20                                     # nw'' = 20 acgt: 1 280 / 64 per equal ACGT pair


# ---- the distance
def acgt(s: str) -> int:
    """The cells of a sequence that are A, C, G or T."""
    return sum(1 for ch in s if ch in "ACGT")


@functools.lru_cache(maxsize=None)
def score(a: str, b: str) -> int:
    """The score of profile_align's DP of sequence a against sequence b as a 1-row leaf."""
    return ar.align_pair_np([b], a)[1]


def shared(a: str, b: str) -> int:
    """s''."""
    return max(score(a, b), 0) // UNIT


def tables(seqs: Sequence[str]) -> Tuple[List[List[int]], List[int]]:
    """(s'' as a full symmetric table over the records with a zero diagonal, nw'' per record) of normalised sequences; a pair with
    an empty record is not run: its entry is 0."""
    n = len(seqs)
    s = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            if seqs[a] and seqs[b]:
                s[a][b] = s[b][a] = shared(seqs[a], seqs[b])
    return s, [MATCH * acgt(x) for x in seqs]


def distance(s: int, nw_a: int, nw_b: int) -> int:
    m = min(nw_a, nw_b)
    return SCALE if m == 0 else SCALE - (SCALE * s) // m


def distances(seqs: Sequence[str], leaves: Sequence[int]):
    """D'' between the leaves, as D[a][b] by record index."""
    return {a: {b: 0 if a == b else distance(shared(seqs[min(a, b)], seqs[max(a, b)]), MATCH * acgt(seqs[a]), MATCH * acgt(seqs[b]))
                for b in leaves} for a in leaves}


def kmer_distances(seqs: Sequence[str], leaves: Sequence[int]):
    """Progressive's D between the leaves, as D[a][b] by record index."""
    small = pr.distances([seqs[a] for a in leaves])[0]
    return {a: {b: small[i][j] for j, b in enumerate(leaves)} for i, a in enumerate(leaves)}


# ---- the whole locus
def how(n_leaves: int, cap: int = MAX_LEAVES) -> Optional[str]:
    return None if n_leaves < MIN_LEAVES else "cap" if n_leaves > cap else "pairs"


def locus(seqs: Sequence[str], collapse: bool = False, cap: int = MAX_LEAVES, pair_distances: bool = True):
    """One locus's raw sequences through Progressive with the tree from D'' (from D without pair_distances, above the cap or below
    3 leaves): (leaves in row order, one row per leaf, the merges, the nested tree, weights per record, representatives, empty
    records, rounds, the distances the tree was built on, (leaves, pairs run, how))."""
    seqs = [sr.normalise(s) for s in seqs]
    if not any(seqs):
        raise ValueError("every sequence is empty")
    rep = cr.classes(seqs) if collapse else list(range(len(seqs)))
    w = cr.weights(rep)
    leaves = [a for a, s in enumerate(seqs) if s and rep[a] == a]
    h = how(len(leaves), cap) if pair_distances else None
    D = distances(seqs, leaves) if h == "pairs" else kmer_distances(seqs, leaves)
    merges, tree = tf.merge_order(D, leaves, w)
    idx, rows, rounds, _ = cr.build(tree, seqs, w)
    pairs = len(leaves) * (len(leaves) - 1) // 2 if h == "pairs" else 0
    return idx, rows, merges, tree, w, rep, sum(1 for s in seqs if not s), rounds, D, (len(leaves), pairs, h)


@functools.lru_cache(maxsize=None)
def _cached(seqs: Tuple[str, ...], collapse: bool, cap: int, pair_distances: bool):
    return locus(seqs, collapse, cap, pair_distances)


def progressive(seqs: Sequence[str], collapse: bool = False, cap: int = MAX_LEAVES, pair_distances: bool = True):
    """(rows in input order, the pair_distancing tuple, the progression tuple) of one locus's raw sequences."""
    idx, rows, _, _, _, rep, _, rounds, _, info = _cached(tuple(seqs), collapse, cap, pair_distances)
    norm = [sr.normalise(s) for s in seqs]
    at = dict(zip(idx, rows))
    return [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(norm)], info, (len(idx), rounds, False)


def composed(seqs: Sequence[str], collapse: bool = False, seq_weights: bool = False, retree: int = 0, refine_tree: int = 0, refine: int = 0):
    """The flag with the stages behind it, each stated by its own reference on what the stage before left: (rows in input order, the
    retreeing tuple or None, the tree_refinement tuple or None, the refinement tuple or None).  seq_weights: q from D'' (weights_ref);
    retree: retree_ref's iteration from the pair-distance tree, D' replacing D''; refine_tree: treerefine_ref's passes on the accepted
    tree; refine: refine_ref's rounds on the rows in input order.  seq_weights goes with none of the later stages here."""
    from tests import refine_ref as rr
    from tests import retree_ref as rt
    from tests import weights_ref as wr
    idx, rows, merges, tree, w, rep, empty, _, D, _ = _cached(tuple(seqs), collapse, MAX_LEAVES, True)
    norm = [sr.normalise(s) for s in seqs]
    leaves = sorted(idx)
    re_info = tree_info = refine_info = None
    if seq_weights:
        assert not (retree or refine_tree)
        idx, rows, _ = wr.build(tree, norm, w, wr.leaf_weights(D, leaves, merges, w)[2])
    if retree:
        s0 = s = tf.objective(rows, [w[a] for a in idx], empty)
        runs = accepted = 0
        why = None
        if len(leaves) >= MIN_LEAVES:
            for _ in range(retree):
                runs += 1
                merges2, tree2 = tf.merge_order(rt.distances(idx, rows), leaves, w)
                if merges2 == merges:
                    why = "same"
                    break
                idx2, rows2, _, _ = cr.build(tree2, norm, w)
                s2 = tf.objective(rows2, [w[a] for a in idx2], empty)
                if s2 <= s:
                    why = "refused"
                    break
                idx, rows, merges, s, accepted = idx2, rows2, merges2, s2, accepted + 1
        re_info = (runs, accepted, why, s0, s)
    if refine_tree:
        idx, rows, tree_info = tf.refine_tree(idx, rows, merges, w, empty, refine_tree)
    at = dict(zip(idx, rows))
    out = [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(norm)]
    if refine:
        out, acc, trail = rr.refine_rows(out, refine)
        refine_info = (acc, trail[0], trail[-1])
    return out, re_info, tree_info, refine_info


def objective(seqs: Sequence[str], **kw) -> int:
    """S of the locus's output MSA."""
    idx, rows, _, _, w, _, empty, _, _, _ = _cached(tuple(seqs), kw.get("collapse", False), kw.get("cap", MAX_LEAVES), kw.get("pair_distances", True))
    return tf.objective(rows, [w[a] for a in idx], empty)


def root_split(seqs: Sequence[str], pair_distances: bool = True):
    """The two sets of leaves under the root's children."""
    tree = _cached(tuple(seqs), False, MAX_LEAVES, pair_distances)[3]

    def under(t):
        return {t} if isinstance(t, int) else under(t[0]) | under(t[1])
    return under(tree[0]), under(tree[1])


def fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --progressive --pair-distances --msa-dir` writes for a locus."""
    rows = progressive([s for _, s in records])[0]
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))


# ---- loci
SATURATED_SEED = 1
STEP = {"A": "C", "C": "G", "G": "T", "T": "A"}


def saturated_locus(seed: int = SATURATED_SEED, L: int = 120) -> List[str]:
    """Two random roots of L nt, each with three copies: copy k has every fifth base from position k (k = 0, 1, 2) substituted
    A -> C -> G -> T -> A; the records interleaved, so family 1 is {0, 2, 4} and family 2 is {1, 3, 5}.  Two copies of a family
    differ at two bases in five and share no 6-mer window: the 6-mer distances saturate."""
    rng = random.Random(seed)
    roots = ["".join(rng.choice("ACGT") for _ in range(L)) for _ in range(2)]
    copies = [["".join(STEP[ch] if i % 5 == k else ch for i, ch in enumerate(root)) for k in range(3)] for root in roots]
    return [copies[f][k] for k in range(3) for f in range(2)]


FAMILIES = ({0, 2, 4}, {1, 3, 5})


def random_pairs(seed: int, n: int = 300):
    """Pairs of sequences of 0 < length <= 90, related or not, a third of them with ambiguity codes, every tenth pair with a side
    that has no ACGT at all."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        a = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 90)))
        b = sr.mutate(rng, a, 0.15, 0.08) if k % 2 else "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 90)))
        b = b or "A"
        if k % 3 == 0:
            a = "".join(rng.choice("RYKMSWN") if rng.random() < 0.15 else ch for ch in a)
            b = "".join(rng.choice("RYKMSWN") if rng.random() < 0.15 else ch for ch in b)
        if k % 10 == 9:
            b = "".join(rng.choice("RYKMSWN") for _ in b)
        out.append((a, b))
    return out
