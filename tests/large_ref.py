"""Test-side statement of the Large loci spec of `from_msa --unaligned --progressive --collapse-identical --large-loci`
(make_prg_amd/from_msa/star_align.py, "Large loci") in plain Python on top of tests/collapse_ref.py, which it does not
change: the rule that counts leaves, then Collapse's classes, weighted UPGMA and merges as they are.  The distances are taken over
the representatives only (prog_ref.distances is quadratic in what it is given), which is what the spec's Collapse says too."""
from typing import List, Optional, Sequence, Tuple

from tests import collapse_ref as cr
from tests import prog_ref as pr
from tests import star_ref as sr

MAX_LEAVES = pr.MAX_LEAVES
MAX_RECORDS = 1 << 20


def progressive(seqs: Sequence[str], max_leaves: int = MAX_LEAVES, max_records: int = MAX_RECORDS
                ) -> Tuple[Optional[List[str]], Tuple[int, int, bool], int]:
    """(rows in input order, progression, merges) of one locus's raw (oriented) sequences.  A locus over a limit: rows None (the
    star MSA, which the tests take from the star pass itself) and (non-empty records, 0, True)."""
    seqs = [sr.normalise(s) for s in seqs]
    if not any(seqs):
        raise ValueError("every sequence is empty")
    rep = cr.classes(seqs)
    w = cr.weights(rep)
    leaves = [a for a, s in enumerate(seqs) if s and rep[a] == a]
    if len(leaves) > max_leaves or len(seqs) > max_records:
        return None, (sum(1 for s in seqs if s), 0, True), 0
    if len(leaves) == 1:
        rows = [seqs[leaves[0]]]
        idx, rounds, merges = leaves, 0, 0
    else:
        small = pr.distances([seqs[a] for a in leaves])[0]          # D between the representatives, put where upgma looks for it
        D = {a: {b: small[i][j] for j, b in enumerate(leaves)} for i, a in enumerate(leaves)}
        idx, rows, rounds, merges = cr.build(cr.upgma(D, leaves, w), seqs, w)
    at = {a: r for a, r in zip(idx, rows)}
    return [at[rep[a]] if s else "-" * len(rows[0]) for a, s in enumerate(seqs)], (len(leaves), rounds, False), merges


def progressive_fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --progressive --collapse-identical --large-loci --msa-dir` writes for a locus the rule builds."""
    rows = progressive([s for _, s in records])[0]
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))
