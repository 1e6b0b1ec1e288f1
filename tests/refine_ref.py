"""Test-side statement of the Refinement spec of `from_msa --unaligned --refine` (make_prg_amd/from_msa/star_align.py, DESIGN.md
§3b) in plain Python: the objective S, one leave-one-out round (tests/align_ref.py's DP against the MSA without the row, the merge
by align_ref.merge over the W columns, all-gap columns removed), and the acceptance rule, on top of tests/star_ref.py's star MSA."""
import random
from typing import List, Sequence, Tuple

from tests import align_ref as ar
from tests import star_ref as sr


def drop_empty_columns(rows: Sequence[str]) -> List[str]:
    keep = [j for j in range(len(rows[0])) if any(r[j] != "-" for r in rows)]
    return ["".join(r[j] for j in keep) for r in rows]


def runs(rows: Sequence[str]) -> int:
    """Maximal runs of '-' over all rows, end runs included."""
    return sum(1 for r in rows for j, ch in enumerate(r) if ch == "-" and (j == 0 or r[j - 1] != "-"))


def objective(rows: Sequence[str]) -> int:
    """S of an MSA (taken after its all-gap columns are removed)."""
    rows = drop_empty_columns(rows)
    R = len(rows)
    sp = 0
    for j in range(len(rows[0])):
        col = [r[j] for r in rows]
        c = [col.count(x) for x in "ACGT"]
        g = col.count("-")
        sp += 20 * sum(v * (v - 1) // 2 for v in c) - 9 * sum(c[x] * c[y] for x in range(4) for y in range(x + 1, 4)) - 10 * g * (R - g)
    return 2 * sp - 11 * (R - 1) * runs(rows)


def objective_by_pairs(rows: Sequence[str]) -> int:
    """The same S from sigma over every pair of rows, cell by cell (what the closed form abbreviates)."""
    rows = drop_empty_columns(rows)
    R = len(rows)
    sp = sum(ar.sigma(rows[a][j], rows[b][j]) for a in range(R) for b in range(a + 1, R) for j in range(len(rows[0])))
    return 2 * sp - 11 * (R - 1) * runs(rows)


def refinable(rows: Sequence[str]) -> bool:
    return sum(1 for r in rows if r.replace("-", "")) >= 3


def one_round(rows: Sequence[str]) -> List[str]:
    """A' of the spec's Round for an MSA with 3 or more non-empty rows."""
    R, W = len(rows), len(rows[0])
    seqs = [r.replace("-", "") for r in rows]
    filled = [a for a in range(R) if seqs[a]]
    ops = [ar.align_pair_np([rows[b] for b in range(R) if b != a], seqs[a])[0] for a in filled]
    merged = ar.merge(["-" * W], [seqs[a] for a in filled], ops)[1:]          # (the all-gap leaf row only carries the W columns)
    width = len(merged[0])
    out = ["-" * width] * R
    for a, r in zip(filled, merged):
        out[a] = r
    return drop_empty_columns(out)


def refine_rows(rows: Sequence[str], n_rounds: int) -> Tuple[List[str], int, List[int]]:
    """(the refined rows, rounds accepted, [S of the input, S after every accepted round]) by the acceptance rule."""
    rows = list(rows)
    trail = [objective(rows)]
    if not refinable(rows):
        return rows, 0, trail
    for _ in range(n_rounds):
        new = one_round(rows)
        s = objective(new)
        if s <= trail[-1]:
            break
        rows = new
        trail.append(s)
    return rows, len(trail) - 1, trail


def refined_star_rows(seqs: Sequence[str], n_rounds: int) -> Tuple[List[str], int, List[int]]:
    """refine_rows on the star MSA (tests/star_ref.py) of one locus's raw sequences."""
    return refine_rows(sr.star_rows(seqs)[1], n_rounds)


DIVERGED_SEEDS = (0, 1, 2, 3, 4, 5)


def diverged_locus(seed: int, n: int = 12) -> List[str]:
    """A locus of n sequences: star_ref.mutate(sub=0.06, indel=0.03) of one random root of 150-300 nt."""
    rng = random.Random(seed)
    root = "".join(rng.choice("ACGT") for _ in range(rng.randint(150, 300)))
    return [sr.mutate(rng, root, 0.06, 0.03) for _ in range(n)]


def special_loci() -> List[List[str]]:
    """Loci with empty records and ambiguity codes that are refined (3 or more non-empty rows), and ones that are not."""
    return [
        ["ACGTACGTTGACCA", "", "ACGTTCGTTGACA", "ACGACGTTGGACCA", ""],
        ["", "ACGTRYKMSWNACGTAC", "ACGTNNNNNACGTAC", "ACGTACGTACGTAC", "ACGTACGNACGTAC"],
        ["AAAAAAAA", "CAAAAAAAAC", "GGAAAAAAAAG", "TAAAAAAAAT", "AAAAAAAA"],
        ["ACGTTTGCA", "ACGTGCA", "ACGTTGCAA", "CGTTTGCA"],
        ["ACGTACGT", "", "ACGTTCGT"],                                      # two non-empty rows: never refined
        ["NNNN", "ACGT", "RYKM", "AC"],
    ]
