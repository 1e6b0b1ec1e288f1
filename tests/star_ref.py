"""Test-side statement of the centre-star spec of `from_msa --unaligned` (make_prg_amd/from_msa/star_align.py) in
plain Python / NumPy: the centre by its k-mer score, the pairs by tests/align_ref.py's DP (the centre as a 1-row leaf), the merge
by align_ref.merge with the rows put back in input order."""
import random
from typing import List, Sequence, Tuple

import numpy as np

from tests import align_ref as ar

K = 6
ALLOWED = set("ACGT-RYKMSWN")


def normalise(seq: str) -> str:
    s = seq.upper().replace("-", "")
    bad = set(s) - ALLOWED
    if bad:
        raise ValueError(f"character {sorted(bad)[0]!r} outside ACGT-RYKMSWN")
    return s


def kmer_counts(s: str) -> np.ndarray:
    """The 4 096 counts of s's 6-mers over ACGT (windows with any other letter skipped)."""
    c = np.zeros(4 ** K, np.int64)
    if len(s) < K:
        return c
    lut = np.full(256, 4, np.int64)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    v = lut[np.frombuffer(s.encode(), np.uint8)]
    win = np.lib.stride_tricks.sliding_window_view(v, K)
    ok = (win < 4).all(1)
    k = (win[ok] * (4 ** np.arange(K - 1, -1, -1))).sum(1)
    np.add.at(c, k, 1)
    return c


def scores(seqs: Sequence[str]) -> List[int]:
    cs = [kmer_counts(s) for s in seqs]
    T = sum(cs) if cs else np.zeros(4 ** K, np.int64)
    return [int(c @ T - c @ c) for c in cs]


def centre(seqs: Sequence[str]) -> int:
    """The smallest index of a non-empty sequence that maximises score; -1 if every sequence is empty."""
    sc = scores(seqs)
    best = -1
    for a, s in enumerate(seqs):
        if s and (best < 0 or sc[a] > sc[best]):
            best = a
    return best


def star_rows(seqs: Sequence[str]) -> Tuple[int, List[str]]:
    """(centre, the MSA's rows in input order) of one locus's sequences (raw: upper-cased and ungapped here)."""
    seqs = [normalise(s) for s in seqs]
    c = centre(seqs)
    if c < 0:
        raise ValueError("every sequence is empty")
    others = [a for a in range(len(seqs)) if a != c]
    C = len(seqs[c])
    ops = [ar.align_pair_np([seqs[c]], seqs[a])[0] if seqs[a] else "D" * C for a in others]
    merged = ar.merge([seqs[c]], [seqs[a] for a in others], ops)
    rows = [None] * len(seqs)
    rows[c] = merged[0]
    for a, r in zip(others, merged[1:]):
        rows[a] = r
    return c, rows


def star_fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --msa-dir` writes for a locus."""
    _, rows = star_rows([s for _, s in records])
    return "".join(f">{t}\n{r}\n" for (t, _), r in zip(records, rows))


def mutate(rng: random.Random, s: str, sub=0.05, indel=0.02) -> str:
    out = []
    for ch in s:
        u = rng.random()
        if u < indel / 2:
            continue
        out.append(rng.choice("ACGT") if u < indel / 2 + sub else ch)
        if u > 1 - indel / 2:
            out.append("".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4))))
    return "".join(out)


def edge_loci() -> List[List[str]]:
    """The spec's edge cases, one locus each."""
    return [
        ["ACGTACGTTGCA"],                                              # one record
        ["ACGTACGTAC", "", "ACGTTCGTAC"],                              # an empty sequence
        ["", "ACGTACGTAC", "ACGTACGTAC"],                              # an empty FIRST record
        ["ACG", "ACGT", "AC", "ACGTA"],                                # all shorter than 6 nt: every score 0
        ["ACGTRYKMSWNACGT", "ACGTNNNNNACGTAC", "NNNNNN", "ACGTACGTACGT"],   # RYKMSWN and N
        ["acgt-acgt-ttga", "ACGTACG--TTGA", "a-c-g-t-a"],              # lower case and stray '-'
        ["ACGTAC", "TTTTTT", "ACGTAC", "TTTTTT"],                      # exact ties in score: the smallest index wins
        ["AAAAAAAA", "CAAAAAAAAC", "GGAAAAAAAAG", "TAAAAAAAAT", "AAAAAAAA"],   # insertions at both ends and at one boundary
        ["ACGTTGCAACGT", "ACGTTGCAACGT", "ACGTAGCAACGT"],              # identical sequences, one substitution
    ]


def random_loci(seed: int, n: int = 40) -> List[List[str]]:
    rng = random.Random(seed)
    loci = []
    for _ in range(n):
        base = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 150)))
        m = rng.randint(1, 9)
        seqs = [mutate(rng, base, rng.choice([0.0, 0.03, 0.1]), rng.choice([0.0, 0.02, 0.08])) for _ in range(m)]
        if rng.random() < 0.2:
            seqs[rng.randrange(m)] = "".join(rng.choice("ACGTN") for _ in range(rng.randint(0, 40)))
        if all(not s for s in seqs):
            seqs[0] = "A"
        loci.append(seqs)
    return loci


def synthetic_loci(seeds, config: str = "C") -> List[Tuple[List[str], List[str]]]:
    """config-shaped synthetic loci (utils/synthetic.py): (true alignment rows, the rows with their gaps removed)."""
    from make_prg_amd.utils.synthetic import config_shape, synth_rows
    out = []
    for seed in seeds:
        rows = [r.decode() for r in synth_rows(seed, *config_shape(config, seed))]
        out.append((rows, [r.replace("-", "") for r in rows]))
    return out


def pair_recovery(true_rows: Sequence[str], star: Sequence[str], c: int) -> Tuple[int, int]:
    """(recovered, total): the true alignment's aligned residue pairs of every row against the centre row (residue i of row a
    and residue j of the centre in one column), and how many of them the star alignment also puts in one column."""
    def pairs(rows, a):
        ia = ic = 0
        got = set()
        for x, y in zip(rows[a], rows[c]):
            if x != "-" and y != "-":
                got.add((ia, ic))
            ia += x != "-"
            ic += y != "-"
        return got
    hit = tot = 0
    for a in range(len(true_rows)):
        if a == c:
            continue
        t = pairs(true_rows, a)
        hit += len(t & pairs(star, a))
        tot += len(t)
    return hit, tot
