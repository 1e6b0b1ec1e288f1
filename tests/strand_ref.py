"""Test-side statement of the Orientation step of `from_msa --unaligned --adjust-direction` (the spec: the docstring of
make_prg_amd/from_msa/star_align.py) in plain Python / NumPy, over tests/star_ref.py (k-mer counts, the existing
centre-star spec) and tests/align_ref.py (the pair DP, whose scores settle what the k-mers leave undecided)."""
import random
from typing import List, Sequence, Tuple

import numpy as np

from tests import align_ref as ar
from tests import star_ref as sr

K = 6
CODE = {c: i for i, c in enumerate("ACGT-RYKMSWN")}
COMP = str.maketrans("ACGTRYKMSWN", "TGCAYRMKSWN")
PREFIX = "_R_"


def rc(s: str) -> str:
    return s.translate(COMP)[::-1]


def key(s: str) -> List[int]:
    """The order of the spec's lexicographic comparisons: cell codes, not letters."""
    return [CODE[x] for x in s]


def rc6(k):
    """Reverse complement of 6-mer indices: 4095 - k, then the six 2-bit groups in reverse order."""
    k = 4095 - np.asarray(k, np.int64)
    out = np.zeros_like(k)
    for q in range(K):
        out = (out << 2) | ((k >> (2 * q)) & 3)
    return out


def kmers(s: str) -> np.ndarray:
    """The 6-mer indices of s's valid windows (ACGT only), in order."""
    if len(s) < K:
        return np.zeros(0, np.int64)
    lut = np.full(256, 4, np.int64)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    win = np.lib.stride_tricks.sliding_window_view(lut[np.frombuffer(s.encode(), np.uint8)], K)
    return (win[(win < 4).all(1)] * (4 ** np.arange(K - 1, -1, -1))).sum(1)


def canonical_counts(s: str) -> np.ndarray:
    c = np.zeros(4 ** K, np.int64)
    k = kmers(s)
    np.add.at(c, np.minimum(k, rc6(k)), 1)
    return c


def canonical_centre(seqs: Sequence[str]) -> int:
    """The centre rule of star_ref.centre over canonical counts; -1 if every sequence is empty."""
    cs = [canonical_counts(s) for s in seqs]
    T = sum(cs) if cs else np.zeros(4 ** K, np.int64)
    best, best_score = -1, None
    for a, s in enumerate(seqs):
        score = int(cs[a] @ T - cs[a] @ cs[a])
        if s and (best < 0 or score > best_score):
            best, best_score = a, score
    return best


def evidence(ref: str, s: str) -> Tuple[int, int, int]:
    """(fwd, rev, nw) of s against the forward 6-mer counts of ref."""
    h, k = sr.kmer_counts(ref), kmers(s)
    return int(h[k].sum()), int(h[rc6(k)].sum()), len(k)


def orient(seqs: Sequence[str]) -> Tuple[int, List[bool], str]:
    """seqs normalised -> (orientation centre, reversed flag per record, how: one of "-kdt" per record)."""
    c = canonical_centre(seqs)
    if c < 0:
        raise ValueError("every sequence is empty")
    opp, how = [False] * len(seqs), ["-"] * len(seqs)
    ref = min(seqs[c], rc(seqs[c]), key=key)
    opp[c] = seqs[c] != ref
    for a, s in enumerate(seqs):
        if a == c or not s:
            continue
        f, r, nw = evidence(ref, s)
        if 8 * abs(f - r) >= max(nw, 1):
            opp[a], how[a] = r > f, "k"
            continue
        fwd_score, rev_score = ar.align_pair_np([ref], s)[1], ar.align_pair_np([ref], rc(s))[1]
        if rev_score != fwd_score:
            opp[a], how[a] = rev_score > fwd_score, "d"
        else:
            opp[a], how[a] = key(rc(s)) < key(s), "t"
    first = next(a for a, s in enumerate(seqs) if s)
    return c, [bool(s) and opp[a] != opp[first] for a, s in enumerate(seqs)], "".join(how)


def oriented(seqs: Sequence[str]) -> Tuple[List[bool], str, List[str]]:
    """(reversed, how, the normalised sequences with the reversed ones reverse-complemented)."""
    seqs = [sr.normalise(s) for s in seqs]
    _, rev, how = orient(seqs)
    return rev, how, [rc(s) if f else s for s, f in zip(seqs, rev)]


def star_rows(seqs: Sequence[str]) -> Tuple[List[bool], str, int, List[str]]:
    """(reversed, how, centre, rows): the EXISTING spec (star_ref.star_rows) on the oriented sequences."""
    rev, how, ori = oriented(seqs)
    return (rev, how) + sr.star_rows(ori)


def titles(records: Sequence[Tuple[str, str]], rev: Sequence[bool]) -> List[str]:
    return [PREFIX + t if f else t for (t, _), f in zip(records, rev)]


def star_fasta(records: Sequence[Tuple[str, str]]) -> str:
    """The file `from_msa --unaligned --adjust-direction --msa-dir` writes for a locus."""
    rev, _, _, rows = star_rows([s for _, s in records])
    return "".join(f">{t}\n{r}\n" for t, r in zip(titles(records, rev), rows))


def flip(rng: random.Random, seqs: Sequence[str], share: float = 0.5, keep_first: bool = True) -> Tuple[List[str], List[bool]]:
    """(the sequences with a random `share` of them reverse-complemented, the flags).  keep_first: the first non-empty record
    is left alone unless it equals its own reverse complement (the subsets of the spec's flip invariance)."""
    norm = [sr.normalise(s) for s in seqs]
    first = next((a for a, s in enumerate(norm) if s), -1)
    flags = [rng.random() < share and not (keep_first and a == first and norm[a] != rc(norm[a])) for a in range(len(norm))]
    return [rc(s) if f else s for s, f in zip(norm, flags)], flags


def strand_edge_loci() -> List[List[str]]:
    """Edge cases of the Orientation step, one locus each (besides star_ref.edge_loci())."""
    a = "ACGGTCATTGCAAGCTTGACCGTATTGCAGGCATCGATTACGGCTAAGCT"
    return [
        ["TA", "TA", "ACGT"],                                          # palindromic records shorter than a window
        ["ACGT", "ACGT"],
        ["ACGTACGTACGT", "ACGTACGTACGT", "ACGTTCGTACGT"],               # a record that is its own reverse complement
        ["", a, rc(a), a[:30] + "T" + a[30:], rc(a[5:])],              # an empty first record, both strands
        [rc(a), a, a, a],                                              # the first record alone on its strand: the others follow it
        [a],                                                           # a single record
        ["ACGTRYKMSWNACGTTTGACCA", rc("ACGTRYKMSWNACGTTTGACCA"), "ACGTNNKMSWNACGTTTGACCA", "RYKM", "SWN"],   # ambiguity codes
        ["ACG", "CGT", "AC", "GT", "T"],                               # all shorter than 6 nt: the DP decides everything
        [a, rc(a), "", rc(a)[:20], a[25:]],                            # fragments of both strands
        ["AAAAAAAAAA", "TTTTTTTTTT", "AAAAATTTTT"],                    # low complexity, and a palindrome of it
    ]
