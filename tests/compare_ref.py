"""TEST-ONLY plain-Python statement of `compare_msa` (make_prg_amd/from_msa/msa_compare.py holds the spec): the DEFINITION (the
sets of aligned residue pairs of the two MSAs, O(R^2 W): for small loci) and the HISTOGRAM form the kernels compute (Counters:
for large ones), the row matching, and the old generator of tools/star_measure.py --diverged, restated."""
import random
from collections import Counter
from typing import List, Optional, Sequence, Tuple

COMPLEMENT = str.maketrans("ACGTRYKMSWN", "TGCAYRMKSWN")
PREFIX = "_R_"


def revcomp(s: str) -> str:
    return s.translate(COMPLEMENT)[::-1]


def ungap(row: str) -> str:
    return row.replace("-", "")


def match(test_ids: Sequence[str], ref_ids: Sequence[str]) -> Tuple[List[int], List[bool]]:
    """Per reference row its test row and whether it is reversed (the spec's Rows)."""
    have = set(test_ids)
    rev = [t.startswith(PREFIX) and t[len(PREFIX):] not in have for t in test_ids]
    keys = [t[len(PREFIX):] if r else t for t, r in zip(test_ids, rev)]
    if len(set(keys)) == len(keys) and len(set(ref_ids)) == len(ref_ids) and set(keys) == set(ref_ids):
        rows = [keys.index(r) for r in ref_ids]
        return rows, [rev[i] for i in rows]
    assert len(test_ids) == len(ref_ids)
    return list(range(len(ref_ids))), [rev[i] and keys[i] == ref_ids[i] for i in range(len(ref_ids))]


def columns_of(row: str) -> List[int]:
    return [c for c, ch in enumerate(row) if ch != "-"]


def t_columns(test: Sequence[str], ref: Sequence[str], rows=None, rev=None) -> List[List[int]]:
    """t(k, .): per reference row the test column of each of its residues, in the reference's numbering; asserts the spec's Same
    sequences."""
    rows = list(range(len(ref))) if rows is None else rows
    rev = [False] * len(ref) if rev is None else rev
    out = []
    for k, r in enumerate(ref):
        t = test[rows[k]]
        assert ungap(r) == (revcomp(ungap(t)) if rev[k] else ungap(t)), (k, r, t)
        cols = columns_of(t)
        out.append(cols[::-1] if rev[k] else cols)
    return out


def by_definition(test: Sequence[str], ref: Sequence[str], rows=None, rev=None) -> Tuple[int, ...]:
    """The six counts from the sets of residue pairs: a pair is ((row a, residue p), (row b, residue q)), a < b, in one column."""
    t = t_columns(test, ref, rows, rev)
    r = [columns_of(x) for x in ref]

    def pairs(cols):
        out = set()
        for a in range(len(cols)):
            for b in range(a + 1, len(cols)):
                at = {c: q for q, c in enumerate(cols[b])}
                out.update(((a, p), (b, at[c])) for p, c in enumerate(cols[a]) if c in at)
        return out

    pt, pr = pairs(t), pairs(r)
    ref_cols = kept = ident = 0
    for c in range(len(ref[0]) if ref else 0):
        members = [(k, r[k].index(c)) for k in range(len(ref)) if c in r[k]]
        if len(members) < 2:
            continue
        ref_cols += 1
        vs = {t[k][p] for k, p in members}
        if len(vs) == 1:
            kept += 1
            v = vs.pop()
            ident += sum(1 for k in range(len(ref)) if v in t[k]) == len(members)
    return len(pt & pr), len(pr), len(pt), ref_cols, kept, ident


def by_histogram(test: Sequence[str], ref: Sequence[str], rows=None, rev=None) -> Tuple[int, ...]:
    """The six counts as the spec's Counts state them."""
    t = t_columns(test, ref, rows, rev)
    m = Counter(c for cols in t for c in cols)
    W = len(ref[0]) if ref else 0
    v = [dict(zip(columns_of(x), t[k])) for k, x in enumerate(ref)]
    shared = ref_pairs = ref_cols = kept = ident = 0
    for c in range(W):
        h = Counter(v[k][c] for k in range(len(ref)) if c in v[k])
        n = sum(h.values())
        shared += sum(x * (x - 1) // 2 for x in h.values())
        ref_pairs += n * (n - 1) // 2
        if n >= 2:
            ref_cols += 1
            if len(h) == 1:
                kept += 1
                ident += m[next(iter(h))] == n
    return shared, ref_pairs, sum(x * (x - 1) // 2 for x in m.values()), ref_cols, kept, ident


def random_alignment(rng: random.Random, seqs: Sequence[str], extra: Optional[int] = None) -> List[str]:
    """The sequences as rows of one width with the gaps placed at random: all-gap columns and all-gap rows happen."""
    W = max((len(s) for s in seqs), default=0) + (rng.randint(0, 3) if extra is None else extra)
    rows = []
    for s in seqs:
        at = set(rng.sample(range(W), len(s)))
        it = iter(s)
        rows.append("".join(next(it) if c in at else "-" for c in range(W)))
    return rows


def random_pair(rng: random.Random, max_rows: int = 7, max_len: int = 9, alphabet: str = "ACGT"):
    """Two random alignments (test, ref) of the same 1 .. max_rows sequences of 0 .. max_len residues."""
    seqs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, max_len))) for _ in range(rng.randint(1, max_rows))]
    return random_alignment(rng, seqs), random_alignment(rng, seqs)


def old_diverged_seqs(seed: int, n: int) -> List[str]:
    """tools/star_measure.py's diverged_seqs as it was before diverged_locus: the draws diverged_locus must repeat."""
    r = random.Random(seed)
    root = "".join(r.choice("ACGT") for _ in range(r.randint(800, 1200)))
    out = []
    for _ in range(n):
        s = []
        for ch in root:
            u = r.random()
            if u < 0.015:
                continue
            s.append(r.choice("ACGT") if u < 0.075 else ch)
            if u > 0.985:
                s.append("".join(r.choice("ACGT") for _ in range(r.randint(1, 4))))
        out.append("".join(s))
    return out
