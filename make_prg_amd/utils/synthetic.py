"""Deterministic synthetic MSAs for the BASELINE.json configs (generator spec: SURVEY.md §8(d)).

One NumPy `default_rng(seed)` stream per MSA; the call order below is part of the spec (fixtures depend on it).
"""
from typing import List, Tuple

import numpy as np

_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _mutate(rng, x, p):
    y = x.copy()
    m = rng.random(x.shape[0]) < p
    y[m] = rng.integers(0, 4, int(m.sum()))
    return y


def synth_rows(seed: int, S: int, C: int, n_clades: int) -> List[bytes]:
    """Rows of one synthetic MSA (bytes over ACGT-), ids are s0..s{S-1}."""
    rng = np.random.default_rng(seed)
    root = rng.integers(0, 4, C)
    clades = [_mutate(rng, root, 0.03) for _ in range(n_clades)]
    rows = []
    for _ in range(S):
        row = _mutate(rng, clades[int(rng.integers(0, n_clades))], 0.004)
        txt = _BASES[row].copy()
        for st in np.nonzero(rng.random(C) < 0.0005)[0]:
            ln = int(rng.integers(1, 12))
            txt[st:st + ln] = ord("-")
        rows.append(txt.tobytes())
    return rows


def config_shape(config: str, seed: int) -> Tuple[int, int, int]:
    """(S, C, n_clades) for a BASELINE config letter: B = 1k x (50x500), C = 30k pan-genome, D = deep single MSA."""
    if config == "B":
        return 50, 500, 2 + seed % 5
    if config == "C":
        g = np.random.default_rng([seed, 1])
        S = int(np.clip(round(g.normal(100, 20)), 20, 300))
        C = int(g.integers(1000, 3001))
        return S, C, 2 + seed % 5
    if config == "D":
        return 10000, 20000, 8
    raise ValueError(config)


def synth_fasta(seed: int, S: int, C: int, n_clades: int) -> str:
    rows = synth_rows(seed, S, C, n_clades)
    return "".join(f">s{i}\n{r.decode()}\n" for i, r in enumerate(rows))


def synth_config_fasta(config: str, seed: int) -> str:
    return synth_fasta(seed, *config_shape(config, seed))


def synth_rows_deep(seed: int, S: int, C: int, fanout=(3, 3, 3, 3, 3), rates=(0.6, 0.5, 0.4, 0.35, 0.3),
                    window: int = 60, period: int = 200, p_background: float = 0.0005, p_row: float = 0.0002,
                    p_gap: float = 0.0001) -> List[bytes]:
    """Rows of a HIERARCHICAL alignment (ids s0..): a conserved backbone with one hyper-variable window of `window`
    columns every `period` columns.  A tree of clades (fanout[l] children per node at level l) is grown from a random
    root: inside the windows a child differs from its parent with substitution rate rates[l], elsewhere with
    p_background; the S rows are drawn from the leaf clades with rare private substitutions (p_row) and gap runs
    (p_gap).  Unlike synth_rows (one flat layer of clades: at 10k x 20k a root and one multi-allele leaf) the recursion
    NESTS here: every window is a non-match interval whose rows KMeans separates by top clade, the children separate the
    sub-clades, and so on down to max_nesting — sibling clades stay further apart than the one-reference-like threshold
    (20 % of the width) at every level.  Used for the parity-checked deep case "Ddeep" (2 000 x 4 000, -N 7); the call
    order on default_rng(seed) is part of the fixture."""
    rng = np.random.default_rng(seed)
    in_window = (np.arange(C) % period) >= (period - window)
    level = [rng.integers(0, 4, C)]
    for fan, rate in zip(fanout, rates):
        pvec = np.where(in_window, rate, p_background)
        nxt = []
        for parent in level:
            for _ in range(fan):
                child = parent.copy()
                m = rng.random(C) < pvec
                child[m] = rng.integers(0, 4, int(m.sum()))
                nxt.append(child)
        level = nxt
    rows = []
    for _ in range(S):
        row = _mutate(rng, level[int(rng.integers(0, len(level)))], p_row)
        txt = _BASES[row].copy()
        for st in np.nonzero(rng.random(C) < p_gap)[0]:
            ln = int(rng.integers(1, 12))
            txt[st:st + ln] = ord("-")
        rows.append(txt.tobytes())
    return rows


def diverged_locus(seed: int, n: int, min_len: int = 800, max_len: int = 1200, p_delete: float = 0.015, p_substitute: float = 0.06,
                   p_insert: float = 0.015, max_insert: int = 4) -> Tuple[List[str], List[str]]:
    """(seqs, true_rows): n sequences mutated from one random root of min_len .. max_len nt, and the alignment that is TRUE by
    construction.  Per root base one draw u on random.Random(seed): u < p_delete deletes it, u < p_delete + p_substitute replaces it
    by a drawn base (which may be the same one), u > 1 - p_insert puts 1 .. max_insert drawn bases behind it: the draws, and so the
    sequences, of `tools/star_measure.py --diverged` (the draw order is part of the recorded digests).  A root base and whatever
    replaces it share a column; a sequence's insertion behind root position j gets columns of its own, behind column j and ordered
    by sequence index (independent insertions are not homologous); all-gap columns are dropped.  Every row ungaps to its sequence."""
    import random
    r = random.Random(seed)
    root = "".join(r.choice("ACGT") for _ in range(r.randint(min_len, max_len)))
    base = [[None] * len(root) for _ in range(n)]            # per sequence and root position its base, None: deleted
    inserts = [dict() for _ in range(n)]                     # per sequence {root position: the insertion behind it}
    seqs = []
    for i in range(n):
        s = []
        for j, ch in enumerate(root):
            u = r.random()
            if u < p_delete:
                continue
            base[i][j] = r.choice("ACGT") if u < p_delete + p_substitute else ch
            s.append(base[i][j])
            if u > 1.0 - p_insert:
                inserts[i][j] = "".join(r.choice("ACGT") for _ in range(r.randint(1, max_insert)))
                s.append(inserts[i][j])
        seqs.append("".join(s))
    rows: List[List[str]] = [[] for _ in range(n)]
    for j in range(len(root)):
        if any(base[i][j] is not None for i in range(n)):
            for i in range(n):
                rows[i].append(base[i][j] or "-")
        for k in range(n):
            ins = inserts[k].get(j)
            if ins:
                for i in range(n):
                    rows[i].append(ins if i == k else "-" * len(ins))
    return seqs, ["".join(x) for x in rows]


def fragment_locus(seed: int, n: int, min_len: int = 800, max_len: int = 1200, share: float = 0.3,
                   keep: Tuple[float, float] = (0.3, 0.8)) -> Tuple[List[str], List[str]]:
    """(seqs, true_rows): diverged_locus(seed, n, min_len, max_len) with partial records: every record but the first is, with
    probability `share`, cut to a piece of keep[0] .. keep[1] of its length (at least 20 nt) that keeps its left end, its right end
    or lies inside, the choice drawn too; the residues cut away become '-' in its true row and all-gap columns are dropped, so the
    alignment stays TRUE by construction.  The cuts are drawn on a generator of their own (seed ^ 0x5EED), behind diverged_locus'
    draws, which are untouched: the sequences of `tools/star_measure.py --diverged --fragments`."""
    import random
    seqs, rows = diverged_locus(seed, n, min_len, max_len)
    r = random.Random(seed ^ 0x5EED)
    out = []
    for k, row in enumerate(rows):
        if k > 0 and r.random() < share:                     # record 0 stays whole
            L = len(seqs[k])
            m = max(20, int(L * r.uniform(*keep)))
            side = r.choice("LRB")                           # keep the left end, the right end, or a piece inside
            a = 0 if side == "L" else (L - m if side == "R" else r.randint(0, L - m))
            q = -1
            new = []
            for ch in row:
                if ch != "-":
                    q += 1
                    new.append(ch if a <= q < a + m else "-")
                else:
                    new.append("-")
            row = "".join(new)
        out.append(row)
    cols = [c for c in range(len(out[0])) if any(x[c] != "-" for x in out)]
    out = ["".join(x[c] for c in cols) for x in out]
    return [x.replace("-", "") for x in out], out


def synth_deep_fasta(seed: int, S: int, C: int) -> str:
    return "".join(f">s{i}\n{r.decode()}\n" for i, r in enumerate(synth_rows_deep(seed, S, C)))
