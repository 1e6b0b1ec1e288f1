"""Seeded alignments that push the forest's kernels onto their rarer paths (global interval stacks, masks read directly, column
segments, wavefront prefix sums, shared counters, one-lane split, byte matrices ...).  Shared by the emulator tests
(tests/test_random_emulated.py) and their GPU twins (tests/test_gpu_edges.py): every builder returns the texts, N and L."""
import itertools

import numpy as np


def wide_fasta(seed, S, C, p_mut, gaps=True):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, C)
    out = []
    for i in range(S):
        y = base.copy()
        m = rng.random(C) < p_mut
        y[m] = rng.integers(0, 4, int(m.sum()))
        txt = np.frombuffer(b"ACGT", np.uint8)[y].copy()
        if gaps:
            for st in np.nonzero(rng.random(C) < 0.003)[0]:
                txt[st:st + int(rng.integers(1, 5))] = ord("-")
        out.append(f">w{i}\n{txt.tobytes().decode()}\n")
    return "".join(out)


def sprinkle(text, seed, p, alphabet="RYKMSW", cols=None):
    """The FASTA text with every non-gap cell of its sequence lines replaced, with probability p, by a uniform draw from `alphabet`
    (ambiguity codes by default; "N" for cells that no base was called for).  cols = (first, end): only cells of these columns."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet.encode(), np.uint8)
    out = []
    for line in text.splitlines():
        if not line.startswith(">"):
            cells = np.frombuffer(line.encode(), np.uint8).copy()
            hit = (rng.random(len(cells)) < p) & (cells != ord("-"))
            if cols is not None:
                hit[:cols[0]] = hit[cols[1]:] = False
            cells[hit] = letters[rng.integers(0, len(letters), int(hit.sum()))]
            line = cells.tobytes().decode()
        out.append(line + "\n")
    return "".join(out)


def sprinkled(built, seed, p, alphabet="RYKMSW", cols=None):
    """A builder's (texts, N, L) with sprinkle() over every text."""
    texts, N, L = built
    return [sprinkle(t, seed, p, alphabet, cols) for t in texts], N, L


P_AMB_WIDE, SEED_AMB_WIDE = 0.002, 7          # ambiguity codes in the three WIDE_VIEWS
P_AMB, SEED_AMB = 0.0008, 8                   # ... and in the other builders: few enough that the expansion of a leaf stays small
# many_short_clusters: only the columns between its two match intervals.  A code in one of those makes the whole alignment one
# interval of sequences longer than the k-mer size, which ten clusters hold: no node with more than SC_RANKS children is left
SHORT_CLUSTER_COLS = (10, 22)
P_N_WIDE, P_N_TALL, P_N_LEAF = 0.003, 0.001, 0.002          # N left in place (object path): WIDE_VIEWS, tall_view, leaf_of_many_alleles

WIDE_VIEWS = [(2, 1, 5, 900, 0.02),       # n/(L-1) exceeds the LDS interval stacks: global stacks
              (2, 2, 4, 1400, 0.05),
              (1, 7, 3, 13000, 0.002)]    # wider than the LDS column bytes (PT_COLS): masks read directly


def wide_view(N, L, S, C, p):
    return [wide_fasta(100 + C, S, C, p)], N, L


GAP_RUN_NL = ((3, 7), (2, 3))


def gap_runs_across_segments(N, L):
    """Rows with gap stretches across columns 2 048 and 4 096 (k_gap_runs' 512-column segments), variation inside them."""
    rng = np.random.default_rng(5)
    C = 4400
    base = rng.integers(0, 4, C)
    rows = []
    for i in range(6):
        y = np.frombuffer(b"ACGT", np.uint8)[base].copy()
        for c in (1990, 2040, 2100, 3000, 4090, 4100, 4300):          # variation: non-match columns inside and next to the stretches
            y[c] = b"ACGT"[(int(base[c]) + 1 + i % 3) % 4]
        rows.append(y)
    rows[1][2030:2060] = ord("-")          # across the first boundary
    rows[2][1985:4200] = ord("-")          # a whole segment and both boundaries
    rows[4][4096:4110] = ord("-")          # begins exactly at a boundary
    rows[5][4080:4096] = ord("-")          # ends exactly before one
    text = "".join(f">g{i}\n{r.tobytes().decode()}\n" for i, r in enumerate(rows))
    return [text], N, L


def leaf_of_many_alleles():
    """300 and 90 and 200 distinct rows under a root at the nesting limit: leaves of more than 128 alleles beside small ones."""
    rng = np.random.default_rng(21)
    texts = []
    for S in (300, 90, 200):
        C = 30
        base = rng.integers(0, 4, C)
        rows = []
        for i in range(S):
            y = base.copy()
            y[5:25] = rng.integers(0, 4, 20)
            t = np.frombuffer(b"ACGT", np.uint8)[y].copy()
            if i % 5 == 0:
                t[10:10 + i % 7] = ord("-")          # alleles of different lengths
            rows.append(t.tobytes().decode())
        texts.append("".join(f">a{i}\n{r}\n" for i, r in enumerate(rows)))
    return texts, 1, 7


def tall_view():
    """1 100 rows drawn from 12 variants of 3 clades: more rows than k_cluster_majority's LDS member lists (CF_ROWS)."""
    rng = np.random.default_rng(77)
    C = 48
    clades = [rng.integers(0, 4, C) for _ in range(3)]
    variants = []
    for cl in clades:
        for _ in range(4):
            y = cl.copy()
            y[rng.integers(0, C, 2)] = rng.integers(0, 4, 2)
            variants.append(y)
    rows = [variants[int(rng.integers(0, len(variants)))] for _ in range(1100)]
    text = "".join(f">t{i}\n{np.frombuffer(b'ACGT', np.uint8)[r].tobytes().decode()}\n" for i, r in enumerate(rows))
    return [text], 5, 7


def many_short_clusters():
    """1 100 distinct sequences shorter than the k-mer size next to 40 long ones: a cluster node with more than 1 024 children."""
    rng = np.random.default_rng(3)
    rows = [f"ACGTTGCAAC{''.join(w)}------GGATCCATGA" for w in itertools.islice(itertools.product("ACGT", repeat=6), 1100)]
    for i in range(40):
        base = list(("ACGTACGTACGT", "TTGACCTGAATC")[i % 2])
        base[int(rng.integers(0, 12))] = "ACGT"[int(rng.integers(0, 4))]
        rows.append("ACGTTGCAAC" + "".join(base) + "GGATCCATGA")
    text = "".join(f">s{i}\n{r}\n" for i, r in enumerate(rows))
    return [text], 5, 7


def wide_and_tall_view():
    """4 200 columns, 530 rows from four variants (one mutated column in every five, at different phases: the whole alignment is
    ONE non-match interval), a few with gaps (gapped twins of rows that are equal without gaps)."""
    rng = np.random.default_rng(31)
    C, S = 4200, 530
    base = rng.integers(0, 4, C)
    variants = [base.copy()]
    for v in range(3):
        y = base.copy()
        cols = np.arange(C)[np.arange(C) % 5 == v + 1]
        y[cols] = (y[cols] + 1 + v) % 4
        variants.append(y)
    pick = rng.integers(0, len(variants), S)
    pick[:8] = [3, 1, 3, 0, 2, 1, 0, 2]          # every variant's first row early, repeats in different candidate classes
    txt = [np.frombuffer(b"ACGT", np.uint8)[variants[int(p)]].copy() for p in pick]
    for i in range(5, S, 37):
        txt[i][100 + i % 50:103 + i % 50] = ord("-")
    text = "".join(f">w{i}\n{t.tobytes().decode()}\n" for i, t in enumerate(txt))
    return [text], 2, 7


def clades_without_tables():
    """Two alignments of 44 distinct sequences (five close clades + noise) whose ~750 k-mers make a 260 KB count matrix."""
    texts = []
    for seed in (92, 97):
        rng = np.random.default_rng(seed)
        C = 44
        base = rng.integers(0, 4, C)
        clades = []
        for _ in range(5):
            y = base.copy(); m = rng.random(C) < 0.3; y[m] = rng.integers(0, 4, int(m.sum())); clades.append(y)
        rows = []
        for i in range(44):
            y = clades[i % 5].copy(); m = rng.random(C) < 0.1; y[m] = rng.integers(0, 4, int(m.sum()))
            rows.append(np.frombuffer(b"ACGT", np.uint8)[y].tobytes().decode())
        texts.append("".join(f">w{i}\n{r}\n" for i, r in enumerate(rows)))
    return texts, 2, 7


def byte_matrix_problem():
    """150 distinct sequences x ~250 4-mers: a 300 KB count matrix, beyond the LDS prepare classes."""
    rng = np.random.default_rng(17)
    clades = [rng.integers(0, 4, 34) for _ in range(3)]
    rows = []
    for i in range(150):
        y = clades[i % 3].copy()
        m = rng.random(34) < 0.25
        y[m] = rng.integers(0, 4, int(m.sum()))
        rows.append("ACGTACGT" + np.frombuffer(b"ACGT", np.uint8)[y].tobytes().decode() + "TTGACCAT")
    text = "".join(f">q{i}\n{r}\n" for i, r in enumerate(rows))
    return [text], 2, 4


def many_special_leaves(n=1300):
    """n three-row alignments whose one non-match column holds R, A, C between two match intervals: a leaf with an ambiguity code in
    every alignment, more of them in one batch than the first capacity (1 024) of assemble_prgs' list of such leaves."""
    texts = []
    for i in range(n):
        b = "ACGT"[i % 4]
        texts.append(f">a\nACGTACG{b}R{b}CGTACGT\n>b\nACGTACG{b}A{b}CGTACGT\n>c\nACGTACG{b}C{b}CGTACGT\n")
    return texts, 5, 7


def special_leaves(eng):
    """The leaves that assemble_prgs hands to the host's expansion: distinct rows listed, ambiguity codes or N in the view."""
    t = eng.tab
    return (t["kind"] == 0) & (t["reps_off"] >= 0) & t["special"]


# Alignments that still hold N (object path: nothing overwrites them), a few rows each; N = 5, L = 7.
N_BY_HAND = {
    # a match interval (columns 0-8) whose first row holds N: its one allele is the N-free row's
    "match_interval_one_row_with_n": (">a\nACNTACGTTTTACGTGCA\n>b\nACGTACGTTATACGTGCA\n>c\nACGTACGTTTTACGTGCA\n",
                                      "ACGTACGTT 5 T 6 A 5 TACGTGCA"),
    # a match interval in which every row holds N, each in another column: no sequence is left
    "match_interval_every_row_with_n": (">a\nNCGTACGTT\n>b\nANGTACGTT\n>c\nACNTACGTT\n", "SequenceCurationError"),
    # a non-match interval (columns 8-10) in which every row holds N: partition status 2
    "nonmatch_interval_every_row_with_n": (">a\nACGTACGTNACTTGCATGC\n>b\nACGTACGTCNGTTGCATGC\n>c\nACGTACGTGTNTTGCATGC\n",
                                           "SequenceCurationError"),
    # a non-match interval (columns 8-10) whose N-free rows are one sequence: retyped to a match interval, three leaves in a row
    "nonmatch_interval_one_sequence_left": (">a\nACGTACGTCNCTTGCATGC\n>b\nACGTACGTATATTGCATGC\n>c\nACGTACGTATATTGCATGC\n",
                                            "ACGTACGTATATTGCATGC"),
}

# (products of alignments that hold N, errors) that the ORACLE ALONE gives for the three WIDE_VIEWS, tall_view and leaf_of_many_alleles
# with N sprinkled at P_N_WIDE, P_N_TALL, P_N_LEAF: in the wider views and among the 1 100 rows some slice has N in every row
N_VIEWS_ORACLE = [(1, 0), (0, 1), (0, 1), (0, 1), (3, 0)]

# tests/random_msas.random_cases(seed, 150) with their N left in place, as (N, L, seed, counts): what the ORACLE ALONE makes of each batch —
# (cases with a product, cases it refuses, products of alignments that hold N).  The checks must find exactly these, so none passes by
# comparing errors only or by leaving the N cases out.  (A row with N is often a cluster of its own, whose only sequence then holds N:
# about half of the alignments with N are refused, as are those with a disallowed base.)
RANDOM_WITH_N = [(5, 7, 11, (116, 34, 31)), (2, 1, 13, (121, 29, 27)), (5, 2, 15, (111, 39, 25))]
