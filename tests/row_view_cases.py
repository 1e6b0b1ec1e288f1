"""One-alignment cases whose root has ONE non-match interval of chosen shape: S rows with a conserved left flank, a variable block of
n columns and a conserved right flank, so that mprg_ungap_dedupe gets an S x n view at column `left` (the flank's length).  The rows
are drawn from a few variants of two or three clades that differ in every column of the block (sub-variation inside a clade: the
cluster children are views over row index lists with narrower blocks); some rows have gaps.  The shapes walk the rule that gives a
view to k_rows_narrow (1 <= n <= 64 columns, 1 <= S <= 512 rows, not a small view of k_dedupe_wave: S <= 64 and n <= 64) from both
sides.  Shared by tests/test_row_views_emulated.py and its GPU twin tests/test_gpu_row_views.py: every builder returns texts, N, L."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
GAP = ord("-")
WIDTHS = (1, 3, 4, 5, 8, 9, 16, 17, 33, 63, 64, 65)            # 65: just outside the predicate
HEIGHTS = (2, 64, 65, 127, 128, 129, 256, 257, 512, 513)       # 513: just outside


def block(rng, S, n, n_clades=3, per_clade=4, p_gap=0.15):
    """S x n ASCII cells: rows 0 .. n_clades - 1 are the clades themselves (they differ in every column, so the block is one non-match
    interval), the rest drawn from the clades' variants; a share of the rows gets a run of gaps."""
    base = rng.integers(0, 4, n)
    variants = []
    for k in range(n_clades):
        clade = (base + k) % 4
        variants.append(clade)
        for _ in range(per_clade - 1):
            v = clade.copy()
            for pos in rng.integers(0, n, 1 + n // 16):
                v[pos] = (v[pos] + 1 + int(rng.integers(0, 3))) % 4
            variants.append(v)
    pick = [k * per_clade for k in range(min(n_clades, S))] + [int(x) for x in rng.integers(0, len(variants), max(S - n_clades, 0))]
    cells = ACGT[np.array([variants[j] for j in pick])].copy()
    for i in np.nonzero(rng.random(S) < p_gap)[0]:
        if i >= n_clades and n > 1:
            st = int(rng.integers(0, n))
            cells[i, st:st + int(rng.integers(1, 6))] = GAP
    return cells


def text_of(cells, left, right=9, seed=0):
    """The alignment: `left` conserved columns, the block, `right` conserved columns (flanks at least the minimum match length)."""
    rng = np.random.default_rng(1000 + seed)
    fl, fr = ACGT[rng.integers(0, 4, left)].tobytes().decode(), ACGT[rng.integers(0, 4, right)].tobytes().decode()
    return "".join(f">r{i}\n{fl}{row.tobytes().decode()}{fr}\n" for i, row in enumerate(cells))


def left_flank(L, col0_mod):
    """The shortest flank of at least L + 1 columns that puts the block at a column = col0_mod (mod 4)."""
    left = L + 1
    while left % 4 != col0_mod:
        left += 1
    return left


def widths(col0_mod, L=7, S=70):
    """A batch with one alignment per width, the block at a column = col0_mod (mod 4); 70 rows: not a small view."""
    rng = np.random.default_rng(300 + col0_mod)
    return [text_of(block(rng, S, n), left_flank(L, col0_mod), seed=n) for n in WIDTHS], 5, L


def heights(n=33, L=7):
    """A batch with one alignment per height (the workgroup's lanes walk 1 .. 4 rows each; 513: the big-view kernels)."""
    rng = np.random.default_rng(400 + n)
    return [text_of(block(rng, S, n), left_flank(L, S % 4), seed=S) for S in HEIGHTS], 5, L


def row_content(L=7, n=24, S=80):
    """Rows that are all gaps; ungapped lengths of exactly 7, 8, 9 and 16 (the 8-byte accumulator just short of full, full, one over,
    full twice); a gap at each of the four byte positions of a word; a row whose only kept byte is the last column."""
    rng = np.random.default_rng(500 + L)
    texts = []
    for col0_mod in range(4):
        cells = block(rng, S, n, p_gap=0.0)
        r = 5
        for _ in range(2):
            cells[r] = GAP; r += 1                                   # ulen 0
        for keep in (7, 8, 9, 16):
            cells[r, keep:] = GAP; r += 1                            # the kept bytes first ...
            cells[r, :n - keep] = GAP; r += 1                        # ... and last
            cells[r, 1:1 + n - keep] = GAP; r += 1                   # ... and around a hole
        for byte in range(4):
            for word in (0, 1, n // 4 - 1):
                cells[r, 4 * word + byte] = GAP; r += 1
        cells[r, :n - 1] = GAP; r += 1                               # only the last column is kept
        cells[r, 1:] = GAP; r += 1                                   # only the first
        assert r <= S
        texts.append(text_of(cells, left_flank(L, col0_mod), seed=col0_mod))
    return texts, 5, L


def identical_rows(L=7, n=20, S=90):
    """Rows equal without gaps but different with them (rep_u != rep_g), rows equal gaps included, a row whose first appearance is
    row 0 and repeats later, and a distinct row that appears first (and only) as the LAST row."""
    rng = np.random.default_rng(600)
    cells = block(rng, S, n, p_gap=0.0)
    twin = cells[4].copy()
    for i, at in ((10, 3), (11, 4), (12, 9), (40, 3)):               # the same ungapped row, the gap column elsewhere
        cells[i] = np.concatenate([twin[:at], [GAP], twin[at:n - 1]])
    cells[41] = cells[11]                                            # ... and a repeat gaps included
    cells[30] = cells[0]; cells[S - 2] = cells[0]                    # first appearance: row 0
    last = cells[1].copy()
    last[n // 2] = ACGT[(int(np.nonzero(ACGT == last[n // 2])[0][0]) + 1) % 4]
    last[2] = GAP
    cells[S - 1] = last                                              # first appearance: the last row
    return [text_of(cells, left_flank(L, 1)), text_of(cells[::-1].copy(), left_flank(L, 2), seed=1)], 5, L


def kmer_boundary(L):
    """Ungapped lengths L - 1 and L side by side: the long list (clustered by k-mers) and the short one (a cluster each) both fill."""
    rng = np.random.default_rng(700 + L)
    n, S = L + 6, 72
    cells = block(rng, S, n, p_gap=0.0)
    for i in range(6, S, 3):
        keep = L - 1 if i % 2 else L
        cells[i, keep:] = GAP
        if i % 4 == 0:
            cells[i] = np.roll(cells[i], n - keep)                   # the gaps first
    return [text_of(cells, left_flank(L, L % 4), seed=L)], 5, L


def mixed_batch(L=7):
    """Narrow, small (k_dedupe_wave's) and wide views in ONE call: 23 alignments, so every launch over the views has more than one
    workgroup and the wavefront-per-view launch ends on a partial group of four."""
    rng = np.random.default_rng(800)
    shapes = [(100, 40), (20, 5), (10, 200), (70, 64), (64, 64), (65, 33), (30, 65), (12, 3)] * 3
    return [text_of(block(rng, S, n), left_flank(L, j % 4), seed=j) for j, (S, n) in enumerate(shapes[:23])], 5, L
