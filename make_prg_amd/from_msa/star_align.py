"""Centre-star MSAs of `from_msa --unaligned`: every locus's unaligned sequences aligned on the GPU against one of them, the
centre, and the insertions merged (kernels: csrc/k_star.inc for the centre and the merge, csrc/k_align.inc for the pairs; C ABI:
mprg_star_centres / mprg_star_merge_columns / mprg_star_merge_rows / mprg_align_profiles / mprg_align_pairs in include/mprg.h).
With `--band` the pairs are computed over a certified band of diagonals in two passes (the spec and the proof that the ops are the
full DP's: make_prg_amd/update/profile_align.py, "Band"; C ABI: mprg_align_bounds / mprg_align_pairs_banded): the same MSAs, byte
for byte, from a fraction of the cells and of the traceback memory.
With `--adjust-direction`, records on the opposite strand are found and reverse-complemented first (Orientation below; kernels in
csrc/k_star.inc, C ABI: mprg_star_centres_canonical / mprg_star_strand / mprg_star_revcomp).

With `--progressive` the MSA is built up a guide tree instead of around a centre (Progressive below; kernels in csrc/k_prog.inc,
C ABI: mprg_prog_distances / mprg_prog_columns / mprg_align_profile_pairs / mprg_prog_rows).  With `--band` as well the merges run
over certified bands of diagonals (Progressive, band below; kernels in csrc/k_prog_band.inc, C ABI: mprg_align_profile_pairs_banded /
mprg_prog_band_widths): the same MSAs, byte for byte.

With `--collapse-identical` the records of a locus whose (oriented) sequences are identical are found on the device and aligned
once, with the class size as an integer weight; every member gets its representative's row (Collapse below; kernels in
csrc/k_collapse.inc, C ABI: mprg_star_identical / mprg_prog_columns_weighted).

With `--refine-tree` (and `--progressive`) the progressive MSA is then cut at the edges of its guide tree, one after the other, and the
two halves realigned as profiles; a realignment is kept if it raises the objective (Tree refinement below; kernels in
csrc/k_tree_refine.inc, C ABI: mprg_tree_split / mprg_tree_objective).

With `--large-loci` (and `--progressive --collapse-identical`) the leaf limit of the progressive pass counts classes, not records: a
locus of up to 2^20 records over at most 4 096 distinct sequences is built progressively (Large loci below; kernel:
csrc/k_prog_tree_wide.inc, C ABI: mprg_prog_tree_wide).

With `--retree` (and `--progressive`) the guide tree is rebuilt from the progressive MSA itself, from the identities of its rows, and
the locus is aligned again up the new tree; the new MSA is kept if it raises the objective (Retree below; kernel:
csrc/k_prog_retree.inc, C ABI: mprg_prog_identities).

With `--seq-weights` (and `--progressive`) every leaf of the guide tree gets a weight from the tree, its share of the edges above it,
and counts that often in every merge (Sequence weights below; kernel: csrc/k_prog_weights.inc, C ABI: mprg_prog_leaf_weights).

With `--pair-distances` (and `--progressive`) the first guide tree is built from the scores of the pair DP over all pairs of a locus's
leaves instead of from 6-mer counts (Pair distances below; kernels: csrc/k_align_scores.inc, C ABI: mprg_align_pair_scores /
mprg_align_pair_scores_banded; with free_end_distances the overlap scores, Free end distances below).

With `--position-gaps` (and `--progressive`) a merge charges the opening of a gap run by the occupancy of the column the run starts
at instead of -704 whatever the column (Position gaps below; kernels: csrc/pg_pairs.inc, csrc/pg_pairs_band.inc,
csrc/pg_band_widths.inc, C ABI: the _posgap entries).

With `--free-end-gaps` (and `--progressive`) a merge is an overlap alignment: the run of one side's columns alone at either end of
it is free (Free end gaps below; the same three kernel texts, C ABI: the _endgap entries).

It is NOT MAFFT.  PRGs built from these alignments differ from PRGs built from a MAFFT alignment of the same sequences.

Spec (the kernels and tests/star_ref.py follow it bit for bit)
  Input.    A locus is the records of one FASTA(.gz) file, in file order.  Each sequence is upper-cased and every '-' removed.
            Only ACGT-RYKMSWN are allowed; any other character is an error that names the locus and the record.
  Centre.   k-mers of k = 6 over ACGT only (a window with any other code is skipped).  c_a: the 4 096 counts of sequence a;
            T = sum over b of c_b; score(a) = <c_a, T> - <c_a, c_a> in int64 (= sum over b != a of <c_a, c_b>).  The centre is the
            smallest index a of a NON-EMPTY sequence that maximises score.  A locus with no records raises from_msa's
            EmptyMSAError; a locus whose sequences are all empty is an error that names it.
  Pairs.    The centre is a 1-row leaf; every other non-empty sequence is aligned against it with exactly the DP, scores and tie
            order of make_prg_amd/update/profile_align.py.  An empty sequence aligns as C deletions, no launch.
  Merge.    As profile_align.merge: boundary j (0..C) gets max_k ins_k(j) new columns, each sequence's inserted residues
            left-justified in them.  Rows in INPUT order (the centre stays at its own index), letters upper case, titles the
            records' original header lines.  (So a locus of one record is that record.)
  Invariants (tested):
            - every row with its gaps removed is its input sequence;
            - no column is all gaps;
            - identical input sequences give identical rows;
            - two equal-length sequences that differ by one substitution align without gaps: a gap-free alignment scores at
              least (L - 1) * 1280 - 576, any gapped one needs an insertion and a deletion, so at most (L - 1) * 1280 - 2688.

Orientation (only with adjust_direction; integers only; tests/strand_ref.py follows it bit for bit).  Per locus, after Input:
  rc(s).    s reversed, with A<->T, C<->G, R<->Y, K<->M, and S, W, N unchanged (cell codes 0<->3, 1<->2, 5<->6, 7<->8).  For a 6-mer
            index k (12 bits, the first base in the top two bits), rc6(k): 4095 - k, then its six 2-bit groups in reverse order.
  Centre^.  The Centre rule over CANONICAL counts: every valid window counts in bin min(k, rc6(k)); the same score and the same
            lowest-index tie rule.  It does not change when any subset of the records is reverse-complemented.
  ref.      The lexicographically smaller (in cell codes) of the sequence of Centre^ and its rc: independent of the orientation in
            which that record arrived.
  Evidence  of every other non-empty sequence a, with h the forward 6-mer counts of ref: fwd = sum of h[k_w], rev = sum of
            h[rc6(k_w)] over a's valid windows w, nw their number (int64).
  Decision  opp(a): a lies on the strand opposite to ref.  By k-mers when 8 |fwd - rev| >= max(nw, 1): opp = rev > fwd.  Else by
            DP: a and rc(a) are both aligned against ref as a 1-row leaf with the DP of Pairs, only the scores are used:
            opp = score(rc(a)) > score(a); on equal scores opp = rc(a) < a (cell codes).  (A pair and its joint reverse
            complement have the same optimal score, so this keeps the result independent of a's input orientation.)
            opp(Centre^) = its sequence is not ref.  An empty sequence is never reversed.
  Anchor.   reversed(a) = opp(a) XOR opp(first), first = the first non-empty record: it always keeps its input orientation
            (MAFFT's --adjustdirection convention), everything else follows it.
  Then      Centre, Pairs and Merge above, unchanged, on the oriented sequences (rc(s_a) where reversed(a)); rows stay in input
            order; the title of a reversed record gets the prefix _R_ (the id is the new title's first word).
  how.      Per sequence one of: - not examined (Centre^, an empty sequence, a single record), k k-mers, d DP, t DP tie.
  The constants (k = 6, the factor 8) are design choices: 6 reuses the 4 096-bin tables that fit LDS; the factor only decides who
  pays for two extra small DPs, never correctness, because an undecided sequence is settled by the alignment scores.
  Properties (tested): the output equals the flag-off output on the records with `reversed` applied and _R_ prefixed; an input
  in which nothing is reversed gives the flag-off bytes; reverse-complementing any records but the first non-empty one changes no
  row; every row with its gaps removed is its input sequence or, exactly where the title starts with _R_, its rc.

Refinement (only with refine = N > 0; integers only; tests/refine_ref.py follows it bit for bit; kernels: csrc/k_refine.inc, C ABI:
mprg_refine_counts / mprg_refine_profiles / mprg_refine_compact).  The star MSA is centre-star, not progressive: a row has only
ever seen the centre.  Up to N rounds of leave-one-out realignment follow it, each kept only if it raises the objective S.
  Round.    On a locus's current MSA A (R rows in input order, W columns).  A locus with fewer than 3 non-empty rows is never
            refined (with two rows the star alignment is already the optimal pair alignment).  s_r: row r with its gaps removed.
            Every non-empty row r is aligned against the profile of A WITH ROW r DELETED, all non-empty rows at once (every row
            sees the same A).  That profile is exactly what mprg_align_profiles gives for the (R - 1) x W matrix: the formulas of
            profile_align.py, its truncating division, by R - 1; the columns that become all-gap without row r are part of it
            (P = -640, Dc = 0).  DP, scores and tie order: profile_align.py.  An empty row stays all gaps, no launch.  The rows' ops
            over the W columns are merged by the Merge rule (boundary j gets the widest insertion of any row, inserted residues
            left-justified); every all-gap column is then removed: A', same row order and titles.
  Objective.  With c_x the count of x in {A, C, G, T} in a column and g its count of '-':
                S(A) = 2 sum_columns [20 sum_x c_x (c_x - 1) / 2 - 9 sum_{x<y} c_x c_y - 10 g (R - g)] - 11 (R - 1) runs(A)
            runs(A): the maximal runs of '-' over all rows, end runs included; int64.  R Y K M S W N score 0 against a residue and
            -10 against '-', as in sigma.  11 = 704 / 64 is the DP's gap-open cost in row-pair units; 2 SP against (R - 1) 11
            matches the sum of the rows' DP scores, in which every row pair is seen from both sides.  S is taken on the MSA after
            its all-gap columns are removed (removing one can join two of a row's runs).
  Acceptance.  A' replaces A only if S(A') > S(A); otherwise the locus keeps A and takes no further round.  A locus stops after
            N accepted rounds.  So a locus whose first round is refused is the star MSA byte for byte.
  Limit.    A round aligns a row of n residues against W columns, not against the centre's C.  A locus whose longest row has
            n + W >= 10^6 (the DP's int32 limit), or needs more full-DP traceback over n x W than the workspace budget (with or
            without band: on sparse profiles the band falls back to the full DP), takes no (further) round and keeps the MSA it
            has; it is reported with the rounds accepted so far.  The run never fails for a locus the star pass aligned.
  With adjust_direction it runs on the oriented sequences, titles unchanged; with band the realignment goes through the banded
  two-pass form (the certificate holds for any profile; sparse columns make m small and the bands wide, pairs the band does not
  help go to the full DP): the same bytes either way.

Progressive (only with progressive; integers only; tests/prog_ref.py follows it bit for bit; kernels: csrc/k_prog.inc).  The star
MSA aligns every row against one sequence; a locus with two or three sub-families has no good centre.  Here the rows are merged up
a guide tree, profile against profile.  It replaces Centre, Pairs and Merge; Input, Orientation and Refinement stay what they are.
  Input.    As above.  The leaves are the locus's non-empty sequences, by input index.  Empty records become all-gap rows; a locus
            with one non-empty record is that record; a locus with no record, or only empty ones, fails exactly as above.
  Distance. c_a: the 4 096 6-mer counts over ACGT of Centre, nw_a their sum.  s(a, b) = sum_k min(c_a[k], c_b[k]), m = min(nw_a,
            nw_b), D(a, b) = 65 536 - floor(65 536 s / m), and 65 536 when m = 0.  So 0 <= D <= 65 536.
  Tree.     Average linkage (UPGMA), exact.  A cluster's key is its lowest member index.  dist(U, V) = sum over a in U, b in V of
            D(a, b) / (|U| |V|), compared by cross-multiplication, never by a rounded quotient.  The pair with the smallest dist is
            merged; on ties the smallest key(U), then the smallest key(V), with key(U) < key(V).  With at most PROG_MAX_LEAVES =
            4 096 leaves every cross product stays below 2^60.  A locus with more non-empty records is not built progressively: it
            gets the star MSA above and is reported; the run never fails on a locus the star pass aligns.
  Merge of a node's two children.  Y is the child with more rows, on equal rows the one with the lower key; X the other.  Y's
            profile is what mprg_align_profiles writes for its R_Y x W_Y matrix: P[j][A, C, G, T], P[j][amb], Dc[j].  X's column i
            has the counts c_i[A, C, G, T], amb_i (R Y K M S W N) and g_i ('-') over its R_X rows.  With C's truncating division:
                s(i, j) = (sum_x c_i[x] P[j][x] + amb_i P[j][amb] + g_i Dc[j]) / R_X          column i against column j
                Dc[j]                                                                        Y's column j alone
                Ic[i] = (64 * -10 * (R_X - g_i)) / R_X                                       X's column i alone
            and every maximal run of either kind pays -704 more.  The DP is the global three-state DP of profile_align.py: the
            same int32 arithmetic, the same tie order (diagonal, then Y's column alone, then X's column alone; extend before open),
            end gaps charged, W_X + W_Y >= 10^6 refused.  The ops give the merged columns one for one (M: both columns, D: Y's
            column and '-' in X's rows, I: X's column and '-' in Y's rows): the node's width is the op count, nothing is
            left-justified.  The node's rows are Y's, then X's.  With R_X = 1 this is profile_align's pair DP exactly (same ops,
            same score).  |sum| <= 1 280 R_X, so the division is a multiplication and a shift on the device (k_prog.inc, pg_div).
  Output.   The root's rows in input order, the empty records as all-gap rows, titles unchanged.
  Not promised.  Identical input sequences need not give identical rows (two different sequences can have D = 0 and merge between
            them).  No sequence weighting unless seq_weights asks for it (Sequence weights below).  It is not MAFFT.  adjust_direction runs first, on the records; refine runs afterwards,
            on the progressive MSA's text on the device, unchanged.  With band the merges run over certified bands (below) and
            the realignments of refine over theirs: the same bytes.
  Invariants (tested): every row with its gaps removed is its input sequence; no column is all gaps.

Progressive, band (only with progressive and band; integers only; tests/progband_ref.py states it in plain Python; kernels:
csrc/k_prog_band.inc).  The merge's DP over the cells of a band of diagonals, with a certificate that the ops are the full DP's.
  Notation. X has n = W_X columns and R_X rows, Y has C = W_Y columns; cell (i, j) lies on diagonal d = j - i, Delta = C - n.  'D'
            (Y's column alone) adds 1 to d, 'I' (X's column alone) subtracts 1.  Band, half-widths, clamping to [-n, C] and the
            minus infinity outside: profile_align.py, "Band", with the merge's scores in place of the pair's.
  Bounds.   B_j = max(P[j][A], P[j][C], P[j][G], P[j][T], P[j][amb], Dc[j]), SB = sum_j B_j, loss_j = B_j - Dc[j] >= 0 (at most
            1 920), ins_i = -Ic[i] >= 0 (at most 640).  LY(k): the sum of the k smallest loss_j, k clamped to C; LX(k): the sum of
            the k smallest ins_i, k clamped to n.
  Why B_j bounds a matched column.  s(i, j) is the truncated quotient by R_X of a sum of R_X terms, each one of the six integers
            above, so the exact quotient is at most B_j; B_j is an integer, so the truncated quotient (a ceiling for negatives) is
            at most B_j too.  A Y column contributes s(i, j) or Dc[j]; an X column alone contributes Ic[i] <= 0.
  Upper bound.  A path that touches d* > max(0, Delta) has at least d* D ops, at least d* - Delta I ops and a run of each: it scores
            at most SB - LY(d*) - LX(d* - Delta) - 1408.  A path that touches d* < min(0, Delta) has at least Delta - d* D ops and
            -d* I ops: at most SB - LY(Delta - d*) - LX(-d*) - 1408.  (The product form m d* of the pair certificate is useless
            here: a Y column with one residue among four or more rows has B_j = Dc[j], so the smallest loss is 0 in nearly every
            merge.)  At half-width w both sides give the same number,
                U(w) = SB - LY(max(0, Delta) + w + 1) - LX(w + 1 - min(0, Delta)) - 1408,
            which does not rise with w.  So there is one certified half-width w*: the smallest w >= 0 with U(w) < S0, clamped per
            side where the band reaches the matrix's edge (w <= n + min(0, Delta) on the minus side, w <= C - max(0, Delta) on the
            plus side; both are min(n, C), and below it neither k is clamped); a side at the edge is closed.  With R_X = 1 and an
            ACGT leaf this is the pair certificate in its sorted form.
  Then      profile_align.py's argument unchanged: with both sides closed the ops and the score are the full DP's; two passes,
            never a loop: pass 1 with w0 = PROG_BAND_W0 (a tuning constant, not part of the result) gives S0, a merge with w* > w0
            runs once more with w*; a merge whose band (of pass 1, or of pass 2) does not help, by profile_align.band_helps with
            n = W_X and C = W_Y, goes to the full DP (mprg_align_profile_pairs).

Collapse (only with collapse; integers only; tests/collapse_ref.py states it in plain Python; kernels: csrc/k_collapse.inc).  It takes
effect after Input and, with adjust_direction, after Orientation: it works on the oriented sequences, so a record and a
reverse-complemented copy of it fall into one class.
  Classes.  Records a and b of a locus are identical when their sequences have the same length and the same cell codes.  rep(a) is
            the smallest index of a's class, w(a) the size of a's class, for a = rep(a).  Empty records stay what they are:
            all-gap rows with no launch (each is its own representative).
  Star.     The centre is computed as above, over ALL records, so T still counts every copy; it is then a representative by the
            lowest-index rule (equal sequences score equally).  Pairs run only for representatives other than the centre.  Members of
            the centre's class get the centre row's k = -1 form: a sequence against itself has the gap-free alignment as its unique
            optimum, so this is what the DP would have written.  mprg_star_merge_columns sees the representatives' rows only (a
            member's insertions are its representative's, so no width changes); mprg_star_merge_rows sees every row, a member's ops
            offset and op count being its representative's.  The MSA is the flag-off MSA, byte for byte; with refine after it (on
            the MSA's text, unchanged) this holds as well.
  Progressive.  The leaves are the representatives of the non-empty classes, each with weight w.  Distances are taken between
            representatives only.  The tree is exact UPGMA, as above, with |U| = sum of w over U's leaves and dist(U, V) = sum over a
            in U, b in V of w_a w_b D(a, b) / (|U| |V|), compared by cross-multiplication; keys and the tie rule are unchanged.  A
            locus with more than PROG_MAX_LEAVES non-empty RECORDS (not classes) still gets the star MSA and is reported: the 2^60
            bound stays where it is (Large loci below counts classes instead).  The merge of a node's two children takes Y as the child with the larger weight sum, on equal
            sums the one with the lower key.  Every count, P, Dc, Ic and R_X are those Progressive gives for the node's matrix with
            row r written w_r times; R is the weight sum (mprg_prog_columns_weighted; the DP kernels, the band certificate and
            pg_div work on such profiles as they are: a weighted sum is a sum of R_X terms).  A node's text holds one row per
            class.  Output: the root's rows in input order, every record its representative's row.
  Promised (tested): identical input sequences give identical rows, also after refine (identical rows see identical
            leave-one-out profiles); a locus without duplicates gives the plain progressive bytes; band gives the same bytes as
            no band.
  Host side: a _collapse stage after _orient: one mprg_star_identical launch over the chunk, one download of rep and the status
            words; the star pass and the progressive one take the class tables.  The progressive pass runs on the chunk's tables
            with the representatives only (the distance tables cover them alone), with the weights beside them; the last
            mprg_prog_rows launch names the representative's root row as the source of every member's output row.

Large loci (only with progressive, collapse and large_loci; integers only; tests/large_ref.py states it in plain Python; kernel:
csrc/k_prog_tree_wide.inc, C ABI: mprg_prog_tree_wide).  Progressive counts its leaf limit in records, so a core gene of 20 000 genomes
with forty alleles gets the star MSA although its tree has forty leaves.  Here the limit counts leaves.
  Constant. PROG_MAX_RECORDS = 2^20 = 1 048 576: PG_MAX_ROWS, the weight sum up to which mprg_prog_columns_weighted, pg_div, the DP
            kernels, the band certificate, mprg_prog_rows and mprg_tree_objective are specified.
  Rule.     A locus is built progressively iff its number of leaves, Collapse's classes of non-empty records (counted after
            Orientation when adjust_direction is on), is at most max_leaves (PROG_MAX_LEAVES unless given) AND its number of
            records, empty ones included, is at most max_records (PROG_MAX_RECORDS unless given).  Any other locus gets what it
            gets today: the star MSA, byte for byte what collapse alone gives, and (non-empty records, 0, True) in progression.
  Unchanged.  Tree, Merge and Output are Collapse's: the weighted UPGMA with its keys and tie rule, Y the child with the larger
            weight sum, every record its representative's row.  Only the bound moves.
  Bound.    With |U| + |V| <= 2^20: |U| |V| <= 2^38, a sum over a in U, b in V of w_a w_b D(a, b) <= 65 536 |U| |V| <= 2^54, and a single
            entry w_a w_b D(a, b) is below 2^56 whatever the two weights (<= 2^54 for two leaves of one locus).  So the sums stay in
            int64, a denominator needs more than 32 bits, and a cross product, at most 2^92, needs 128: mprg_prog_tree_wide
            compares in unsigned 128-bit integers, the host's prog_tree in Python integers.
  Never fails.  The run never fails on a locus the star pass aligns.  A later stage with a bound of its own that such a locus
            cannot meet skips it and reports that by its own Limit rule: Tree refinement leaves out a locus with
            (weight sum + E)^2 W > 2^58 (mprg_tree_objective's bound) and a locus above its leaf cap.
  Promised (tested): a locus of at most max_leaves records gives the bytes it gives without large_loci; multiplying every weight of
            a tree by a constant does not change the tree; band, device_tree and the host tree give the same bytes; equal sequences
            get equal rows; every row with its gaps removed is its input sequence.
  Host side: the classes exist only after _orient and _collapse, inside a chunk, so the decision is made there: the loci of more
            than max_records records go to the star chunks beforehand, every other locus to a progressive chunk, which counts
            classes per locus from Collapse's own table and, where some locus is over max_leaves, runs the star pass over those and
            the progressive pass over the others, both on the chunk's code buffer and class table (_star_chunk_parts).  With
            device_tree the loci whose weight sum exceeds PROG_MAX_LEAVES form budget groups of their own, whose distances launch is
            followed by mprg_prog_tree_wide; all others go to mprg_prog_tree as before.

Tree refinement (only with progressive and refine_tree = N > 0; integers only; tests/treerefine_ref.py states it in plain Python;
kernels: csrc/k_tree_refine.inc, C ABI: mprg_tree_split / mprg_tree_objective).  Progressive never looks back at a merge, and
Refinement's second look is one row against all others; a locus of two or three sub-families carries its errors on the tree's inner
edges, clade against clade.  Here the tree is cut at an edge, the two halves are realigned as profiles, and the result is kept if
the objective rises.
  Where.    After the last merge of Progressive, on the root's text: one row per leaf (with collapse one row per class, with the
            class weights), before the rows are put into input order.  adjust_direction has run before it, refine runs after it,
            unchanged, on the text that results.
  Which loci.  Those built progressively with 4 <= m <= TREE_REFINE_MAX_LEAVES = 512 leaves (with fewer no edge has two leaves on
            either side).  The cap is a cost constant: a pass costs about as many DP cells as the whole progressive stage, and its
            steps are sequential per locus.  A locus above it keeps its progressive MSA and is reported.
  Steps.    The tree's merges are numbered t = 0 .. m - 2 in the order UPGMA made them (prog_tree's and mprg_prog_tree's order);
            L_t is the set of leaves under node t.  The steps of a locus are the nodes t = 0 .. m - 3, ascending, with
            m - |L_t| >= 2.  If both children of the root are inner nodes they cut the same split: the one with the smaller t is
            left out, so the root's split comes last.
  A step    on the current MSA A (rows = leaves, weights w, all 1 without collapse): G = L_t, G' the other leaves.  A_G: G's rows
            over the columns in which one of them is not '-', columns in order, rows in the order they have in A; A_G' likewise.
            Y is the side with the larger weight sum, on equal sums the side that holds the locus's lowest leaf index; X the
            other.  The merge is exactly Progressive's "Merge of a node's two children" with Collapse's weights: the same planes,
            DP and ties.  A': Y's rows, then X's, over the ops; it has no all-gap column by construction.
  Objective.  Refinement's S of the locus's OUTPUT MSA: every row counts w_r times and the locus's E empty records count as all-gap
            rows.  R = sum w + E; c_x is summed over the weights, g over the weights plus E; runs = sum w_r runs(row r) + E.  So it
            is the number mprg_refine_counts gives for the MSA as written.
  Acceptance.  A' replaces A only if S(A') > S(A).  A pass visits all steps in order, each on the MSA the accepted steps before it
            left.  A locus takes up to N passes; a pass without an accepted step ends its refinement.
  Limit.    A step with W_X + W_Y >= 10^6, or whose full-DP traceback exceeds the workspace budget, is skipped and counts as
            refused; skipped steps are reported.  The run never fails on a locus that the progressive pass built.
  With band the merges go through _prog_pairs' certified two passes: the same bytes.
  Promised (tested): every row with its gaps removed is its input sequence; no column is all gaps; S never falls; a locus all of
            whose steps are refused has its progressive bytes; with collapse equal sequences get equal rows; band and device_tree
            give the same bytes.
  Host side (_tree_refine, between _prog_rounds and _prog_output): step s of every locus of the chunk that still has a step s
            goes together: one mprg_tree_split launch into a buffer of the step's own, one download of the widths and status
            words (20 bytes per item), _prog_groups / _prog_pairs on the two halves as ordinary sides, mprg_prog_rows into a new
            text buffer per group, one mprg_tree_objective launch, one download of S (8 bytes per item).  The host keeps per
            locus its row order (Y's leaves, then X's) and where its current text is; a buffer is dropped when no locus points to
            it.  No MSA text leaves the device during the stage.

Retree (only with progressive and retree = N > 0; integers only; tests/retree_ref.py states it in plain Python; kernel:
csrc/k_prog_retree.inc, C ABI: mprg_prog_identities).  The guide tree is built once, from 6-mer distances, which say little about how
two sequences align and saturate on diverged sub-families; Tree refinement only re-cuts the edges of that same tree.  Here the
distances are taken a second time, from the MSA the first tree built, a new tree is built from them and the locus aligned again
(MAFFT's --retree 2, MUSCLE's stage 2, Clustal Omega's --iter).
  Where.    After the last merge of Progressive, on the root's text: one row per leaf (with collapse one row per class, with the
            class weights), before Tree refinement, before the rows are put into input order and before refine.  adjust_direction
            has run before it.
  Which loci.  Those built progressively with 3 or more leaves (two leaves have one tree).  A locus for which mprg_tree_objective's
            bound does not hold ((weight sum + E)^2 W > 2^58) is left out and reported ("bound"), as Tree refinement does.  The run
            never fails on a locus the progressive pass built.
  Distance. Rows a and b are the leaves' rows of the current MSA A.  nw'_a: the cells of row a that are A, C, G or T (cell codes
            0..3).  s'(a, b): the columns in which both rows hold the same code and that code is 0..3; '-' against '-' is no match,
            nor are two equal ambiguity codes or N against N.  D'(a, b) = 65 536 - floor(65 536 s' / min(nw'_a, nw'_b)), and 65 536
            when the minimum is 0.  So s' <= min(nw'_a, nw'_b): a table of s above the diagonal and a vector nw, exactly what
            prog_distance_matrix, mprg_prog_tree and mprg_prog_tree_wide take from mprg_prog_distances; they are used unchanged.
            It is the identity over the shorter sequence, and was chosen for that reason: the same shape, scale and bounds as
            Progressive's D, so the tree code, its 2^60 (2^92) bounds and its tie rule need nothing new.
  Tree.     Progressive's Tree on D'; Collapse's weighted tree when there are weights: exact, the same keys and tie rule; on the
            host, or with device_tree on the device, a locus whose weight sum exceeds 4 096 by mprg_prog_tree_wide.
  Iteration.  Up to N times per locus: (1) D' from the current MSA, and the tree T' on it.  (2) If T' has the same merge list as
            the tree that built the current MSA the locus stops ("same"): no merge is run, a rebuild would reproduce the bytes.
            (3) Otherwise the MSA A' is built from the leaves up T': Merge, the choice of Y and X and the row order are
            Progressive's (Collapse's with weights).  (4) A' replaces A only if S(A') > S(A); otherwise the locus keeps A and stops
            ("refused").  S is Tree refinement's Objective: rows count w_r times, the locus's E empty records as all-gap rows.
  Limit.    A merge of the rebuild that Tree refinement's Limit would skip (W_X + W_Y >= 10^6, or a full-DP traceback beyond the
            workspace budget) ends the locus's retree with the MSA it has ("limit").
  Afterwards.  Tree refinement, if asked for, runs on the accepted MSA with the accepted tree's merges and row order; progression
            reports the leaves and rounds of the tree that built the MSA that is written.
  Promised (tested): every row with its gaps removed is its input sequence; no column is all gaps; S never falls; a locus that
            stops "same" or "refused" at its first iteration has its progressive bytes; band, device_tree and the host tree give
            the same bytes; with collapse equal sequences get equal rows and a locus without copies gets the bytes it gets without
            collapse; with large_loci the large loci go through it like any other.
  Host side (_retree, between _prog_rounds and _tree_refine): one mprg_tree_objective launch for S of the first MSAs; then per
            iteration all loci of the chunk that are still iterating go together: in _prog_trees' budget groups (prog_tree_bytes)
            one mprg_prog_identities launch into tables laid out as _distances_launch lays them out (PI_BLOCK_ROWS = 16 rows a
            work item), and with device_tree mprg_prog_tree(_wide) over the tables where they are (the merges and the status words
            come back), without it the tables downloaded and prog_tree(prog_distance_matrix(...)) on the host; _prog_plan for the
            loci whose tree changed; _prog_rounds for those loci alone, from the leaves in buffer 0, into new text buffers; one
            mprg_tree_objective launch, 8 bytes of S per locus downloaded.  The old root's buffer is dropped when the new MSA is
            accepted, the new one when it is refused (_prog_rounds' live counts).  No MSA text leaves the device during the stage.

Sequence weights (only with progressive and seq_weights; integers only; tests/weights_ref.py states it in plain Python; kernel:
csrc/k_prog_weights.inc, C ABI: mprg_prog_leaf_weights).  At a merge every row of a profile counts once, so an over-sampled clade
outvotes a rare sub-family wherever the two are joined (with collapse: a class of 6 000 copies counts 6 000 times).  A leaf's weight
is the tree length it does not share with its relatives (ClustalW's scheme), so a crowded clade counts about as much as a lonely one.
  Per locus, over what the tree was built from: the leaves (non-empty records; with collapse the class representatives) and their
            multiplicities m_a (1 without collapse), the distances D(a, b) the tree was built on (Progressive's 6-mer D, or
            Retree's D' for a rebuilt tree), and the tree's merges in order, as (key(U), key(V)).
  Heights.  For the inner node t that merges clusters U and V: N_t = sum over a in U, b in V of m_a m_b D(a, b); |U| = sum of m_a
            over U; H_t = floor(N_t / (|U| |V|)).  A leaf has H = 0.  Under Large loci's limits N_t <= 2^54, the divisor <= 2^38,
            H_t <= 65 536.
  Edges.    The edge above a node c with parent t has len(c) = max(H_t - H_c, 0) and n_c = the multiplicity sum of the leaves
            below c.  UPGMA's own trees never need the clamp (average linkage has no inversions and the floor is monotone;
            tests/weights_ref.py's loci show none); the kernel accepts any valid merge list.
  Raw weight.  c_a = sum over the nodes c on the path from leaf a (inclusive) to the root (exclusive) of
            floor(256 len(c) m_a / n_c).  The numerator is at most 2^44, and c_a <= 2^24.  With collapse this is the weight of the
            whole class: m_a records, each with its share.
  Weight.   M = max_a c_a.  q_a = 1 if M = 0, else 1 + floor(255 c_a / M).  So 1 <= q_a <= 256 and the sum over at most 4 096 leaves
            is at most 2^20: exactly what mprg_prog_columns_weighted, pg_div and PG_MAX_ROWS accept.
  Merge.    Progressive's merge through Collapse's weighted column tables, with the row of leaf a counting q_a times on both
            sides; R_Y and R_X are the q sums.
  Nothing else changes: the tree, the choice of Y (rows, or with collapse the multiplicity sum, then the lower key), the rounds and
            the output order, Collapse's expansion, and the objective S, which stays the sum of pairs over records and
            multiplicities, never over q.
  Two facts (tested): multiplying every q of a locus by a constant changes no plane and no score ((64 k v) / (k R) truncates like
            (64 v) / R, and the same holds for X's counts); so, without collapse, a locus whose leaves all get the same q keeps
            its progressive bytes, and a locus of fewer than 3 leaves needs no weights at all (two leaves always get equal q).
  With      adjust_direction first; band, device_tree and a small budget_bytes give the same bytes; collapse and large_loci as
            above (equal sequences still get equal rows); retree: the pass up a rebuilt tree uses the weights from that tree and
            from D', acceptance by S as before; refine_tree: a step's realignment counts every row with the q of the tree that
            built the accepted MSA, acceptance by S with multiplicities as before; refine runs afterwards, unchanged and unweighted.
  The flag promises the stated weights, not a higher S: S counts every record equally, and moves either way by fractions of a percent.
  Host side: a stage in _progressive after the plan.  With device_tree the weights launch joins each group's launches in
            _prog_trees (the tables and the merges are still on the device); with the host's tree the group's tables are computed
            again by _distances_launch and the merges uploaded (the tables are never weighted on the host).  Only q (4 bytes a
            record) and the status words come back.  _prog_rounds, _tree_refine and _retree take q as a second per-record array,
            the alignment weights, beside the multiplicities, which keep their role in the plan, the expansion and S;
            _retree_trees launches the weights over the identity tables it already has on the device.  leaf_weights is the same
            statement in Python integers.

Pair distances (only with progressive and pair_distances; integers only; tests/pairdist_ref.py states it in plain Python; kernels:
csrc/k_align_scores.inc, C ABI: mprg_align_pair_scores / mprg_align_pair_scores_banded).  Progressive's 6-mer distances saturate: two
records that differ at one base in five share almost no 6-mer, so on a locus of diverged sub-families nearly every D sits near 65 536
and UPGMA's tie rule decides the tree, not the data.  Here the first tree comes from the scores of the pair DP over all pairs of
leaves (ClustalW's pairwise mode, MAFFT's --globalpair).
  Leaves.   Progressive's: the non-empty records, with collapse the class representatives, after Orientation.
  Score.    For leaves a < b (table indices) score(a, b) is the score of profile_align.py's DP of sequence a against sequence b as a
            1-row leaf: its formulas, its int32 arithmetic, end gaps charged.  Three facts of two sequences against each other
            (tested): score(a, b) = score(b, a), because a residue against a gap costs -640 on either side and a run -704 on
            either; every score is a multiple of 64 (one row: no division leaves a remainder); score <= 1 280 min(acgt_a, acgt_b),
            acgt the cells with code 0..3, because only an equal ACGT pair scores above 0.
  Tables.   s''(a, b) = max(score(a, b), 0) / 64, nw''_a = 20 acgt_a, D''(a, b) = 65 536 - floor(65 536 s'' / min(nw''_a, nw''_b)),
            and 65 536 when the minimum is 0.  So 0 <= s'' <= min(nw''): a table of s'' above the diagonal beside a vector nw'', the
            shape and the bounds of what _distances_launch leaves, so prog_distance_matrix, prog_tree, mprg_prog_tree,
            mprg_prog_tree_wide and mprg_prog_leaf_weights, with their 2^60 and 2^92 bounds, are used unchanged.  A pair with an
            empty record is not run: its entry is 0 and the record's nw'' is 0.
  Which loci.  Those built progressively with 3 to PAIR_DIST_MAX_LEAVES = 512 leaves.  The cap is a cost constant, like
            TREE_REFINE_MAX_LEAVES: a locus costs m (m - 1) / 2 pair DPs.  A locus above it is reported as "cap", a locus with a pair
            of n + C >= 10^6 as "limit"; both get Progressive's 6-mer tree.  The run never fails on a locus the progressive pass
            builds without the flag.
  Nothing else changes: Merge, Y and X, the rounds, the output order and the objective S.  collapse: the tree is the weighted one
            over the representatives.  large_loci: the wide tree kernel on the same tables.  device_tree: the tables stay on the
            device.  seq_weights: the heights come from D'', the distances the tree was built on.  retree: its D' replaces D'' for
            a rebuilt tree, as it replaces D without the flag; "same" compares with the tree that built the current MSA.
            refine_tree, refine, adjust_direction: unchanged.  band: the scores come over certified bands (profile_align.py,
            "Band": band_plan and certified_widths unchanged, SB and m from mprg_align_bounds) and are the same scores.
  The flag promises these distances, not a higher S.
  Host side (_pair_scores_launch, in place of _distances_launch for these loci): per group of loci one mprg_align_profiles launch
            over the leaves as 1-row texts where they lie in the code buffer, with band one mprg_align_bounds launch, then the
            pairs longest first through mprg_align_pair_scores in launches whose row buffers (8 (C + 1) bytes a pair) fit
            budget_bytes; with band pass 1 at BAND_W0, pass 2 for the pairs with w* > w0, the full form for a pair whose band spans
            the columns anyway.  The kernels write s'' into the group's tables themselves; {status, score} (8 bytes a pair) and,
            with band, the bounds are all that comes back; nw'' is counted on the host from the code arrays it holds and uploaded
            (8 bytes a record).  A locus's pair scores are computed once per run: on the host's tree with seq_weights the tables
            _prog_shared downloaded are kept and uploaded for the weights launch (_PairTables).

Position gaps (only with progressive and position_gaps; integers only; tests/posgap_ref.py states it in plain Python; kernels:
csrc/pg_pairs.inc, csrc/pg_pairs_band.inc, csrc/pg_band_widths.inc, C ABI: mprg_prog_columns_posgap /
mprg_prog_columns_weighted_posgap / mprg_align_profile_pairs_posgap / mprg_align_profile_pairs_posgap_banded /
mprg_prog_band_widths_posgap).  Progressive's merge scales what a skipped column costs to EXTEND a run by the column's occupancy (Dc,
Ic) but charges -704 to OPEN one, whatever the column: skipping a Y column in which 1 row of 50 has a residue costs -12 to extend and
-704 to open, as if all 50 rows had a residue there.  So the DP pushes X's residues into an existing insertion column and closes up
independent insertions.  Here the open of a run is scaled by the occupancy of the column it starts at, as ClustalW, MUSCLE and
MAFFT scale a profile position's gap open.
  Opens.    With Progressive's notation (Y: R_Y rows, g^Y_j gaps in column j; X: R_X rows, g_i gaps in column i; C's truncating
            division; with weights R is the weight sum and g is weighted):
                Oc[j] = (64 * -11 * (R_Y - g^Y_j)) / R_Y    opening a run of D ops whose FIRST skipped Y column is j    (-704 .. 0)
                Ox[i] = (64 * -11 * (R_X - g_i)) / R_X      opening a run of I ops whose FIRST lone X column is i       (-704 .. 0)
                D[i][j] = max(D[i][j-1] + Dc[j-1],  H[i][j-1] + Oc[j-1] + Dc[j-1])
                I[i][j] = max(I[i-1][j] + Ic[i-1],  H[i-1][j] + Ox[i-1] + Ic[i-1])
                H[i][j] = max(H[i-1][j-1] + s(i-1, j-1), D[i][j], I[i][j])
                H[0][J] = Oc[0] + sum_{j<J} Dc[j],  H[i][0] = Ox[0] + sum_{k<i} Ic[k]
  Everything else is Progressive's merge, unchanged: s(i, j), Dc, Ic, the int32 arithmetic, the tie order (diagonal, then D, then
            I; extend before open), the 4-bit traceback cell, the walk back from (n, C), the refusal at n + C >= 10^6, the ops and
            the status contract.  |64 * -11 * (R_X - g_i)| <= 704 R_X lies inside pg_div's proven range of 1 280 R_X.
  Which merges.  Every profile-profile merge of a locus: those of Progressive, of a rebuild of Retree and of a step of Tree
            refinement (all go through _prog_pairs).
  Nothing else changes: the distances and the tree, which child is Y, the row order, the objective S, refine (which runs afterwards
            unweighted and with the fixed open), the star pass, adjust_direction, pair_distances (its pair DPs keep the fixed open)
            and `update --aligner builtin`.  The flag promises these opens, not a higher S.
  Two facts (tested): when neither side has a '-' cell, Oc = Ox = -704 everywhere, so ops and score are
            mprg_align_profile_pairs' exactly; in particular every leaf-leaf merge is unchanged.  A profile over weighted rows
            equals the profile of the rows written that often, for Oc and Ox as well.
  Band.     With band the same bytes.  "Progressive, band" holds with oy = max_j Oc[j] and ox = max_i Ox[i] (both <= 0; ox = 0 when
            n = 0) in place of the two -704: a path that leaves the band touches d* > max(0, Delta) or d* < min(0, Delta), so it
            has at least one D op and at least one I op (on the plus side d* D ops and d* - Delta >= 1 I ops, on the minus side
            Delta - d* >= 1 D ops and -d* I ops), hence at least one maximal run of each kind.  The run of D ops starts at some
            column j and pays Oc[j] <= oy, the run of I ops at some column i and pays Ox[i] <= ox; further runs pay <= 0.  The
            rest of the count is unchanged (a matched or skipped Y column contributes at most B_j or Dc[j], a lone X column
            Ic[i]; the opens are extra terms, never part of B_j), so
                U(w) = SB - LY(max(0, Delta) + w + 1) - LX(w + 1 - min(0, Delta)) + oy + ox,
            which does not rise with w (oy and ox do not depend on w).  With all-ACGT one-row sides oy = ox = -704: the old U.
            The closed-sides induction of profile_align.py is untouched: it uses only that no path outside the band beats S0.  The
            bound is weaker by up to 1 408 per merge, so more merges take a second pass; the counts are in DESIGN.md §3b.
  Host side: _prog_pairs writes Y's items as kind 2 (7 planes: mprg_prog_columns_posgap, with weights
            mprg_prog_columns_weighted_posgap), sizes the column tables by 7 W_Y + 7 W_X, and calls the _posgap entries in pass 1,
            for the widths, in pass 2 and for the full form; nothing else in the launches changes.  timings receives
            position_gap_merges.

Free end gaps (only with progressive and free_end_gaps; integers only; tests/endgap_ref.py states it in plain Python; kernels:
csrc/pg_pairs.inc, csrc/pg_pairs_band.inc, csrc/pg_band_widths.inc, C ABI: mprg_align_profile_pairs_endgap /
mprg_align_profile_pairs_endgap_banded / mprg_align_profile_pairs_posgap_endgap / mprg_align_profile_pairs_posgap_endgap_banded /
mprg_prog_band_widths_endgap).  Progressive's merge is a global alignment with end gaps charged: a run of gaps at either end of a
merge pays the open and every column, like an internal deletion.  For a partial record (a gene cut at a contig edge, a truncated
hit) that is wrong twice: the missing end is billed as a deletion of hundreds of columns, and since that deletion costs no more than
an internal gap the DP can push the fragment's last residues to the far end of the profile whenever they match there slightly
better.  Here the merge is an overlap (semi-global) alignment.
  The merge of a node's two children is Progressive's merge, or Position gaps' merge when position_gaps is given too, with four
            changes to the boundary and nothing else (X has n columns, Y has C columns):
                Row 0.      H[0][J] = D[0][J] = 0 for all J: the leading D ops, where Y's columns come before X starts, pay
                            neither an open nor Dc.
                Column 0.   H[i][0] = I[i][0] = 0 for all i.
                Row n.      In the cells of the last row a D op costs 0 to extend and 0 to open:
                                D[n][j] = max(D[n][j-1], H[n][j-1])
                            (a D op in row n can only be followed by D ops, so these are exactly the trailing ones).
                Column C.   In the cells of the last column an I op costs 0 to extend and 0 to open:
                                I[i][C] = max(I[i-1][C], H[i-1][C])
  Unchanged: s(i, j), Dc, Ic and the opens of every other cell; the int32 arithmetic; the tie order (diagonal, then D, then I;
            extend before open: d_ext >= d_open extends, also where both are free); the 4-bit traceback cell; the walk back from
            (n, C) in state H; the refusal at n + C >= 10^6; the ops and the status contract.
  Score.    The score at (n, C) is the overlap optimum: it equals the maximum over the last row and the last column of the DP with
            zero borders and every other cell charged (tested against that by-definition form).  With n = 0 the result is C D ops
            and a score of 0.  Only one leading and one trailing run can be free: an I run that follows a free leading D run is an
            ordinary run and is charged.
  Which merges.  Every merge that goes through _prog_pairs: those of Progressive, of a rebuild of Retree and of a step of Tree
            refinement, the leaf-leaf merges included.
  Nothing else changes: the distances and the tree; which child is Y, and the row order; the objective S, which still counts end
            runs, so Retree and Tree refinement accept by the same S; refine, which runs afterwards with charged ends (as it runs
            with the fixed open after position_gaps); the star pass; adjust_direction; the pair DPs of pair_distances; `update
            --aligner builtin`.  Not part of it: treating the terminal '-' cells inside a profile's rows as missing data in the
            planes; any change of defaults.  The pair scores of pair_distances keep their charged ends under this flag; they are
            free under free_end_distances ("Free end distances" below).  The flag promises these boundaries, not a higher S.
  Band.     With band the same bytes.  The bound of "Progressive, band" does not carry over: a path that leaves the band can now
            take both of its forced runs for free, a leading D run in row 0 and a trailing I run in column C.  With B_j as there,
                B'_j = max(B_j, 0),   SB' = sum_j B'_j,   LY'(k) = the sum of the k smallest B'_j (k clamped to C).
            Proof.  (1) Of a path's score a matched Y column contributes at most B_j <= B'_j; a skipped Y column, charged or free,
            at most 0 = B'_j - B'_j; lone X columns and opens at most 0.  (2) A path that touches a diagonal beyond half-width w
            has at least k = max(0, Delta) + w + 1 D ops: on the plus side it touches d* >= max(0, Delta) + w + 1 and has d* D ops,
            on the minus side d* <= min(0, Delta) - w - 1 and has Delta - d* >= max(0, Delta) + w + 1 of them: the same count on
            both sides, as before.  (3) So it scores at most SB' minus the B'_j of the columns it skips, which is at most
                U(w) = SB' - LY'(max(0, Delta) + w + 1).
            U does not rise with w (LY' does not fall with k).  No open enters it, so it holds for both forms of the open and one
            widths kernel serves both.  The two-pass rule, the clamping at the matrix's edge, band_helps, w0 = PROG_BAND_W0 and
            the closed-sides induction (it uses only that no path outside the band beats S0) are unchanged.  The bound is weaker
            than Progressive's: a dense column loses about 1 280 instead of about 1 920, X's side and the two opens no longer
            count; so more merges take a second pass or go to the full DP (the counts are in DESIGN.md §3b).
  Host side: _prog_pairs chooses the entry by (position_gaps, free_end_gaps) in pass 1, for the widths
            (mprg_prog_band_widths_endgap with either open), in pass 2 and for the full form; the column tables, the sizing and
            the groups do not change.  timings receives free_end_gap_merges.

Free end pairs (opt-in: free_end_pairs, with or without progressive; integers only; tests/freepairs_ref.py states it in plain
Python; kernels: csrc/al_pairs.inc, csrc/al_pairs_band.inc, k_align_bounds_endgap in csrc/k_align.inc; C ABI:
mprg_align_pairs_endgap / mprg_align_pairs_endgap_banded / mprg_align_bounds_endgap).  Free end gaps left the sequence-against-profile
DP alone: the Pairs of the star pass and the realignments of Refinement still charge end gaps, so a fragment's missing end is billed
as a deletion of hundreds of columns there, and refine after free_end_gaps realigns every row by the DP that flag replaced.  Here
that DP is an overlap alignment too.
  The DP of a sequence s (n >= 1 residues) against a profile of C columns is profile_align.py's DP with the four boundary changes of
            Free end gaps, taken at R_X = 1 with the fixed open:
                Row 0.      H[0][J] = D[0][J] = 0.
                Column 0.   H[i][0] = I[i][0] = 0.
                Row n.      D[n][j] = max(D[n][j-1], H[n][j-1]).
                Column C.   I[i][C] = max(I[i-1][C], H[i-1][C]).
  Unchanged: P and Dc, -640, and -704 for every other run; the int32 arithmetic; the tie order (diagonal, then D, then I; extend
            before open, also where both are free); the 4-bit traceback cell; the walk back from (n, C) in state H; the refusal at
            n + C >= 10^6; the ops and the {status, score, count} contract.
  Score.    The score at (n, C) is the overlap optimum.  Identity (tested): the ops and the score equal those of
            mprg_align_profile_pairs_endgap with X the sequence as a one-row side: then s(i, j) = P[j][x] and Ic = -640.
  Which alignments.  The Pairs of the star pass, also of the loci a progressive run leaves to it (with collapse: the
            representatives' pairs), and every realignment of Refinement, on a star or a progressive MSA.
  Not changed: the score-only DPs of adjust_direction; pair_distances (its pair scores get this boundary under free_end_distances,
            "Free end distances" below, not under this flag); `update --aligner builtin`; the merges (free_end_gaps'
            business); Centre; the Merge rule (insertions at boundaries 0 and C are left-justified as always); the objective S and
            the acceptance rule, limits and reports of Refinement; the planes of a profile (terminal '-' cells stay gaps there);
            any default.
  Promised (tested): every row with its gaps removed is its input sequence; no all-gap column; identical sequences get identical
            rows in the star pass; collapse gives the bytes of the run without it; band gives the same bytes; a sequence that is an
            exact substring of the centre, occurring once, gets its residues in place with no internal gap (no path scores more
            than 1 280 n, a path with an op other than M between its first and last M, or a mismatch, scores less, and only an
            occurrence reaches 1 280 n); with the flag off every byte and every call, upload and download is what it was.
  Band.     With band the same bytes.  "Free end gaps, Band" applies with a one-row X: with B'_j = max(B_j, 0) and SB' = sum_j B'_j
            a path that leaves the band at half-width w skips at least k = max(0, Delta) + w + 1 of the profile's columns and so
            scores at most SB' - LY'(k), LY'(k) the sum of the k smallest B'_j.  The pair stage has no sort, so LY' is bounded from
            below by counting: T = 640 (a design constant, not part of any result), z = the number of columns with B'_j < T, m' =
            the smallest B'_j >= T (0 if there is none).
            Proof.  Among any k columns at most z have B'_j < T, and those contribute >= 0; each of the other max(0, k - z) or more
            has B'_j >= m'.  So LY'(k) >= m' max(0, k - z), and a path that leaves the band scores at most
                U(w) = SB' - m' max(0, max(0, Delta) + w + 1 - z),
            which does not rise with w.  (k <= C for every w < min(n, C), so no column is counted that the profile does not have;
            at w >= min(n, C) the band is the matrix.)  S0, pass 1's score, is the score of a real path, so S0 <= SB'.  The
            smallest w >= 0 with U(w) < S0 is
                w* = max(0, floor((SB' - S0) / m') + z - max(0, Delta)),
            the same on both sides, clamped per side as certified_widths clamps; with m' = 0 no U(w) falls below SB' and w* =
            min(n, C), which sends the pair to the full DP.  The two-pass rule, band_plan, band_helps, BAND_W0 and the closed-sides
            induction (it uses only that no path outside the band beats S0) are unchanged.  For a one-row centre of ACGT m' = 1 280
            and z = 0; an N in the centre costs one column of width, not the band; the sparse columns of a leave-one-out profile
            land in z.
  Host side: _star_pass and _refine hand free_end_pairs to profile_align.pairs_on_device(free_ends=True), which calls the _endgap
            form of the three entries and certified_widths_endgap; nothing else in the launches, the sizing or the counters
            changes.  timings receives free_end_pair_alignments: the pairs run with free ends, over the star pass and all
            refine rounds.

Free end distances (only with progressive, pair_distances and free_end_distances; integers only; tests/freedist_ref.py states it in
plain Python; kernels: csrc/al_scores.inc, csrc/al_scores_band.inc, included from csrc/k_align_scores.inc; C ABI:
mprg_align_pair_scores_endgap / mprg_align_pair_scores_endgap_banded).  Free end gaps and Free end pairs made the alignments overlap
alignments; the pair scores of Pair distances still charged end gaps.  With partial records that score does not measure distance: an
equal ACGT pair scores 1 280, a residue against a gap -640, a run -704 to open, so a fragment that is an exact copy of a share f of a
record of length L scores 1 280 f L - 640 (1 - f) L - 704 against it: below 0 for f < 1/3, hence s'' = 0 and D'' = 65 536, as far from
its own source as a random sequence; at f = 1/2 an exact copy still sits at D'' near 33 000.  UPGMA then joins the fragments last, or
to each other by the tie rule, and free_end_gaps cannot do its work, which needs the fragment beside its relatives.  Here the score
is the overlap score.
  Score.    For leaves a < b, score(a, b) is the score of "Free end pairs"' DP of sequence a against sequence b as a one-row leaf:
            profile_align.py's DP with four boundary changes: row 0 = 0, column 0 = 0, D ops free in row n, I ops free in column C.
            Everything else is unchanged: the cell, the int32 arithmetic, the tie order, the refusal at n + C >= 10^6.  The value
            at (n, C) is the overlap optimum.
  Four facts (tested): score(a, b) = score(b, a) (the costs are the same on either side and the four changes are mirrored by the
            exchange of rows and columns); every score is a multiple of 64; 0 <= score <= 1 280 min(acgt_a, acgt_b): the path of
            free D ops along row 0 and free I ops down column C scores 0, and only an equal ACGT pair scores above 0; score >= the
            charged score of "Pair distances", because every path costs no more here.
  Tables.   s'' = score / 64 (score >= 0: the max of "Pair distances" changes nothing); nw'' and D'' exactly as in "Pair distances".
            Hence 0 <= s'' <= min(nw''), and the tree kernels, prog_distance_matrix, prog_tree and mprg_prog_leaf_weights take the
            tables unchanged.
  Consequence (tested).  An ACGT-only record that is an exact substring of another has s'' = nw'' of the shorter, so D'' = 0.
  Which loci, the cap, "limit", the reports: "Pair distances"' rules, unchanged.
  Nothing else changes: the merges, Y and X, the row order, the objective S, the acceptance rules of Retree, Tree refinement and
            Refinement; adjust_direction's DPs; `update --aligner builtin`; any default.  seq_weights takes its heights from these
            D'', as it does from D'' without the flag; retree replaces them with D' for a rebuilt tree as before.  The flag is
            independent of free_end_gaps and free_end_pairs: any combination is allowed.
  Band.     With band the same scores.  The bound is "Free end pairs, Band" verbatim with the one-row leaf as the profile: {SB', m',
            z} from mprg_align_bounds_endgap, w* from profile_align.certified_widths_endgap; band_plan, BAND_W0 and the two-pass rule
            are unchanged.  For an ACGT leaf m' = 1 280 and z = 0, so w* = floor((1 280 C - S0) / 1 280) - max(0, Delta): every
            mismatch and every gap column of pass 1's path costs about one column of width, where the charged bound paid about
            two thirds of one; so more pairs take a second pass (the counts are in DESIGN.md §3b).
  The flag promises these distances, not a higher S and not a higher recovery.
  Host side: _pair_scores_launch(free_ends=True) calls the _endgap form of the two score entries in pass 1, in pass 2 and for the full
            form, and with band mprg_align_bounds_endgap (three int64 a leaf) and certified_widths_endgap; nothing else in the
            sizing, the order or the launches changes.  _PairTables and prog_pair_tables carry the switch.  timings receives
            free_end_distance_pairs: the pairs scored with free ends.  With the flag off every call, upload and download is what
            it was.

Progressive, host side: per chunk the distances in launches whose m x m tables fit budget_bytes (loci of three or more leaves), D
and the tree per locus in NumPy / Python integers (prog_tree: a float64 quotient only shortlists, the choice is exact).  A node's
round is 1 + the larger of its children's rounds.  With device_tree the tree is built on the device instead (csrc/k_prog_tree.inc):
per group, sized by the tables plus the tree workspaces (8 m (m + 2) bytes a locus), the distances launch and one mprg_prog_tree
launch over the tables it left there; the merges (8 bytes each) and the status words are downloaded, the shared tables and nw are
not; the plan (_prog_plan: rounds, Y and X, node ids, row order) is made on the host from either source's merges.
All nodes of one round, over all loci of the chunk, go longest first in groups
whose workspace and column tables fit budget_bytes; per group one mprg_prog_columns launch (Y's profiles, X's column tables), one
mprg_align_profile_pairs launch, {status, score, op count} per merge downloaded, one mprg_prog_rows launch that writes the
parents' texts (cell codes) into a buffer of the group's own; a buffer is dropped when its last node has been merged.  One more
mprg_prog_rows launch puts the roots' rows into input order as ASCII, where the star pass leaves its text.
With band the groups are sized by the banded need (pass 1's; the full need for a merge pass 1's band does not help), and per group
the merges go through: pass 1 (one mprg_align_profile_pairs_banded launch), one mprg_prog_band_widths launch over the same tables
and pass 1's results, one download of {SB, w*, status} (20 bytes per merge; no histogram or profile leaves the device), pass 2 for
the merges with w* > w0 and the full DP for the rest, each longest first in launches sized by the budget; a later pass overwrites
the same ops range.  The {status, score, op count} triples of all launches are downloaded at the end of the group.

Host side: loci in chunks (CHUNK_BYTES of estimated ops and output per chunk); per chunk the centres in one launch, the pairs
through profile_align.pairs_on_device (longest first, workspace-budget launches, ops left on the device), the widths and column
starts in one call, the output size downloaded (one int64 per locus), the rows in one more launch, the MSAs downloaded.
With adjust_direction, per chunk in front of that: the residues uploaded once, the canonical centres and the evidence in two
launches (the centres stay on the device between them), the decisions in NumPy, one small pairs_on_device call for the undecided
sequences in both orientations (none when there are none), one mprg_star_revcomp launch that writes the reversed records into a
tail of the code buffer, to which the sequence table then points: the centre and merge kernels read oriented sequences from that
buffer.  The pair stage uploads its sequences from host arrays, so it gets the host-side rc of the reversed records only.
With refine, per chunk behind the rows launch and on the MSA text it left on the device: one counts launch over the chunk (S of the
star MSAs, the column counts); then the loci with 3 or more non-empty rows in groups whose leave-one-out profiles (24 W bytes per
non-empty row, sized from the star widths; a round may widen them a little) fit budget_bytes (a locus that alone exceeds it is a
group of its own).  What a group holds on the device at once: its profiles (about budget_bytes), the pair stage's workspace
(budget_bytes more) and ops, its column tables, and one MSA text buffer per round that still has a locus whose last accepted round
it is (a buffer is dropped as soon as no locus points to it; at most N + 1 texts of the group).  So the refinement's memory is
bounded by two budgets and the group's texts, not by the chunk.  Per group and round: the profiles in one launch into the buffer the DP kernels read, the pairs through
profile_align.pairs_on_device(prepared=...) (residues read from the code buffer already on the device, ops left there), the merge
calls with C = W, one counts launch (S, kept columns), and only where a column emptied the compaction and a second counts launch.
Per round the host downloads S and the widths per locus and the status words, nothing larger; only the loci whose round was
accepted go into the next one.  The text of a locus whose MSA changed is downloaded from the buffer of its last accepted round.
"""
import time
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ..msa import MSA, encode
from ..update import profile_align as pa
from ..update.profile_align import _ranges, _tile_work, add_to, exclusive_sum   # (tests reach _tile_work through this module too)

K = 6
LOCUS_FIELDS, ROW_FIELDS = 4, 6           # MPRG_ST_LOCUS_FIELDS, MPRG_ST_ROW_FIELDS
CENTRE_BAD = -2                           # MPRG_ST_CENTRE_BAD
REVERSED_PREFIX = "_R_"                   # of the title of a record that --adjust-direction reverse-complemented
ROW_STATUS = {1: "row fields or ops inconsistent with the buffers", 2: "output row outside the buffer"}
CHUNK_BYTES = 1 << 29                     # estimated ops + output bytes of the loci of one chunk
RF_LOCUS_FIELDS, RF_ROW_FIELDS = 4, 3     # MPRG_RF_LOCUS_FIELDS, MPRG_RF_ROW_FIELDS
RF_STATUS = {1: "a locus's ranges outside the buffers", 2: "a row or tile out of range", 3: "the profile or the output outside its buffer"}
REFINE_DEFAULT, REFINE_MAX = 2, 16        # rounds of `--refine` alone, and the most it takes
PROG_MAX_LEAVES = 4096                    # the spec's leaf limit of a progressive locus
PROG_MAX_RECORDS = 1 << 20                # the spec's record limit of a large locus (Large loci): PG_MAX_ROWS of csrc/k_prog.inc
PROG_SCALE = 1 << 16                      # D = PROG_SCALE - floor(PROG_SCALE s / m)
PG_ITEM_FIELDS, PG_PAIR_FIELDS, PG_ROW_FIELDS = 6, 6, 8   # MPRG_PG_ITEM_FIELDS, MPRG_PG_PAIR_FIELDS, MPRG_PG_ROW_FIELDS
PG_BAND_PAIR_FIELDS = 8                   # MPRG_PG_BAND_PAIR_FIELDS
PG_WITEM_FIELDS = 8                       # MPRG_PG_WITEM_FIELDS
PG_TREE_FIELDS = 5                        # MPRG_PG_TREE_FIELDS
PROG_BAND_W0 = 64                         # pass 1's half-width of a banded merge (what was tried)
TS_ITEM_FIELDS, TS_OBJ_FIELDS = 8, 7      # MPRG_TS_ITEM_FIELDS, MPRG_TS_OBJ_FIELDS
TREE_REFINE_MAX_LEAVES = 512              # the spec's cost cap of a tree-refined locus
TREE_REFINE_MIN_LEAVES = 4                # below it no step leaves two leaves on either side
TREE_REFINE_DEFAULT, TREE_REFINE_MAX = 1, 4   # passes of `--refine-tree` alone, and the most it takes
PI_ITEM_FIELDS, PI_BLOCK_ROWS = 8, 16         # MPRG_PI_ITEM_FIELDS, MPRG_PI_BLOCK_ROWS
RETREE_DEFAULT, RETREE_MAX = 1, 4             # rebuilds of `--retree` alone, and the most it takes
SEQ_WEIGHT_UNIT = 256                         # the spec's Sequence weights: the scale of a raw weight, and the largest q
AL_SCORE_PAIR_FIELDS, AL_SCORE_BAND_PAIR_FIELDS = 5, 7   # MPRG_AL_SCORE_PAIR_FIELDS, MPRG_AL_SCORE_BAND_PAIR_FIELDS
PAIR_DIST_MAX_LEAVES = 512                    # the spec's cost cap of a locus whose tree comes from pair scores: m (m - 1) / 2 pair DPs
PAIR_DIST_MATCH = 20                          # nw'' = 20 acgt: 1 280 / 64, the most a cell of either sequence can add to s''
PAIR_DIST_MIN_LEAVES = 3                      # two leaves have one tree
PG_STATUS = {1: "an index, a tile or a source range outside its table or buffer", 2: "ops, widths and cells that do not fit each other",
             3: "the output outside its buffer"}
TREE_STATUS = {1: "a range outside its buffer, a leaf's weight below 1 or a weight sum above 4 096", 3: "the workspace outside its buffer"}
WIDE_TREE_STATUS = {1: "a range outside its buffer, a leaf's weight below 1, a weight sum above 2^20 or more than 4 096 leaves",
                    3: "the workspace outside its buffer"}
WEIGHTS_STATUS = {1: "a range outside its buffer, a multiplicity below 1, a multiplicity sum above 2^20, more than 4 096 leaves, a merge list "
                     "that is no tree over the leaves, or a table entry out of bounds", 3: "the workspace outside its buffer"}
_GAP = ord("-")
_ASCII = np.frombuffer(b"ACGT-RYKMSWN", np.uint8)


class StarAlignError(ValueError):
    pass


def _check(status: np.ndarray, what: str, table: dict, noun: str = "work item"):
    """The first non-zero status word of a launch as an error: `what` (the entry point), the `noun` it counts, its text in `table`."""
    bad = np.nonzero(status)[0]
    if len(bad):
        raise StarAlignError(f"{what}: {noun} {bad[0]}: {table.get(int(status[bad[0]]), int(status[bad[0]]))}")


class Chunk(NamedTuple):
    """The loci of one chunk: per locus its name, its records' titles and gap-free code arrays; lens, seq_off: each record's
    length and offset in the code buffer (all loci's records in one table); first, counts: each locus's records in that table;
    d_codes, codes_bytes: the code buffer on the device."""
    names: list
    titles: list
    codes: list
    lens: np.ndarray
    seq_off: np.ndarray
    first: np.ndarray
    counts: np.ndarray
    d_codes: object
    codes_bytes: int

    @property
    def n_loci(self) -> int:
        return len(self.counts)


class _Laps:
    """The wall seconds of a chunk's stages: lap(key) adds what passed since the last lap to timings[key] (no key: to nothing)."""

    def __init__(self, timings: Optional[dict]):
        self.timings, self.t = timings, time.perf_counter()

    def lap(self, key: Optional[str] = None):
        now = time.perf_counter()
        if key:
            add_to(self.timings, key, now - self.t)
        self.t = now


def locus_codes(name: str, records: Sequence[Tuple[str, str]]) -> List[np.ndarray]:
    """The locus's sequences as gap-free cell codes (upper-cased, '-' removed); a character outside ACGT-RYKMSWN is an error."""
    out = []
    for i, (title, seq) in enumerate(records):
        raw = np.frombuffer(seq.encode(), np.uint8)
        raw = np.where((raw >= ord("a")) & (raw <= ord("z")), raw - 32, raw).astype(np.uint8)
        raw = raw[raw != _GAP]
        codes = encode(raw)
        if (codes == 255).any():
            bad = chr(raw[int(np.argmax(codes == 255))]) if raw.max() < 128 else "non-ASCII"
            raise StarAlignError(f"locus {name}, record {i + 1} ({title}): character {bad!r} outside ACGT-RYKMSWN")
        out.append(codes)
    return out


def _chunks(codes: List[List[np.ndarray]], limit: int):
    lo, used = 0, 0
    for k, cs in enumerate(codes):
        longest = max((len(c) for c in cs), default=0)
        est = 3 * len(cs) * (2 * longest + 1)
        if k > lo and used + est > limit:
            yield lo, k
            lo, used = k, 0
        used += est
    if lo < len(codes):
        yield lo, len(codes)


class Options(NamedTuple):
    """The settings of star_msas, made once from its keywords and handed down to every stage.  Per keyword, with the list of
    Reports and the counters of timings that go with it:
    adjust_direction: the spec's Orientation step first; the title of a reversed record gets the prefix _R_.  orientation: a list
    that then receives per locus (reversed: a bool per record, how: a string of one of "-kdt" per record).
    band: the pairs over a certified band (True: profile_align.BAND_W0, or pass 1's half-width); the same MSAs.  timings then also
    receives profile_align.pairs_on_device's counters (band_pairs, band_second_passes, band_full_pairs, band_cells, band_full_cells).
    The score-only DP of adjust_direction keeps the full form.
    refine: N, the spec's Refinement: up to N accepted rounds per locus (0: none, nothing launches differently).  refinement: a list
    that then receives per locus (rounds accepted, S of the star MSA, S of the result).  timings also receives refine_s; the band
    counters keep adding up across the rounds.
    progressive: the spec's Progressive instead of the centre-star pass (orientation first, refinement afterwards, both unchanged).
    With band the merges run over certified bands too (True: PROG_BAND_W0, or pass 1's half-width; the same MSAs) and timings
    also receives prog_band_merges, prog_band_second_passes, prog_band_full_merges (merges sent to the full DP), prog_band_cells
    (DP cells computed, all passes and the full form) and prog_band_full_cells (W_X W_Y summed).  progression: a list that then receives per locus (leaves, rounds, fell back to star).
    max_leaves: PROG_MAX_LEAVES unless given; a locus with more non-empty records gets the star MSA.  timings also receives tree_s
    (distances and trees) and progressive_s (the merges and the rows).
    collapse: the spec's Collapse: every class of identical (oriented) sequences is aligned once and its row written for every
    member; the star MSAs are the same bytes, the progressive ones get equal rows for equal sequences.  timings also receives
    collapse_s, collapse_records, collapse_classes (the representatives, empty records included) and collapse_pairs (star) or
    collapse_merges (progressive): the pair alignments and merges made.  False: nothing launches differently.
    device_tree: only with progressive (else a ValueError): the trees of the loci of three or more leaves by mprg_prog_tree, on the
    tables mprg_prog_distances left on the device; the same merges, so the same MSAs.  timings also receives tree_device_loci.
    False: nothing launches differently.  Either way timings receives tree_plan_s: the part of tree_s spent in _prog_plan on the
    host (with device_tree the plan alone, without it the host's UPGMA too).
    refine_tree: only with progressive (else a ValueError): N, the passes of the spec's Tree refinement (1 to TREE_REFINE_MAX), on
    the loci built progressively with 4 to tree_refine_max_leaves leaves; before the rows go into input order, so before refine.
    None: nothing launches differently.  tree_refinement: a list that then receives per locus (steps tried: every step visited,
    accepted, skipped: the spec's Limit, S before, S after), None for a locus left to the star pass.  timings also receives
    tree_refine_s and tree_refine_loci, tree_refine_steps, tree_refine_accepted, tree_refine_skipped, tree_refine_above_cap
    (and tree_refine_over_bound: loci left out because mprg_tree_objective's bound on rows^2 W does not hold for them).
    large_loci: only with progressive and collapse (else a ValueError): the spec's Large loci: a locus is built progressively iff
    its classes of non-empty records number at most max_leaves and its records at most max_records (PROG_MAX_RECORDS unless
    given); the others get the star MSA and (non-empty records, 0, True) in progression, as without it.  With device_tree the
    trees of the loci whose records exceed PROG_MAX_LEAVES are built by mprg_prog_tree_wide.  timings also receives large_loci (the
    loci of more than max_leaves non-empty records built progressively), large_records (their records) and large_fallbacks (the
    loci over either limit).  False: nothing launches or computes differently.
    retree: only with progressive (else a ValueError): N, the rebuilds of the spec's Retree (1 to RETREE_MAX), on the loci built
    progressively with 3 or more leaves; behind the last merge, so before refine_tree and refine.  None: nothing launches or
    computes differently.  retreeing: a list that then receives per locus (iterations run, accepted, why it stopped: "same",
    "refused", "limit", "bound", or None when every iteration was accepted or the locus has fewer than 3 leaves, S before, S after),
    None for a locus left to the star pass.  timings also receives retree_s and retree_loci, retree_rebuilds, retree_accepted,
    retree_same_tree, retree_refused, retree_over_bound.
    seq_weights: only with progressive (else a ValueError): the spec's Sequence weights: every leaf of a locus of three or more
    leaves counts q times (1 to 256) in the merges, in the rebuilds of retree and in the realignments of refine_tree.  timings also
    receives seq_weight_loci (the loci weighted), seq_weight_min_q (the smallest q of any leaf) and seq_weight_s (the stage's wall
    seconds: its launches and downloads; on the host's tree the second distances launches too).  False: nothing launches, uploads
    or downloads differently.
    pair_distances: only with progressive (else a ValueError): the spec's Pair distances: the first tree of every locus built
    progressively with 3 to pair_dist_max_leaves leaves (PAIR_DIST_MAX_LEAVES unless given) comes from the DP scores of all its
    pairs of leaves.  pair_distancing: a list that then receives per locus (leaves, pairs run, how: "pairs", "cap", "limit", or None
    for fewer than 3 leaves), None for a locus left to the star pass.  timings also receives pair_dist_s (part of tree_s, and with
    seq_weights on the host's tree of its second lap), pair_dist_loci, pair_dist_pairs, pair_dist_cells, pair_dist_above_cap,
    pair_dist_limit, and with band pair_dist_second_passes and pair_dist_full_pairs.  False: nothing launches, uploads or
    downloads differently.
    position_gaps: only with progressive (else a ValueError): the spec's Position gaps: every profile-profile merge of a locus (of
    Progressive, of a rebuild of retree, of a step of refine_tree) opens its runs by the occupancy of the column they start at.
    timings also receives position_gap_merges (the merges made with them).  False: nothing launches, uploads or downloads
    differently.
    free_end_gaps: only with progressive (else a ValueError): the spec's Free end gaps: every such merge as an overlap alignment,
    the run of one side's columns alone at either end of it free; with position_gaps too, its opens elsewhere.  timings also
    receives free_end_gap_merges.  False: nothing launches, uploads or downloads differently.
    free_end_pairs: with or without progressive: the spec's Free end pairs: the pairs of the star pass (also of the loci a
    progressive run leaves to it) and every realignment of refine as overlap alignments.  timings also receives
    free_end_pair_alignments (the pairs run with free ends, over the star pass and all refine rounds).  False: nothing launches,
    uploads or downloads differently.
    free_end_distances: only with progressive and pair_distances (else a ValueError): the spec's Free end distances: the pair
    scores of pair_distances are overlap scores.  timings also receives free_end_distance_pairs (the pairs scored with free ends).
    False: nothing launches, uploads or downloads differently.
    The fields hold them as the stages read them: band is None, True or pass 1's half-width; refine_tree and retree are 0 when off;
    limits (large_loci, max_records) is None or (max_leaves, max_records); pair_dist (pair_distances, its cap) None or the cap."""
    budget_bytes: int = pa.DEFAULT_BUDGET_BYTES
    band: object = None
    adjust_direction: bool = False
    refine: int = 0
    progressive: bool = False
    max_leaves: int = PROG_MAX_LEAVES
    collapse: bool = False
    device_tree: bool = False
    refine_tree: int = 0
    tree_refine_max_leaves: int = TREE_REFINE_MAX_LEAVES
    limits: Optional[Tuple[int, int]] = None
    retree: int = 0
    seq_weights: bool = False
    pair_dist: Optional[int] = None
    position_gaps: bool = False
    free_end_gaps: bool = False
    free_end_pairs: bool = False
    free_end_distances: bool = False

    def star(self) -> "Options":
        """The settings of loci that go to the star pass: none of the options of progressive (free_end_pairs is not one: kept)."""
        return self._replace(progressive=False, device_tree=False, refine_tree=0, limits=None, retree=0, seq_weights=False, pair_dist=None,
                             position_gaps=False, free_end_gaps=False, free_end_distances=False)

    def merge(self, counters: Optional[dict]) -> "_Merge":
        """How the merges of a stage run under these settings, their counters into `counters`."""
        return _Merge(self.band, self.budget_bytes, counters, self.position_gaps, self.free_end_gaps)


class Reports(dict):
    """The per-locus lists star_msas fills for its caller, by keyword (KEYS); None: the caller did not ask for that one."""
    KEYS = ("orientation", "refinement", "progression", "tree_refinement", "retreeing", "pair_distancing")

    @classmethod
    def of(cls, make) -> "Reports":
        """Lists of the host's own for loci that are aligned in parts: make() for every keyword."""
        return cls((key, make()) for key in cls.KEYS)

    def add(self, key: str, values):
        if self[key] is not None:
            self[key].extend(values)

    def scatter(self, sel, part: "Reports"):
        """What the stages reported on a part's loci, `sel` of these lists' slots, into those slots (a stage that did not run: nothing)."""
        for key, vals in part.items():
            if vals:
                for k, l in enumerate(sel):
                    self[key][l] = vals[k]


def star_msas(backend, loci: Sequence[Sequence[Tuple[str, str]]], names: Optional[Sequence[str]] = None,
              budget_bytes: int = pa.DEFAULT_BUDGET_BYTES, chunk_bytes: int = CHUNK_BYTES, timings: Optional[dict] = None,
              adjust_direction: bool = False, orientation: Optional[list] = None, band=False, refine: int = 0,
              refinement: Optional[list] = None, progressive: bool = False, progression: Optional[list] = None,
              max_leaves: Optional[int] = None, collapse: bool = False, device_tree: bool = False, refine_tree: Optional[int] = None,
              tree_refinement: Optional[list] = None, tree_refine_max_leaves: int = TREE_REFINE_MAX_LEAVES, large_loci: bool = False,
              max_records: Optional[int] = None, retree: Optional[int] = None, retreeing: Optional[list] = None,
              seq_weights: bool = False, pair_distances: bool = False, pair_distancing: Optional[list] = None,
              pair_dist_max_leaves: int = PAIR_DIST_MAX_LEAVES, position_gaps: bool = False,
              free_end_gaps: bool = False, free_end_pairs: bool = False, free_end_distances: bool = False) -> List[MSA]:
    """loci: per locus its records as (title, sequence).  Returns the loci's centre-star MSAs (ids: the titles' first words,
    descriptions: the titles).  names: the loci's names for error messages (default: their indices).  timings: a dict that
    receives the wall seconds of the stages (orient, centre, pairs, merge: each ends at a download, so includes its kernels).
    Every other keyword is a setting, described at Options, or one of the lists of Reports, described there with its setting."""
    for key, on in (("device_tree", device_tree), ("seq_weights", seq_weights), ("pair_distances", pair_distances),
                    ("position_gaps", position_gaps), ("free_end_gaps", free_end_gaps)):
        if on and not progressive:
            raise ValueError(f"{key}: only with progressive")
    if free_end_distances and not (progressive and pair_distances):
        raise ValueError("free_end_distances: only with progressive and pair_distances")
    if large_loci and not (progressive and collapse):
        raise ValueError("large_loci: only with progressive and collapse")
    if max_records is not None and not (large_loci and 0 <= int(max_records) <= PROG_MAX_RECORDS):
        raise ValueError(f"max_records: only with large_loci, and at most {PROG_MAX_RECORDS}, not {max_records!r}")
    for key, n, what, most in (("refine_tree", refine_tree, "passes", TREE_REFINE_MAX), ("retree", retree, "rebuilds", RETREE_MAX)):
        if n is not None and not progressive:
            raise ValueError(f"{key}: only with progressive")
        if n is not None and not (isinstance(n, (int, np.integer)) and not isinstance(n, bool) and 1 <= n <= most):
            raise ValueError(f"{key}: a number of {what} from 1 to {most}, not {n!r}")
    if not (isinstance(refine, (int, np.integer)) and not isinstance(refine, bool) and 0 <= refine <= REFINE_MAX):
        raise ValueError(f"refine: a number of rounds from 0 to {REFINE_MAX}, not {refine!r}")
    band = None if band is False or band is None else band      # from here on: None, True or pass 1's half-width
    names = [str(i) for i in range(len(loci))] if names is None else list(names)
    for name, recs in zip(names, loci):
        if not len(recs):
            from ..subcommands.from_msa import EmptyMSAError
            raise EmptyMSAError(f"No records found in MSA of locus {name}")
    codes = [locus_codes(n, recs) for n, recs in zip(names, loci)]
    max_leaves = PROG_MAX_LEAVES if max_leaves is None else int(max_leaves)
    opts = Options(budget_bytes, band, adjust_direction, int(refine), bool(progressive), max_leaves, bool(collapse), bool(device_tree),
                   int(refine_tree or 0), int(tree_refine_max_leaves),
                   (max_leaves, PROG_MAX_RECORDS if max_records is None else int(max_records)) if large_loci else None, int(retree or 0),
                   bool(seq_weights), int(pair_dist_max_leaves) if pair_distances else None, bool(position_gaps), bool(free_end_gaps),
                   bool(free_end_pairs), bool(free_end_distances))
    reports = Reports(orientation=orientation, refinement=refinement, progression=progression, tree_refinement=tree_refinement,
                      retreeing=retreeing, pair_distancing=pair_distancing)
    if progressive:
        return _progressive_msas(backend, loci, codes, names, opts, chunk_bytes, timings, reports)
    return [m for lo, hi in _chunks(codes, chunk_bytes)
            for m in _star_chunk(backend, loci[lo:hi], codes[lo:hi], names[lo:hi], opts, timings, reports)]


def _progressive_msas(be, loci, codes, names, opts: Options, chunk_bytes, timings, reports: Reports) -> List[MSA]:
    """star_msas with progressive: the loci within the leaf limit through the progressive chunks, the others through the star
    chunks, the results (and what the caller's lists receive) back in the loci's order.  opts.limits (the spec's Large loci; None:
    without it): only the loci of more records go to the star chunks here; the progressive chunks count every locus's classes
    once Collapse has made them and send those above max_leaves through the star pass themselves."""
    n_leaves = [sum(1 for c in cs if len(c)) for cs in codes]
    out, got = [None] * len(loci), Reports.of(lambda: [None] * len(loci))
    for prog in (True, False):
        sel = [l for l in range(len(loci)) if (n_leaves[l] <= opts.max_leaves if opts.limits is None else len(codes[l]) <= opts.limits[1]) == prog]
        sub = [codes[l] for l in sel]
        part, msas = Reports.of(list), []
        for lo, hi in _chunks(sub, chunk_bytes):
            idx = sel[lo:hi]
            msas.extend(_star_chunk(be, [loci[l] for l in idx], sub[lo:hi], [names[l] for l in idx], opts if prog else opts.star(), timings, part))
        if not prog:
            part["progression"] = [(n_leaves[l], 0, True) for l in sel]
        for k, l in enumerate(sel):
            out[l] = msas[k]
        got.scatter(sel, part)
    progression = got["progression"]
    if opts.limits is not None:
        built = [l for l in range(len(loci)) if n_leaves[l] > opts.max_leaves and not progression[l][2]]
        add_to(timings, "large_loci", len(built))
        add_to(timings, "large_records", sum(len(codes[l]) for l in built))
        add_to(timings, "large_fallbacks", sum(1 for p in progression if p[2]))
    for key in Reports.KEYS:
        reports.add(key, got[key])
    return out


def _star_chunk(be, loci, codes, names, opts: Options, timings, reports: Reports) -> List[MSA]:
    """One chunk: pack, optionally orient, optionally collapse, the star pass or the progressive one (with its tree refinement),
    optionally refine, collect.  opts.limits (the spec's Large loci; only with progressive and collapse): (max_leaves, max_records):
    the loci with more classes of non-empty records, or more records, go through the star pass."""
    laps = _Laps(timings)
    chunk = _pack(be, codes, names, [[t for t, _ in recs] for recs in loci])
    if opts.adjust_direction:
        chunk, result = _orient(be, chunk, opts.budget_bytes)
        reports.add("orientation", result)
        laps.lap("orient_s")
    classes = _collapse(be, chunk, laps) if opts.collapse else None
    if opts.limits is not None:
        n_classes = np.add.reduceat(((classes.weight > 0) & (chunk.lens > 0)).astype(np.int64), chunk.first)
        build = (n_classes <= opts.limits[0]) & (chunk.counts <= opts.limits[1])
        if not build.all():
            return _star_chunk_parts(be, chunk, classes, build, opts, laps, reports)
    return _star_chunk_rest(be, chunk, classes, opts, laps, reports)


def _star_chunk_parts(be, chunk: Chunk, classes, build, opts: Options, laps, reports: Reports) -> List[MSA]:
    """_star_chunk behind Collapse for a chunk of which only the loci `build` (a bool per locus) are built progressively (the spec's
    Large loci): those as one chunk through the progressive pass, the others as one through the star pass, both over the same code
    buffer and the classes already made; the MSAs, and what the caller's lists receive, back in the chunk's order."""
    n_filled = np.add.reduceat((chunk.lens > 0).astype(np.int64), chunk.first)
    msas, got = [None] * chunk.n_loci, Reports.of(lambda: [None] * chunk.n_loci)
    for prog in (True, False):
        sel = np.nonzero(build == prog)[0]
        if not len(sel):
            continue
        rec = _ranges(chunk.first[sel], chunk.counts[sel])      # the part's records in the chunk's table, and its own tables
        at = np.full(len(chunk.lens), -1, np.int64)
        at[rec] = np.arange(len(rec))
        part = chunk._replace(names=[chunk.names[l] for l in sel], titles=[chunk.titles[l] for l in sel], codes=[chunk.codes[l] for l in sel],
                              lens=chunk.lens[rec], seq_off=chunk.seq_off[rec], first=exclusive_sum(chunk.counts[sel]), counts=chunk.counts[sel])
        mine = Reports.of(list)
        out = _star_chunk_rest(be, part, Classes(at[classes.rep[rec]], classes.weight[rec]), opts if prog else opts.star(), laps, mine)
        if not prog:
            mine["progression"] = [(int(n_filled[l]), 0, True) for l in sel]
        for k, l in enumerate(sel.tolist()):
            msas[l] = out[k]
        got.scatter(sel.tolist(), mine)
    # (orientation has been reported for the whole chunk; every other list only when its stage was asked for)
    for key, asked in (("refinement", opts.refine), ("progression", True), ("tree_refinement", opts.refine_tree), ("retreeing", opts.retree),
                       ("pair_distancing", opts.pair_dist is not None)):
        if asked:
            reports.add(key, got[key])
    return msas


def _star_chunk_rest(be, chunk: Chunk, classes, opts: Options, laps, reports: Reports) -> List[MSA]:
    """_star_chunk behind Collapse: the star pass or the progressive one (with its tree refinement), optionally refine, collect."""
    text = _progressive(be, chunk, opts, laps, reports, classes) if opts.progressive else _star_pass(be, chunk, opts.budget_bytes, opts.band, laps, classes, opts.free_end_pairs)
    moved = {}
    if opts.refine:
        res = _refine(be, chunk, text, opts.refine, opts.budget_bytes, opts.band, laps.timings, opts.free_end_pairs)
        moved = {l: r[3] for l, r in enumerate(res) if r[3] is not None}
        reports.add("refinement", (r[:3] for r in res))
        laps.lap("refine_s")
    msas = _collect(be, chunk, text, moved)
    laps.lap(None if opts.progressive else "merge_s")           # (merge_s ends at the star MSAs' download)
    return msas


def _pack(be, codes, names=None, titles=None) -> Chunk:
    """The chunk of these loci (per locus its gap-free code arrays), its residues uploaded."""
    flat = [c for cs in codes for c in cs]
    lens = np.array([len(c) for c in flat], np.int64)
    counts = np.array([len(cs) for cs in codes], np.int64)
    first = exclusive_sum(counts)
    if (np.add.reduceat(lens, first) >= 1 << 32).any():         # (every locus has a record)
        raise StarAlignError("a locus of 2^32 residues or more")
    host = np.concatenate(flat + [np.zeros(1, np.uint8)]).astype(np.uint8)
    return Chunk([str(l) for l in range(len(codes))] if names is None else names, [[""] * len(cs) for cs in codes] if titles is None else titles,
                 codes, lens, exclusive_sum(lens), first, counts, be.upload(host), len(host))


def _collect(be, chunk: Chunk, text, moved) -> List[MSA]:
    """The chunk's MSAs from the device: `text` as the star or progressive pass left it; moved: per refined locus where its text
    is instead, (device buffer, its bytes, offset, width)."""
    d_out, out_bytes, base, W = text
    counts, titles = chunk.counts, chunk.titles
    data = be.download(d_out, np.uint8, out_bytes)
    fetched, upto = {}, {}
    for l, (buf, _, off, w) in moved.items():                   # (a buffer is read up to the last byte a locus needs of it)
        upto[id(buf)] = max(upto.get(id(buf), 0), off + int(counts[l]) * w)
    msas = []
    for l in range(chunk.n_loci):
        src, off, w = data, base[l], W[l]
        if l in moved:                                          # its last accepted round's buffer, downloaded once for all its loci
            buf, _, off, w = moved[l]
            if id(buf) not in fetched:
                fetched[id(buf)] = be.download(buf, np.uint8, upto[id(buf)])
            src = fetched[id(buf)]
        rows = src[off:off + counts[l] * w].reshape(int(counts[l]), int(w))
        msas.append(MSA(_data=rows, _ids=[(t.split(None, 1) or [""])[0] for t in titles[l]], _descs=titles[l]))
    return msas


# ---- collapse
class Classes(NamedTuple):
    """The spec's Classes over a chunk's sequence table: rep: per record the index IN THAT TABLE of its representative; weight: the
    size of the class at a representative, 0 at every other record."""
    rep: np.ndarray
    weight: np.ndarray


def _identical(be, chunk: Chunk, filter_bits: int = 64) -> np.ndarray:
    """mprg_star_identical over a chunk: rep per record, as an index within its locus; one launch, one download."""
    d_seqs, d_loci = _seq_tables(be, chunk)
    n_seqs, n_loci = len(chunk.lens), chunk.n_loci
    d_got = be.empty(4 * (n_seqs + n_loci))                     # rep, then the status words
    be.call("mprg_star_identical", be.ptr(chunk.d_codes), chunk.codes_bytes, be.ptr(d_seqs), n_seqs, be.ptr(d_loci), n_loci, int(filter_bits),
            be.ptr(d_got), be.ptr(d_got) + 4 * n_seqs, be.stream, work=float(2 * chunk.lens.sum()))
    got = be.download(d_got, np.int32, n_seqs + n_loci)
    if got[n_seqs:].any():
        raise StarAlignError("mprg_star_identical: a locus's sequences lie outside the buffers")
    return got[:n_seqs].astype(np.int64)


def identical(backend, codes: Sequence[Sequence[np.ndarray]], filter_bits: int = 64) -> List[np.ndarray]:
    """mprg_star_identical over the loci (per locus its gap-free code arrays): per locus rep, the smallest index of an equal
    sequence per record.  filter_bits: how many bits of the hash filter the comparisons (the result does not depend on it)."""
    chunk = _pack(backend, codes)
    got = _identical(backend, chunk, filter_bits)
    return [got[f:f + c] for f, c in zip(chunk.first.tolist(), chunk.counts.tolist())]


def _collapse(be, chunk: Chunk, laps: _Laps) -> Classes:
    """The spec's Classes for one chunk, on the (oriented) sequences in chunk.d_codes."""
    t0 = time.perf_counter()
    rep = np.repeat(chunk.first, chunk.counts) + _identical(be, chunk)
    weight = np.bincount(rep, minlength=len(rep)).astype(np.int64)
    spent = time.perf_counter() - t0
    add_to(laps.timings, "collapse_s", spent)
    laps.t += spent                                             # (the stage before and the stage behind keep what is theirs)
    add_to(laps.timings, "collapse_records", len(rep))
    add_to(laps.timings, "collapse_classes", int((weight > 0).sum()))
    return Classes(rep, weight)


# ---- the star pass
def centres(backend, codes: Sequence[Sequence[np.ndarray]]) -> np.ndarray:
    """mprg_star_centres over the loci (per locus its gap-free code arrays): the centre index per locus, -1 if all are empty."""
    return _centre_launch(backend, "mprg_star_centres", _pack(backend, codes))[0]


def _seq_tables(be, chunk: Chunk):
    """The chunk's sequence table {offset, n} and locus table {first sequence, sequences, 0, 0}, uploaded."""
    ltab = np.zeros((chunk.n_loci, LOCUS_FIELDS), np.int64)
    ltab[:, 0], ltab[:, 1] = chunk.first, chunk.counts
    return be.upload(np.stack([chunk.seq_off, chunk.lens], 1).reshape(-1)), be.upload(ltab)


def _centre_launch(be, call, chunk: Chunk):
    """mprg_star_centres or mprg_star_centres_canonical over sequence and locus tables uploaded here: (the centres, the device
    buffers of the sequence table, the locus table and the centres)."""
    d_seqs, d_loci = _seq_tables(be, chunk)
    d_centre = be.empty(4 * chunk.n_loci)
    be.call(call, be.ptr(chunk.d_codes), chunk.codes_bytes, be.ptr(d_seqs), len(chunk.lens), be.ptr(d_loci), chunk.n_loci,
            be.ptr(d_centre), be.stream, work=float(3 * chunk.lens.sum()))
    centre = be.download(d_centre, np.int32, chunk.n_loci).astype(np.int64)
    if (centre == CENTRE_BAD).any():
        raise StarAlignError(f"{call}: a locus's sequences lie outside the buffers")
    return centre, (d_seqs, d_loci, d_centre)


def _star_pass(be, chunk: Chunk, budget_bytes, band, laps: _Laps, classes: Optional[Classes] = None, free_ends: bool = False):
    """The spec's Centre, Pairs and Merge over one chunk, on the (oriented) sequences in chunk.d_codes.  Returns the MSAs' ASCII
    text on the device: (the buffer, its bytes, each locus's offset in it, its width).  classes: the spec's Collapse: pairs for
    the representatives only, the columns from their rows, every member's row through its representative's ops.
    free_ends: the spec's Free end pairs: the pairs as overlap alignments."""
    codes, first, counts, n_loci = chunk.codes, chunk.first, chunk.counts, chunk.n_loci
    centre = _centre_launch(be, "mprg_star_centres", chunk)[0]
    laps.lap("centre_s")
    for l in np.nonzero(centre < 0)[0]:
        raise StarAlignError(f"locus {chunk.names[l]}: every sequence is empty")
    C = np.array([len(codes[l][centre[l]]) for l in range(n_loci)], np.int64)
    # the pairs: the centre as a 1-row leaf, every other non-empty sequence against it
    leaves = [codes[l][centre[l]].reshape(1, -1) for l in range(n_loci)]
    others = [[a for a in range(len(cs)) if a != centre[l] and len(cs[a])] for l, cs in enumerate(codes)]
    if classes is not None:                                     # (the centre is the lowest index of its class: equal sequences score equally)
        is_rep = classes.weight > 0
        others = [[a for a in oth if is_rep[first[l] + a]] for l, oth in enumerate(others)]
        add_to(laps.timings, "collapse_pairs", sum(map(len, others)))
    dp = pa.pairs_on_device(be, leaves, [[codes[l][a] for a in others[l]] for l in range(n_loci)], budget_bytes, band, laps.timings,
                            free_ends=free_ends)
    if free_ends:
        add_to(laps.timings, "free_end_pair_alignments", sum(map(len, others)))
    laps.lap("pairs_s")
    # rows in input order: {locus, sequence offset, n, ops offset, ops count (-1: residue i in column i), output offset}
    rows = np.zeros((len(chunk.lens), ROW_FIELDS), np.int64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4] = np.repeat(np.arange(n_loci), counts), chunk.seq_off, chunk.lens, -1
    d_ops, ops_bytes = be.empty(16), 0
    if dp is not None:
        r = first[dp.leaf] + np.array([others[l][i] for l, i in zip(dp.leaf.tolist(), dp.index.tolist())], np.int64)
        rows[r, 3], rows[r, 4] = dp.ops_off, dp.count
        d_ops, ops_bytes = dp.d_ops, dp.ops_bytes
    col_rows = None
    if classes is not None:                                     # a member's ops are its representative's; the centre's class keeps k = -1
        rows[:, 3:5] = rows[classes.rep, 3:5]
        col_rows = np.nonzero(is_rep)[0]
    text = _star_merge(be, chunk, d_ops, ops_bytes, rows, first, counts, C, col_rows)
    laps.lap("merge_s")
    return text


def _star_merge(be, chunk: Chunk, d_ops, ops_bytes, rows, lfirst, R, C, col_rows=None):
    """The spec's Merge on the device: `rows` (the row table without output offsets) of loci that have rows lfirst .. lfirst + R of
    it and C columns before the merge; residues from the chunk's code buffer, ops from d_ops.  mprg_star_merge_columns, the
    widths downloaded, mprg_star_merge_rows into a new buffer: (the buffer, its bytes, each locus's offset in it, its width).
    col_rows: the rows mprg_star_merge_columns sees (default: all)."""
    n_loci = len(R)
    cols = rows if col_rows is None else rows[col_rows]
    n_width = int((C + 1).sum())
    d_loci, d_rows = be.upload(np.stack([lfirst, R, C, exclusive_sum(C + 1)], 1).astype(np.int64)), be.upload(cols)
    d_width, d_start = be.zeros(4 * n_width), be.empty(8 * n_width)
    d_w, d_status = be.empty(8 * n_loci), be.empty(4 * len(rows))
    be.call("mprg_star_merge_columns", be.ptr(d_ops), ops_bytes, be.ptr(d_rows), len(cols), be.ptr(d_loci), n_loci, be.ptr(d_width),
            be.ptr(d_start), n_width, chunk.codes_bytes, be.ptr(d_w), be.ptr(d_status), be.stream, work=float(ops_bytes))
    W = be.download(d_w, np.int64, n_loci)
    _check(be.download(d_status, np.int32, len(cols)), "mprg_star_merge_columns", ROW_STATUS, "row")
    if (W < C).any():
        raise StarAlignError("mprg_star_merge_columns: a locus's boundaries lie outside the buffers")
    base = exclusive_sum(R * W)
    rows[:, 5] = np.repeat(base, R) + (np.arange(len(rows)) - np.repeat(lfirst, R)) * np.repeat(W, R)
    out_bytes = int((R * W).sum())
    d_rows, d_out = be.upload(rows), be.empty(max(out_bytes, 1))
    be.call("mprg_star_merge_rows", be.ptr(chunk.d_codes), chunk.codes_bytes, be.ptr(d_ops), ops_bytes, be.ptr(d_rows), len(rows),
            be.ptr(d_loci), n_loci, be.ptr(d_width), be.ptr(d_start), n_width, be.ptr(d_w), be.ptr(d_out), max(out_bytes, 1),
            be.ptr(d_status), be.stream, work=float(out_bytes + ops_bytes))
    _check(be.download(d_status, np.int32, len(rows)), "mprg_star_merge_rows", ROW_STATUS, "row")
    return d_out, out_bytes, base, W


# ---- orientation
_COMP = np.array([3, 2, 1, 0, 4, 6, 5, 8, 7, 9, 10, 11], np.uint8)


def revcomp(codes: np.ndarray) -> np.ndarray:
    """The reverse complement of a gap-free code array (A<->T, C<->G, R<->Y, K<->M; S, W, N unchanged)."""
    return _COMP[codes[::-1]]


def _lex_less(x: np.ndarray, y: np.ndarray) -> bool:
    """x < y in cell codes, for arrays of one length."""
    d = np.nonzero(x != y)[0]
    return bool(len(d)) and bool(x[d[0]] < y[d[0]])


def canonical_centres(backend, codes: Sequence[Sequence[np.ndarray]]) -> np.ndarray:
    """mprg_star_centres_canonical over the loci: the orientation centre per locus, -1 if all its sequences are empty."""
    return _centre_launch(backend, "mprg_star_centres_canonical", _pack(backend, codes))[0]


def strand_evidence(backend, codes: Sequence[Sequence[np.ndarray]], centre: Sequence[int]) -> np.ndarray:
    """mprg_star_strand over the loci against the given centre per locus, AS STORED (no swap): {fwd, rev, nw} per sequence, all
    loci's sequences in one (n, 3) int64 array."""
    chunk = _pack(backend, codes)
    return _evidence(backend, chunk, (*_seq_tables(backend, chunk), backend.upload(np.asarray(centre, np.int32))))


def _evidence(be, chunk: Chunk, tables):
    d_seqs, d_loci, d_centre = tables
    n_seqs, n_loci = len(chunk.lens), chunk.n_loci
    d_ev, d_status = be.empty(24 * n_seqs), be.empty(4 * n_loci)
    be.call("mprg_star_strand", be.ptr(chunk.d_codes), chunk.codes_bytes, be.ptr(d_seqs), n_seqs, be.ptr(d_loci), n_loci, be.ptr(d_centre),
            be.ptr(d_ev), be.ptr(d_status), be.stream, work=float(chunk.codes_bytes))
    if be.download(d_status, np.int32, n_loci).any():
        raise StarAlignError("mprg_star_strand: a locus's sequences or its centre lie outside the buffers")
    return be.download(d_ev, np.int64, 3 * n_seqs).reshape(-1, 3)


def revcomp_on_device(be, d_codes, codes_bytes: int, jobs: np.ndarray):
    """mprg_star_revcomp: jobs (n, 3) int64 {source offset, n, destination offset} inside the device buffer."""
    d_jobs, d_status = be.upload(jobs.astype(np.int64)), be.empty(4 * len(jobs))
    be.call("mprg_star_revcomp", be.ptr(d_codes), codes_bytes, be.ptr(d_jobs), len(jobs), be.ptr(d_status), be.stream,
            work=float(2 * jobs[:, 1].sum()))
    if len(jobs) and be.download(d_status, np.int32, len(jobs)).any():
        raise StarAlignError("mprg_star_revcomp: a job's ranges lie outside the buffer or overlap")


def orientations(backend, codes: Sequence[Sequence[np.ndarray]], names: Optional[Sequence[str]] = None,
                 budget_bytes: int = pa.DEFAULT_BUDGET_BYTES) -> List[Tuple[List[bool], str]]:
    """The spec's Orientation step alone over the loci (per locus its gap-free code arrays): per locus (reversed, how)."""
    return _orient(backend, _pack(backend, codes, names), budget_bytes)[1]


def _orient(be, chunk: Chunk, budget_bytes):
    """The spec's Orientation step for one chunk.  The reverse complements of the records it reverses are written by the device
    into a tail of the code buffer, and the sequence table points there.  Returns the oriented chunk (its code arrays: what the
    pair stage uploads; the sequence offsets, the device buffer and its size; the reversed records' titles prefixed) and per
    locus (reversed flags, how codes)."""
    lens, seq_off, first, counts, n_loci = chunk.lens, chunk.seq_off, chunk.first, chunk.counts, chunk.n_loci
    n_seqs = len(lens)
    centre, tables = _centre_launch(be, "mprg_star_centres_canonical", chunk)
    for l in np.nonzero(centre < 0)[0]:
        raise StarAlignError(f"locus {chunk.names[l]}: every sequence is empty")
    ev = _evidence(be, chunk, tables)
    flat = [c for cs in chunk.codes for c in cs]
    locus_of = np.repeat(np.arange(n_loci), counts)
    cidx = first + centre
    # the reference orientation: the smaller of the centre and its reverse complement; against the latter fwd and rev swap
    refs, c_opp = [], np.zeros(n_loci, bool)
    for l in range(n_loci):
        s = flat[cidx[l]]
        r = revcomp(s)
        c_opp[l] = _lex_less(r, s)
        refs.append(r if c_opp[l] else s)
    swap = c_opp[locus_of]
    fwd, rev, nw = np.where(swap, ev[:, 1], ev[:, 0]), np.where(swap, ev[:, 0], ev[:, 1]), ev[:, 2]
    nonempty = lens > 0
    other = nonempty & (np.arange(n_seqs) != cidx[locus_of])
    by_k = other & (8 * np.abs(fwd - rev) >= np.maximum(nw, 1))
    opp = by_k & (rev > fwd)
    opp[cidx] = c_opp
    how = np.full(n_seqs, ord("-"), np.uint8)
    how[by_k] = ord("k")
    und = np.nonzero(other & ~by_k)[0]
    if len(und):
        # both orientations of every undecided sequence against its locus's reference: one small batch of pairs, scores only
        und_loci = np.unique(locus_of[und])
        dp = pa.pairs_on_device(be, [refs[l].reshape(1, -1) for l in und_loci],
                                [[x for u in und[locus_of[und] == l] for x in (flat[u], revcomp(flat[u]))] for l in und_loci], budget_bytes)
        score = dp.score.reshape(-1, 2)                  # (pairs come back in leaf order, then sequence order: und's order)
        opp[und], how[und] = score[:, 1] > score[:, 0], ord("d")
        for i in np.nonzero(score[:, 1] == score[:, 0])[0]:
            opp[und[i]], how[und[i]] = _lex_less(revcomp(flat[und[i]]), flat[und[i]]), ord("t")
    # the first non-empty record keeps its orientation, everything else follows it
    anchor = np.minimum.reduceat(np.where(nonempty, np.arange(n_seqs), n_seqs), first)
    rev_flag = nonempty & (opp != opp[anchor[locus_of]])
    rv = np.nonzero(rev_flag)[0]
    d_codes, codes_bytes = chunk.d_codes, chunk.codes_bytes
    if len(rv):
        dst = chunk.codes_bytes + exclusive_sum(lens[rv])
        codes_bytes = chunk.codes_bytes + int(lens[rv].sum())
        d_codes = be.grown(d_codes, chunk.codes_bytes, codes_bytes)
        revcomp_on_device(be, d_codes, codes_bytes, np.stack([seq_off[rv], lens[rv], dst], 1))
        seq_off = seq_off.copy()
        seq_off[rv] = dst
        for u in rv:
            flat[u] = revcomp(flat[u])
    per_locus = [slice(first[l], first[l] + counts[l]) for l in range(n_loci)]
    result = [(rev_flag[s].tolist(), how[s].tobytes().decode()) for s in per_locus]
    titles = [[REVERSED_PREFIX + t if r else t for t, r in zip(ts, rev)] for ts, (rev, _) in zip(chunk.titles, result)]
    return chunk._replace(titles=titles, codes=[flat[s] for s in per_locus], seq_off=seq_off, d_codes=d_codes, codes_bytes=codes_bytes), result


# ---- progressive
def _distances_launch(be, chunk: Chunk, d_seqs, grp):
    """One mprg_prog_distances launch over the loci `grp` of a chunk: (m, each table's offset, the tables' words, the tables, nw
    and the status words on the device, the work items)."""
    lens, first = chunk.lens, chunk.first
    m = chunk.counts[grp]
    toff = exclusive_sum(m * m)
    words = int((m * m).sum())
    ltab = np.zeros((len(grp), LOCUS_FIELDS), np.int64)
    ltab[:, 0], ltab[:, 1], ltab[:, 3] = first[grp], m, toff
    work = np.stack([np.repeat(np.arange(len(grp)), m), _ranges(np.zeros(len(grp), np.int64), m)], 1).astype(np.int32)
    d_loci, d_work = be.upload(ltab), be.upload(work)
    d_shared, d_nw, d_status = be.zeros(4 * words), be.zeros(8 * len(lens)), be.empty(4 * len(work))
    be.call("mprg_prog_distances", be.ptr(chunk.d_codes), chunk.codes_bytes, be.ptr(d_seqs), len(lens), be.ptr(d_loci), len(grp),
            be.ptr(d_work), len(work), be.ptr(d_shared), words, be.ptr(d_nw), be.ptr(d_status), be.stream,
            work=float((m * np.add.reduceat(lens, first)[grp]).sum() + 16384.0 * (m * m).sum()))
    return m, toff, words, d_shared, d_nw, d_status, len(work)


def _acgt(chunk: Chunk) -> np.ndarray:
    """Per record of the chunk's tables the cells with code 0..3, from the code arrays the host holds (reverse-complementing a
    record does not change the number)."""
    return np.array([int((c < 4).sum()) for cs in chunk.codes for c in cs], np.int64)


def _pair_scores_launch(be, chunk: Chunk, d_seqs, grp, band=None, counters=None, acgt=None, budget_bytes=pa.DEFAULT_BUDGET_BYTES,
                        free_ends=False):
    """The spec's Pair distances over the loci `grp` of a chunk: what _distances_launch returns, the tables s'' and nw'' in its layout,
    so _prog_shared, _prog_trees and _prog_weights take either source.  One mprg_align_profiles launch over the group's leaves as
    1-row texts, with band one mprg_align_bounds launch, then the pairs a < b of every locus (sequence a against leaf b), longest
    first, through mprg_align_pair_scores in launches whose row buffers fit budget_bytes; with band the spec's two passes
    (profile_align.band_plan, certified_widths) through mprg_align_pair_scores_banded and the full form for the rest, a later pass
    overwriting the pair's entry.  {status, score} per pair and, with band, the bounds are all that comes back.  acgt: per record
    of the chunk's tables its ACGT cells (default: counted from chunk.codes); nw'' = 20 acgt is uploaded.  counters receives
    pair_dist_pairs, pair_dist_cells and with band pair_dist_second_passes, pair_dist_full_pairs.  The status words returned are
    a single zero: every pair's status has been checked here.
    free_ends: the spec's Free end distances: the _endgap form of the two score entries, with band mprg_align_bounds_endgap (three
    int64 a leaf) and certified_widths_endgap; nothing else in the sizing, the order or the launches changes.  counters then also
    receives free_end_distance_pairs."""
    lens, first = chunk.lens, chunk.first
    m = chunk.counts[grp]
    toff = exclusive_sum(m * m)
    words = int((m * m).sum())
    acgt = _acgt(chunk) if acgt is None else np.asarray(acgt, np.int64)
    d_shared, d_nw, d_status = be.zeros(4 * words), be.upload(PAIR_DIST_MATCH * acgt), be.zeros(4)
    # the leaves: the group's non-empty records, each a 1-row text where it lies in the code buffer
    rec = _ranges(first[grp], m)
    lrec = rec[lens[rec] > 0]
    C = lens[lrec]
    leaf_at = np.full(len(lens), -1, np.int64)
    leaf_at[lrec] = np.arange(len(lrec))
    pa_, pb_, dst = [], [], []
    for k, l in enumerate(grp.tolist()):
        lv = np.nonzero(lens[first[l]:first[l] + m[k]] > 0)[0]
        ia, ib = np.triu_indices(len(lv), 1)
        pa_.append(first[l] + lv[ia])
        pb_.append(first[l] + lv[ib])
        dst.append(toff[k] + lv[ia] * m[k] + lv[ib])
    pa_, pb_, dst = (np.concatenate(x).astype(np.int64) if x else np.zeros(0, np.int64) for x in (pa_, pb_, dst))
    n_pairs = len(pa_)
    if not n_pairs:
        return m, toff, words, d_shared, d_nw, d_status, 1
    pn, pc, pl = lens[pa_], lens[pb_], leaf_at[pb_]
    k = np.nonzero(pn + pc >= pa.MAX_LEN)[0]
    if len(k):
        raise StarAlignError(f"a pair of {pn[k[0]]} residues against {pc[k[0]]} columns: n + C must stay below {pa.MAX_LEN}")
    prof_off = exclusive_sum(6 * C)
    d_leaves = be.upload(np.stack([chunk.seq_off[lrec], np.ones(len(lrec), np.int64), C, prof_off], 1).astype(np.int64))
    work = _tile_work(C)
    d_work, d_prof = be.upload(work), be.empty(4 * int((6 * C).sum()))
    be.call("mprg_align_profiles", be.ptr(chunk.d_codes), be.ptr(d_leaves), be.ptr(d_work), len(work), be.ptr(d_prof), be.stream,
            work=float(C.sum()))
    soff = chunk.seq_off[pa_]
    score = np.zeros(n_pairs, np.int64)
    pending = []                                                # (pairs, call, the launch's {status, score}): in launch order

    def launches(call, idx, wordsv, dlo=None, dhi=None):
        for sel, ws_off, used in pa.budget_launches(idx, wordsv, budget_bytes, StarAlignError, "pair", pn, pc):
            band_cols = () if dlo is None else (dlo[sel], dhi[sel])
            d_pairs = be.upload(np.stack([pl[sel], soff[sel], pn[sel], ws_off, dst[sel], *band_cols], 1).astype(np.int64))
            d_ws, d_out = be.empty(4 * used), be.empty(8 * len(sel))
            be.call(call, be.ptr(d_prof), be.ptr(d_leaves), len(lrec), be.ptr(chunk.d_codes), be.ptr(d_pairs), len(sel), be.ptr(d_ws), used,
                    be.ptr(d_shared), words, be.ptr(d_out), be.stream, work=pa.sweep_work(pn[sel], pc[sel], *band_cols))
            pending.append((sel, call, d_out))

    def collect():
        for sel, call, d_out in pending:                         # in launch order: a later pass's result replaces pass 1's
            res = be.download(d_out, np.int32, 2 * len(sel)).reshape(-1, 2)
            bad = np.nonzero(res[:, 0])[0]
            if len(bad):
                raise StarAlignError(f"{call}: {pa.STATUS.get(int(res[bad[0], 0]), int(res[bad[0], 0]))}")
            score[sel] = res[:, 1]
        pending.clear()
    need = (2 * (pc + 1) + 63) // 64 * 64
    w0 = None if band is None or band is False else pa.BAND_W0 if band is True else int(band)
    full_call, band_call = (("mprg_align_pair_scores_endgap", "mprg_align_pair_scores_endgap_banded") if free_ends else
                            ("mprg_align_pair_scores", "mprg_align_pair_scores_banded"))
    if w0 is None:
        launches(full_call, np.argsort(-((pn + 1) * pc), kind="stable"), need)
        collect()
        cells = int((pn * pc).sum())
    else:
        if w0 < 0:
            raise StarAlignError("band: a negative half-width")
        n_bounds = 3 if free_ends else 2
        d_bounds = be.empty(8 * n_bounds * len(lrec))
        be.call("mprg_align_bounds_endgap" if free_ends else "mprg_align_bounds", be.ptr(d_prof), be.ptr(d_leaves), len(lrec), be.ptr(d_bounds),
                be.stream, work=float((6 * C).sum()))
        bounds = be.download(d_bounds, np.int64, n_bounds * len(lrec)).reshape(-1, n_bounds)[pl]

        def band_need(dlo, dhi):
            return (2 * (dhi - dlo + 1) + 63) // 64 * 64

        def pass1(firstp, dlo, dhi):
            launches(band_call, firstp, band_need(dlo, dhi), dlo, dhi)
            collect()
            return (pa.certified_widths_endgap if free_ends else pa.certified_widths)(pn, pc, *bounds.T, score)
        second, rest, dlo, dhi, counts = pa.band_plan(pn, pc, w0, pass1)
        launches(band_call, second, band_need(dlo, dhi), dlo, dhi)
        launches(full_call, rest, need)
        collect()
        cells = int(counts[3])
        add_to(counters, "pair_dist_second_passes", int(counts[1]))
        add_to(counters, "pair_dist_full_pairs", int(counts[2]))
    add_to(counters, "pair_dist_pairs", n_pairs)
    add_to(counters, "pair_dist_cells", cells)
    if free_ends:
        add_to(counters, "free_end_distance_pairs", n_pairs)
    return m, toff, words, d_shared, d_nw, d_status, 1


class _PairTables:
    """The spec's Pair distances as a source of tables for _prog_shared, _prog_trees and _prog_weights: called like
    _distances_launch.  keep: the tables _prog_shared downloads are kept per locus, and a group all of whose loci are kept is
    uploaded, not launched again (the host's tree with seq_weights: a locus's pair scores are computed once per run).  free_ends: the
    spec's Free end distances."""

    def __init__(self, band, counters, acgt, budget_bytes, keep=False, free_ends=False):
        self.band, self.counters, self.acgt, self.budget_bytes, self.free_ends = band, counters, acgt, budget_bytes, free_ends
        self.cache, self.spent = ({} if keep else None), 0.0

    def __call__(self, be, chunk: Chunk, d_seqs, grp):
        t0 = time.perf_counter()
        if self.cache is not None and all(l in self.cache for l in grp.tolist()):
            m = chunk.counts[grp]
            flat = np.concatenate([self.cache[l] for l in grp.tolist()]).astype(np.uint32)
            got = (m, exclusive_sum(m * m), int((m * m).sum()), be.upload(flat), be.upload(PAIR_DIST_MATCH * self.acgt), be.zeros(4), 1)
        else:
            got = _pair_scores_launch(be, chunk, d_seqs, grp, self.band, self.counters, self.acgt, self.budget_bytes,
                                      self.free_ends)
        self.spent += time.perf_counter() - t0
        return got


def prog_pair_tables(backend, codes: Sequence[Sequence[np.ndarray]], band=None, budget_bytes: int = pa.DEFAULT_BUDGET_BYTES,
                     counters: Optional[dict] = None, free_ends: bool = False):
    """The spec's Pair distances over the loci (per locus its gap-free code arrays; an empty one is no leaf): per locus (s'', nw''):
    s'' an (m, m) int64 array whose part above the diagonal holds max(score(a, b), 0) / 64 of the records a < b, nw'' = 20 acgt per
    record (0 for an empty one).  band: None, True or pass 1's half-width: the same tables over certified bands.  free_ends: the spec's Free end
    distances: score is the overlap score."""
    chunk = _pack(backend, codes)
    got = _prog_shared(backend, chunk, np.arange(len(codes)), budget_bytes,
                       _PairTables(band, counters, _acgt(chunk), budget_bytes, free_ends=free_ends))
    return [got[l] for l in range(len(codes))]


def _prog_shared(be, chunk: Chunk, sel, budget_bytes, tables=None):
    """mprg_prog_distances over the loci `sel` of a chunk, in groups whose m x m tables fit budget_bytes: per locus (s as an
    (m, m) int64 array of which the part above the diagonal is filled, nw).  tables: another source of the tables, called like
    _distances_launch (the spec's Pair distances)."""
    lens, first, counts = chunk.lens, chunk.first, chunk.counts
    out = {}
    d_seqs = be.upload(np.stack([chunk.seq_off, lens], 1).reshape(-1))
    for lo, hi in pa.budget_groups(4 * counts[sel] ** 2, budget_bytes):
        grp = sel[lo:hi]
        m, toff, words, d_shared, d_nw, d_status, n_work = (tables or _distances_launch)(be, chunk, d_seqs, grp)
        _check(be.download(d_status, np.int32, n_work), "mprg_prog_distances", PG_STATUS)
        shared = be.download(d_shared, np.uint32, words).astype(np.int64)
        nw = be.download(d_nw, np.int64, len(lens))
        for k, l in enumerate(grp.tolist()):
            out[l] = (shared[toff[k]:toff[k] + m[k] * m[k]].reshape(int(m[k]), int(m[k])), nw[first[l]:first[l] + counts[l]])
            if getattr(tables, "cache", None) is not None:
                tables.cache[l] = shared[toff[k]:toff[k] + m[k] * m[k]]
    return out


def prog_shared(backend, codes: Sequence[Sequence[np.ndarray]], budget_bytes: int = pa.DEFAULT_BUDGET_BYTES):
    """mprg_prog_distances over the loci (per locus its gap-free code arrays): per locus (s, nw): s an (m, m) int64 array whose
    part above the diagonal holds the shared 6-mers of the records a < b, nw the records' valid windows."""
    got = _prog_shared(backend, _pack(backend, codes), np.arange(len(codes)), budget_bytes)
    return [got[l] for l in range(len(codes))]


def prog_tree_words(m):
    """mprg_prog_tree's workspace need (int64 words) of a locus of m records."""
    return m * (m + 2)


def prog_tree_bytes(m):
    """What a locus of m records holds on the device while its tree is built: the m x m table of shared 6-mers and the workspace."""
    return 4 * m * m + 8 * prog_tree_words(m)


def prog_weights_words(m):
    """mprg_prog_leaf_weights' workspace need (int64 words) of a locus of m records."""
    return 6 * m


def _prog_trees(be, chunk: Chunk, sel, budget_bytes, weights=None, lw: Optional["_LeafWeights"] = None, tables=None):
    """The spec's Tree of the loci `sel` of a chunk on the device, in groups whose m x m tables and tree workspaces fit budget_bytes:
    per group one mprg_prog_distances launch and one mprg_prog_tree launch over the tables it left on the device; the status words
    and the merges are all that is downloaded.  Per locus its merges as prog_tree gives them.  weights: per record of the chunk's
    tables how many times it counts (the spec's Collapse).  The loci whose weight sum exceeds PROG_MAX_LEAVES (the spec's Large
    loci) form groups of their own, whose trees mprg_prog_tree_wide builds.  lw (the spec's Sequence weights): every group
    is followed by an mprg_prog_leaf_weights launch over the same tables and the merges where the tree launch left them.  tables:
    another source of the tables, called like _distances_launch (the spec's Pair distances)."""
    lens, first = chunk.lens, chunk.first
    out = {}
    d_seqs = be.upload(np.stack([chunk.seq_off, lens], 1).reshape(-1))
    d_weights = None if weights is None else be.upload(np.asarray(weights, np.int32))
    n_leaves = np.add.reduceat((lens > 0).astype(np.int64), first)
    # the spec's Large loci: a locus whose weight sum exceeds mprg_prog_tree's bound goes to mprg_prog_tree_wide, in groups (and so
    # in launches) of such loci alone; without one nothing launches differently
    for grp, entry, table in _tree_groups(chunk, sel, budget_bytes, weights):
        m, toff, words, d_shared, d_nw, d_status, n_work = (tables or _distances_launch)(be, chunk, d_seqs, grp)
        launched = _tree_launch(be, chunk, grp, entry, d_seqs, d_weights, n_leaves, toff, words, d_shared, d_nw)
        if lw is not None:
            lw.launch(grp, d_seqs, d_weights, toff, words, d_shared, d_nw, *launched[1:])
        _check(be.download(d_status, np.int32, n_work), "mprg_prog_distances", PG_STATUS)
        out.update(_tree_merges(be, grp, entry, table, *launched))
    return out


class _LeafWeights:
    """The spec's Sequence weights of a chunk on the device: q and raw per record of the chunk's tables, one pair of buffers for all
    launches; launch() is one mprg_prog_leaf_weights launch over a group's tables and merges where they are; q() downloads the
    status words of the launches and q, nothing else."""

    def __init__(self, be, chunk: Chunk):
        self.be, self.chunk, self.pending, self.groups, self.spent = be, chunk, [], [], 0.0
        self.n_leaves = np.add.reduceat((chunk.lens > 0).astype(np.int64), chunk.first)
        self.d_q, self.d_raw = be.zeros(4 * len(chunk.lens)), be.zeros(8 * len(chunk.lens))

    def launch(self, grp, d_seqs, d_weights, toff, words, d_shared, d_nw, d_merges, n_merges, moff):
        be, chunk = self.be, self.chunk
        t0 = time.perf_counter()
        m = chunk.counts[grp]
        ws_words = prog_weights_words(m)
        ttab = np.stack([chunk.first[grp], m, toff, exclusive_sum(ws_words), moff], 1).astype(np.int64)
        total = int(n_merges.sum())
        d_ttab, d_ws = be.upload(ttab), be.empty(8 * int(ws_words.sum()))
        d_heights, d_status = be.empty(4 * total), be.empty(4 * len(grp))
        be.call("mprg_prog_leaf_weights", be.ptr(d_shared), words, be.ptr(d_nw), be.ptr(d_seqs), len(chunk.lens), be.ptr(d_ttab), len(grp),
                0 if d_weights is None else be.ptr(d_weights), be.ptr(d_ws), int(ws_words.sum()), be.ptr(d_merges), 2 * total,
                be.ptr(d_heights), be.ptr(self.d_raw), be.ptr(self.d_q), be.ptr(d_status), be.stream,
                work=float((self.n_leaves[grp] ** 2).sum() * 8.0))
        self.pending.append((d_status, len(grp), d_heights))
        self.groups.append(grp.tolist())
        self.spent += time.perf_counter() - t0

    def upload_and_launch(self, grp, trees, d_seqs, d_weights, toff, words, d_shared, d_nw):
        """launch() for merges made on the host: trees[l], the merges of every locus of grp, uploaded."""
        n_merges = np.array([len(trees[l]) for l in grp.tolist()], np.int64)
        flat = np.array([p for l in grp.tolist() for p in trees[l]], np.int32).reshape(-1)
        self.launch(grp, d_seqs, d_weights, toff, words, d_shared, d_nw, self.be.upload(flat), n_merges, 2 * exclusive_sum(n_merges))

    def q(self) -> np.ndarray:
        t0 = time.perf_counter()
        for d_status, n, _ in self.pending:
            _check(self.be.download(d_status, np.int32, n), "mprg_prog_leaf_weights", WEIGHTS_STATUS, "locus")
        self.pending = []
        got = self.be.download(self.d_q, np.int32, len(self.chunk.lens)).astype(np.int64)
        self.spent += time.perf_counter() - t0
        return got


def _prog_weights(be, chunk: Chunk, sel, trees, budget_bytes, weights=None, tables=None, lw=None) -> "_LeafWeights":
    """The spec's Sequence weights of the loci `sel` whose trees were built on the host: in groups whose tables fit budget_bytes the
    distances launch again (the tables are not kept on the device, and never weighted on the host), the merges uploaded, one
    mprg_prog_leaf_weights launch.  tables: another source of the tables, called like _distances_launch (the spec's Pair distances);
    lw: the chunk's _LeafWeights when an earlier call made one."""
    lw = _LeafWeights(be, chunk) if lw is None else lw
    t0, before = time.perf_counter(), lw.spent
    d_seqs = be.upload(np.stack([chunk.seq_off, chunk.lens], 1).reshape(-1))
    d_weights = None if weights is None else be.upload(np.asarray(weights, np.int32))
    checks = []
    for lo, hi in pa.budget_groups(4 * chunk.counts[sel] ** 2 + 8 * prog_weights_words(chunk.counts[sel]), budget_bytes):
        grp = sel[lo:hi]
        m, toff, words, d_shared, d_nw, d_status, n_work = (tables or _distances_launch)(be, chunk, d_seqs, grp)
        lw.upload_and_launch(grp, trees, d_seqs, d_weights, toff, words, d_shared, d_nw)
        checks.append((d_status, n_work))
    for d_status, n_work in checks:
        _check(be.download(d_status, np.int32, n_work), "mprg_prog_distances", PG_STATUS)
    lw.spent = before + time.perf_counter() - t0                # (the distances launches are the stage's here)
    return lw


def prog_leaf_weights(backend, codes: Sequence[Sequence[np.ndarray]], merges: Sequence[Sequence[Tuple[int, int]]],
                      weights: Optional[Sequence[Sequence[int]]] = None, budget_bytes: int = pa.DEFAULT_BUDGET_BYTES):
    """mprg_prog_distances and mprg_prog_leaf_weights over the loci (per locus its gap-free code arrays; an empty one is no leaf) and
    their trees (per locus the merges in order as (key(U), key(V)), as prog_trees and prog_tree give them): per locus the spec's
    Sequence weights as (heights per merge, raw per record, q per record), what leaf_weights gives from D; a record that is no leaf
    has 0 in raw and q.  weights: per locus, per record, its multiplicity (the spec's Collapse)."""
    be = backend
    chunk = _pack(be, codes)
    flat = None if weights is None else np.concatenate([np.asarray(w, np.int64) for w in weights])
    lw = _prog_weights(be, chunk, np.arange(len(codes)), list(merges), budget_bytes, flat)
    heights = [be.download(d_heights, np.int32, sum(len(merges[l]) for l in grp)) for grp, d_heights in
               zip(lw.groups, [p[2] for p in lw.pending])]
    q = lw.q()
    raw = be.download(lw.d_raw, np.int64, len(chunk.lens))
    out = [None] * len(codes)
    for grp, h in zip(lw.groups, heights):
        at = 0
        for l in grp:
            rec = slice(int(chunk.first[l]), int(chunk.first[l] + chunk.counts[l]))
            out[l] = (h[at:at + len(merges[l])].astype(np.int64), raw[rec].copy(), q[rec].copy())
            at += len(merges[l])
    return out


def leaf_weights(D, leaves: Sequence[int], merges: Sequence[Tuple[int, int]], weights=None):
    """The spec's Sequence weights in Python integers: D[a][b] the distances the tree was built on, leaves (ascending indices into
    D), merges the tree as prog_tree gives it, weights per leaf its multiplicity (default 1).  Returns (heights per merge, raw per
    leaf, q per leaf)."""
    lv = [int(a) for a in leaves]
    mult = {a: 1 if weights is None else int(w) for a, w in zip(lv, lv if weights is None else weights)}
    live = {a: (None, [a], mult[a]) for a in lv}              # per key: its cluster's node (None: a leaf), leaves, multiplicity sum
    heights, par, lpar, below = [], {}, {}, {}
    for t, (u, v) in enumerate(merges):
        (nu, mu, su), (nv, mv, sv) = live[u], live.pop(v)
        heights.append(sum(mult[a] * mult[b] * int(D[a][b]) for a in mu for b in mv) // (su * sv))
        for key, node in ((u, nu), (v, nv)):
            if node is None:
                lpar[key] = t
            else:
                par[node] = t
        below[t] = su + sv
        live[u] = (t, mu + mv, su + sv)
    raw = []
    for a in lv:
        c, h, n, t = 0, 0, mult[a], lpar.get(a)
        while t is not None:
            c += (SEQ_WEIGHT_UNIT * max(heights[t] - h, 0) * mult[a]) // n
            h, n, t = heights[t], below[t], par.get(t)
        raw.append(c)
    top = max(raw, default=0)
    return heights, raw, [1 if top == 0 else 1 + ((SEQ_WEIGHT_UNIT - 1) * c) // top for c in raw]


def _tree_groups(chunk: Chunk, sel, budget_bytes, weights=None):
    """_prog_trees' groups of the loci `sel`: (the group's loci, the entry point that builds their trees, its status texts)."""
    n_leaves = np.add.reduceat((chunk.lens > 0).astype(np.int64), chunk.first)
    wsum = n_leaves if weights is None else np.add.reduceat(np.where(chunk.lens > 0, np.asarray(weights, np.int64), 0), chunk.first)
    wide = wsum[sel] > PROG_MAX_LEAVES
    return [(part[lo:hi], entry, table)
            for part, entry, table in ((sel[~wide], "mprg_prog_tree", TREE_STATUS), (sel[wide], "mprg_prog_tree_wide", WIDE_TREE_STATUS))
            if len(part) for lo, hi in pa.budget_groups(prog_tree_bytes(chunk.counts[part]), budget_bytes)]


def _tree_launch(be, chunk: Chunk, grp, entry, d_seqs, d_weights, n_leaves, toff, words, d_shared, d_nw):
    """One mprg_prog_tree(_wide) launch over the tables of the loci `grp` where a launch left them on the device: what
    _tree_merges downloads."""
    m = chunk.counts[grp]
    n_merges = np.maximum(n_leaves[grp] - 1, 0)
    moff = 2 * exclusive_sum(n_merges)
    ws_words = prog_tree_words(m)
    ttab = np.stack([chunk.first[grp], m, toff, exclusive_sum(ws_words), moff], 1).astype(np.int64)
    d_ttab, d_ws = be.upload(ttab), be.empty(8 * int(ws_words.sum()))
    d_merges, d_tstatus = be.empty(8 * int(n_merges.sum())), be.empty(4 * len(grp))
    be.call(entry, be.ptr(d_shared), words, be.ptr(d_nw), be.ptr(d_seqs), len(chunk.lens), be.ptr(d_ttab), len(grp),
            0 if d_weights is None else be.ptr(d_weights), be.ptr(d_ws), int(ws_words.sum()), be.ptr(d_merges), 2 * int(n_merges.sum()),
            be.ptr(d_tstatus), be.stream, work=float((m * m).sum() * 24.0))
    return d_tstatus, d_merges, n_merges, moff


def _tree_merges(be, grp, entry, table, d_tstatus, d_merges, n_merges, moff):
    """The status words and the merges of a _tree_launch, downloaded: per locus its merges as prog_tree gives them."""
    _check(be.download(d_tstatus, np.int32, len(grp)), entry, table, "locus")
    merges = be.download(d_merges, np.int32, 2 * int(n_merges.sum())).reshape(-1, 2)
    return {l: [tuple(p) for p in merges[moff[k] // 2:moff[k] // 2 + n_merges[k]].tolist()] for k, l in enumerate(grp.tolist())}


def prog_trees(backend, codes: Sequence[Sequence[np.ndarray]], weights: Optional[Sequence[Sequence[int]]] = None,
               budget_bytes: int = pa.DEFAULT_BUDGET_BYTES) -> List[List[Tuple[int, int]]]:
    """mprg_prog_distances and mprg_prog_tree over the loci (per locus its gap-free code arrays; an empty one is no leaf): per locus
    the spec's Tree as prog_tree gives it, the merges in order as (key(U), key(V)).  weights: per locus, per record, how many times
    it counts (the spec's Collapse); a locus whose weights add up to more than PROG_MAX_LEAVES, up to PROG_MAX_RECORDS, is built by
    mprg_prog_tree_wide (the spec's Large loci)."""
    chunk = _pack(backend, codes)
    flat = None if weights is None else np.concatenate([np.asarray(w, np.int64) for w in weights])
    got = _prog_trees(backend, chunk, np.arange(len(codes)), budget_bytes, flat)
    return [got[l] for l in range(len(codes))]


def prog_distance_matrix(shared: np.ndarray, nw: np.ndarray) -> np.ndarray:
    """The spec's D (symmetric, int64, zero diagonal) from what mprg_prog_distances gave for a locus."""
    s = np.triu(shared, 1)
    s = s + s.T
    m = np.minimum(nw[:, None], nw[None, :])
    D = np.where(m > 0, PROG_SCALE - (PROG_SCALE * s) // np.maximum(m, 1), PROG_SCALE).astype(np.int64)
    np.fill_diagonal(D, 0)
    return D


def prog_tree(D: np.ndarray, leaves: Sequence[int], weights=None) -> List[Tuple[int, int]]:
    """The spec's Tree over the leaves (ascending indices into D): the merges in order as (key(U), key(V)), key(U) < key(V); the
    merged cluster keeps key(U).  Exact: a float64 quotient only shortlists the pairs within 2^-40 of the smallest, the choice
    among them is made by cross-multiplication in Python integers, ties to the first in (key(U), key(V)) order.
    weights: per leaf how many times it counts (the spec's Collapse): the tree of the leaves written that often, one leaf each."""
    idx = np.asarray(leaves, np.int64)
    n = len(idx)
    S = D[np.ix_(idx, idx)].astype(np.int64)                    # sums of D between the clusters, slot = rank of the key
    size = np.ones(n, np.int64)
    alive = np.ones(n, bool)
    Q = np.full((n, n), np.inf)
    iu = np.triu_indices(n, 1)
    Q[iu] = S[iu]
    if weights is not None:                                     # S: sums of w_a w_b D(a, b); a cluster's size: its weight sum
        size = np.asarray(weights, np.int64).copy()            # (Q stays D: the quotient of w_a w_b D(a, b) by w_a w_b)
        # int64 up to the spec's Large loci: sum w <= 2^20, so w_a w_b <= 2^38 off the diagonal and 2^40 on it (where D = 0), an
        # entry w_a w_b D <= 2^54, a sum between two clusters <= 65 536 |U| |V| <= 2^54 and size[u] * size[v] <= 2^38; the cross
        # products (up to 2^92) are made in Python integers
        S = S * np.outer(size, size)
    merges = []
    for _ in range(n - 1):
        qmin = Q.min()
        cu, cv = np.nonzero(Q <= qmin * (1 + 2.0 ** -40))      # row-major: (key(U), key(V)) order
        u, v = int(cu[0]), int(cv[0])
        for a, b in zip(cu[1:].tolist(), cv[1:].tolist()):
            if int(S[a, b]) * int(size[u] * size[v]) < int(S[u, v]) * int(size[a] * size[b]):
                u, v = a, b
        merges.append((int(idx[u]), int(idx[v])))
        S[u, :] += S[v, :]
        S[:, u] = S[u, :]
        size[u] += size[v]
        alive[v] = False
        Q[v, :] = np.inf
        Q[:, v] = np.inf
        r = S[u] / (size[u] * size).astype(np.float64)
        r[~alive] = np.inf
        Q[u, u + 1:] = r[u + 1:]
        Q[:u, u] = r[:u]
    return merges


class Plan(NamedTuple):
    """What the spec's Tree decides for a chunk (_prog_plan): leaves: per locus the non-empty records; by_round: per round its merges
    (locus, y, x, parent), Y the child with more rows; root: per locus its root node; order: per locus the records of the root's
    rows in row order: Y's rows, then X's, at every node; trees: per locus the merges (key(U), key(V)) in the order UPGMA made
    them; progression: per locus the tuple (leaves, rounds, False)."""
    leaves: list
    by_round: dict
    root: list
    order: list
    trees: list
    progression: list


def _prog_plan(lens, first, counts, shared, weights=None, merges=None) -> Plan:
    """The Plan of a chunk, from its tables and _prog_shared's of the loci of three or more leaves (two leaves have one tree); no
    device, no clock.  A leaf's node id is its record index, an inner node's counts on from the locus's records.
    weights: per record of the tables how many rows it stands for (the spec's Collapse): the tree is the weighted one and Y the
    child with the larger weight sum.  merges: per locus of three or more leaves its tree as _prog_trees gave it; `shared` is then
    not read."""
    leaves, by_round, roots, root_members, trees, progression = [], {}, [], [], [], []
    for l in range(len(counts)):
        lv = np.nonzero(lens[first[l]:first[l] + counts[l]] > 0)[0].tolist()
        wl = None if weights is None else weights[first[l]:first[l] + counts[l]]
        tree = ([(lv[0], lv[1])] if len(lv) == 2 else [] if len(lv) < 2 else merges[l] if merges is not None else
                prog_tree(prog_distance_matrix(*shared[l]), lv, None if wl is None else wl[lv]))
        members = {a: [a] for a in lv}
        size = {a: 1 if wl is None else int(wl[a]) for a in lv}
        node_at, rnd, nxt = {a: a for a in lv}, {a: 0 for a in lv}, int(counts[l])
        for u, v in tree:
            a, b = node_at[u], node_at[v]                       # key(a) = u < v = key(b)
            y, x = (a, b) if size[a] >= size[b] else (b, a)
            members[nxt] = members.pop(y) + members.pop(x)
            size[nxt] = size.pop(y) + size.pop(x)
            rnd[nxt] = 1 + max(rnd[a], rnd[b])
            by_round.setdefault(rnd[nxt], []).append((l, y, x, nxt))
            node_at[u] = nxt
            nxt += 1
        leaves.append(lv)
        roots.append(node_at[lv[0]])
        root_members.append(members[roots[-1]])
        trees.append(tree)
        progression.append((len(lv), rnd[roots[-1]], False))
    return Plan(leaves, by_round, roots, root_members, trees, progression)


def _prog_w0(band):
    """Pass 1's half-width of the banded merges, or None: the full DP."""
    if band is None or band is False:
        return None
    w0 = PROG_BAND_W0 if band is True else int(band)
    if w0 < 0:
        raise StarAlignError("band: a negative half-width")
    return w0


class _Merge(NamedTuple):
    """How the merges of a stage run (Options.merge); counters: the dict that receives their counters, or None."""
    band: object = None
    budget_bytes: int = pa.DEFAULT_BUDGET_BYTES
    counters: Optional[dict] = None
    position_gaps: bool = False
    free_end_gaps: bool = False

    def group(self, be, texts: "_Texts", X, Y, weights=None, reuse=True) -> list:
        """One budget group of merges end to end: X, Y (n, 4) int64 {buffer, offset, R, W} of the two sides' texts in `texts`.  The
        table of the buffers uploaded, _prog_pairs, _prog_parents into a buffer of the group's own, which joins `texts` (reuse: in a
        dropped buffer's place if there is one).  Returns per merge the parent's (buffer, offset, rows, width); the caller places
        them.  weights: _prog_pairs'."""
        d_bufs, n_bufs = texts.table(be), len(texts.bufs)
        d_ops, ops_bytes, ops_off, count, _ = _prog_pairs(be, d_bufs, n_bufs, X, Y, self, weights)
        d_new, new_bytes, poff, R = _prog_parents(be, d_bufs, n_bufs, X, Y, d_ops, ops_bytes, ops_off, count)
        b = texts.add(d_new, new_bytes, reuse)
        return [(b, int(poff[i]), int(R[i]), int(count[i])) for i in range(len(X))]


def _prog_groups(WX, WY, merge: _Merge):
    """The merges (X's and Y's columns) longest first in groups whose workspace and column tables each fit the budget; with band
    the workspace is pass 1's (the full DP's for a merge its band does not help).  merge.position_gaps: Y's profile has 7 planes."""
    order = np.argsort(-((WX + 1) * WY), kind="stable")
    need, w0 = pa.workspace_words_v(WX, WY), _prog_w0(merge.band)
    if w0 is not None:
        dlo, dhi, helps = pa.band_first(WX, WY, w0)
        need = np.where(helps, pa.band_workspace_words(WX, WY, dlo, dhi), need)
    for grp, _, _ in pa.budget_launches(order, need, merge.budget_bytes, StarAlignError, "merge", WX, WY,
                                        also=7 * WX + (7 if merge.position_gaps else 6) * WY):
        yield grp


def _prog_pairs(be, d_bufs, n_bufs, X, Y, merge: _Merge = _Merge(), weights=None):
    """One group of merges on the device: X, Y (n, 4) int64 {buffer, offset, R, W} of the two sides' texts.  mprg_prog_columns (Y's
    profiles, X's column tables) and mprg_align_profile_pairs in one launch each; {status, score, op count} downloaded.  With
    merge.band the spec's two passes instead (the module docstring, host side), merge.counters receiving the prog_band_* counts.
    weights: (per merge the weights of X's rows, of Y's rows), the spec's Collapse: the column tables through
    mprg_prog_columns_weighted and R_X the weight sum; everything else is the same.
    merge.position_gaps (the spec's Position gaps): Y's profile gets its seventh plane (kind 2) and every call its _posgap form.
    merge.free_end_gaps (the spec's Free end gaps): the DP calls get their _endgap form (of either open) and the widths come from
    mprg_prog_band_widths_endgap (one entry for both opens); the column tables, the sizing and the groups are unchanged.
    Returns (the ops buffer, its bytes, each merge's ops offset, op count, score)."""
    band, budget_bytes, counters, position_gaps, free_end_gaps = merge
    n = len(X)
    WX, WY = X[:, 3], Y[:, 3]
    k = np.nonzero(WX + WY >= pa.MAX_LEN)[0]
    if len(k):
        raise StarAlignError(f"a merge of {WX[k[0]]} columns against {WY[k[0]]}: their sum must stay below {pa.MAX_LEN}")
    posgap, PY = ("_posgap", 7) if position_gaps else ("", 6)    # the calls' suffix, the planes of Y's profile
    ycol = exclusive_sum(PY * WY + 7 * WX)
    xcol = ycol + PY * WY
    words = int((PY * WY + 7 * WX).sum())
    items = np.zeros((2 * n, PG_ITEM_FIELDS if weights is None else PG_WITEM_FIELDS), np.int64)
    items[:n, :4], items[:n, 4], items[:n, 5] = Y, 2 if position_gaps else 0, ycol
    items[n:, :4], items[n:, 4], items[n:, 5] = X, 1, xcol
    work = _tile_work(items[:, 3])
    RX, columns = X[:, 2], "mprg_prog_columns" + posgap
    if weights is not None:
        per_item = list(weights[1]) + list(weights[0])          # Y's items, then X's
        flat = np.concatenate(per_item).astype(np.int32)
        items[:, 6], items[:, 7] = exclusive_sum(items[:, 2]), [int(w.sum()) for w in per_item]
        RX, columns = items[n:, 7], "mprg_prog_columns_weighted" + posgap
    d_items, d_work, d_cols, d_status = be.upload(items), be.upload(work), be.empty(4 * words), be.empty(4 * len(work))
    d_weights = None if weights is None else be.upload(flat)    # (the weighted entry takes the rows' weights in front of the tables)
    be.call(columns, be.ptr(d_bufs), n_bufs, be.ptr(d_items), len(items), be.ptr(d_work), len(work),
            *(() if weights is None else (be.ptr(d_weights), len(flat))), be.ptr(d_cols), words, be.ptr(d_status), be.stream,
            work=float((items[:, 2] * items[:, 3]).sum()))
    need = pa.workspace_words_v(WX, WY)
    ops_off = exclusive_sum(WX + WY)
    ops_bytes = int((WX + WY).sum())
    leaf_tab = np.stack([np.zeros(n, np.int64), Y[:, 2], WY, ycol], 1).astype(np.int64)
    d_leaves = be.upload(leaf_tab)
    d_ops = be.empty(ops_bytes)
    w0 = _prog_w0(band)
    endgap = "_endgap" if free_end_gaps else ""
    full, banded = "mprg_align_profile_pairs" + posgap + endgap, "mprg_align_profile_pairs" + posgap + endgap + "_banded"
    widths = "mprg_prog_band_widths" + (endgap or posgap)
    pending = []                                                # (merges, call, the launch's triples, its table): downloaded at the end

    def launches(call, idx, wordsv, dlo=None, dhi=None):
        """The merges idx (longest first) through `call` in launches that fit the workspace budget."""
        for sel, ws_off, used in pa.budget_launches(idx, wordsv, budget_bytes, StarAlignError, "merge", WX, WY):
            band_cols = () if dlo is None else (dlo[sel], dhi[sel])
            d_pairs = be.upload(np.stack([sel, xcol[sel], WX[sel], ws_off, ops_off[sel], RX[sel], *band_cols], 1).astype(np.int64))
            d_ws, d_out = be.empty(4 * used), be.empty(12 * len(sel))
            be.call(call, be.ptr(d_cols), be.ptr(d_leaves), n, be.ptr(d_cols), words, be.ptr(d_pairs), len(sel), be.ptr(d_ws), used,
                    be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream, work=pa.sweep_work(WX[sel], WY[sel], *band_cols))
            pending.append((sel, call, d_out, d_pairs))

    def pass1(first, dlo, dhi):
        # one launch where the group was sized by its need; the widths over the same table and its triples
        wstar = np.zeros(n, np.int64)
        launches(banded, first, pa.band_workspace_words(WX, WY, dlo, dhi), dlo, dhi)
        for sel, _, d_out, d_pairs in list(pending):
            d_got = be.empty(20 * len(sel))                     # {SB, w*} per merge, then the status words
            be.call(widths, be.ptr(d_cols), be.ptr(d_leaves), n, be.ptr(d_cols), words, be.ptr(d_pairs), len(sel),
                    be.ptr(d_out), be.ptr(d_got), be.ptr(d_got) + 16 * len(sel), be.stream, work=float((WX[sel] + WY[sel]).sum()))
            got = be.download(d_got, np.uint8, 20 * len(sel))
            status = got[16 * len(sel):].view(np.int32)
            if status.any():
                _check(be.download(d_status, np.int32, len(work)), columns, PG_STATUS)
                res = be.download(d_out, np.int32, 3 * len(sel)).reshape(-1, 3)
                code = int(res[res[:, 0] != 0][0, 0]) if res[:, 0].any() else int(status[status != 0][0])
                raise StarAlignError(f"{banded} / {widths}: {pa.STATUS.get(code, code)}")
            wstar[sel] = got[:16 * len(sel)].view(np.int64).reshape(-1, 2)[:, 1]
        return wstar, wstar
    if w0 is None:                                              # (one launch: _prog_groups sized the group by this need)
        launches(full, np.arange(n), need)
    else:
        second, rest, dlo, dhi, counts = pa.band_plan(WX, WY, w0, pass1)
        launches(banded, second, pa.band_workspace_words(WX, WY, dlo, dhi), dlo, dhi)
        launches(full, rest, need)
    _check(be.download(d_status, np.int32, len(work)), columns, PG_STATUS)
    count, score = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for sel, call, d_out, _ in pending:                          # in launch order: a later pass's result replaces pass 1's
        res = be.download(d_out, np.int32, 3 * len(sel)).reshape(-1, 3)
        bad = np.nonzero(res[:, 0])[0]
        if len(bad):
            raise StarAlignError(f"{call}: {pa.STATUS.get(int(res[bad[0], 0]), int(res[bad[0], 0]))}")
        score[sel], count[sel] = res[:, 1], res[:, 2]
    if position_gaps:
        add_to(counters, "position_gap_merges", n)
    if free_end_gaps:
        add_to(counters, "free_end_gap_merges", n)
    for key, v in zip(("prog_band_merges", "prog_band_second_passes", "prog_band_full_merges", "prog_band_cells", "prog_band_full_cells"),
                      () if w0 is None else counts):
        add_to(counters, key, int(v))
    return d_ops, ops_bytes, ops_off, count, score


def _bufs_table(be, bufs):
    """The {address, bytes} table of the text buffers (a dropped one: {0, 0}, no text fits it)."""
    return be.upload(np.array([[be.ptr(b), n] if b is not None else [0, 0] for b, n in bufs], np.int64))


class _Texts:
    """The texts of a chunk's nodes on the device and their lifetime: bufs[b] is (buffer, bytes) of text buffer b, 0 the chunk's
    code buffer (the leaves), (None, 0) a dropped one; where[locus, node] is (b, offset, rows, width) of a node not yet merged
    (behind the last round: of every locus its root, whose entry then names the locus's current text); live[b] counts the nodes
    of where in b.  A buffer (but 0) is dropped when nothing of where is in it."""

    def __init__(self, chunk: Chunk, leaves):
        lens, seq_off, first = chunk.lens, chunk.seq_off, chunk.first
        self.where = {(l, a): (0, int(seq_off[first[l] + a]), 1, int(lens[first[l] + a])) for l in range(chunk.n_loci) for a in leaves[l]}
        self.bufs, self.live = [(chunk.d_codes, chunk.codes_bytes)], [len(self.where)]

    def table(self, be):
        return _bufs_table(be, self.bufs)

    def add(self, buf, nbytes, reuse=True) -> int:
        """The buffer's index in bufs: with reuse a dropped buffer's place if there is one (the rounds number theirs as they come)."""
        b = next((i for i in range(1, len(self.bufs)) if self.bufs[i][0] is None), len(self.bufs)) if reuse else len(self.bufs)
        if b == len(self.bufs):
            self.bufs.append(None)
            self.live.append(0)
        self.bufs[b], self.live[b] = (buf, nbytes), 0
        return b

    def place(self, locus, node, text):
        """The node's text is `text` (b, offset, rows, width) from now on, in place of the one it had."""
        if (locus, node) in self.where:
            self.live[self.where[locus, node][0]] -= 1
        self.where[locus, node] = text
        self.live[text[0]] += 1

    def merged(self, locus, node):
        """The node has gone into its parent: its buffer goes with its last node."""
        b = self.where.pop((locus, node))[0]
        self.live[b] -= 1
        self.drop_unused([b])

    def drop_unused(self, bs):
        for b in bs:
            if b and not self.live[b]:
                self.bufs[b] = (None, 0)


def merge_profiles(backend, pairs: Sequence[Tuple[np.ndarray, np.ndarray]], budget_bytes: int = pa.DEFAULT_BUDGET_BYTES, band=None,
                   counters: Optional[dict] = None, position_gaps: bool = False, free_end_gaps: bool = False):
    """mprg_align_profile_pairs on (X, Y) pairs of cell-code matrices (R_X x W_X, R_Y x W_Y), through the launches a round of
    merges makes: per pair (ops as bytes over b"MID" in forward order, score).  band (True: PROG_BAND_W0, or pass 1's half-width):
    the spec's banded two passes, the same results; counters then receives the prog_band_* counts (added up).  position_gaps:
    the spec's Position gaps (mprg_align_profile_pairs_posgap and the other _posgap entries); free_end_gaps: the spec's Free end
    gaps (the _endgap entries)."""
    be = backend
    mats = [m for xy in pairs for m in xy]
    off = np.concatenate([[0], np.cumsum([m.size for m in mats])]).astype(np.int64)
    text = np.concatenate([np.ascontiguousarray(m, np.uint8).reshape(-1) for m in mats])
    bufs = [(be.upload(text), len(text))]
    d_bufs = _bufs_table(be, bufs)
    X = np.array([[0, off[2 * k], *pairs[k][0].shape] for k in range(len(pairs))], np.int64).reshape(-1, 4)
    Y = np.array([[0, off[2 * k + 1], *pairs[k][1].shape] for k in range(len(pairs))], np.int64).reshape(-1, 4)
    out = [None] * len(pairs)
    merge = _Merge(band, budget_bytes, counters, position_gaps, free_end_gaps)
    for grp in _prog_groups(X[:, 3], Y[:, 3], merge):
        d_ops, ops_bytes, ops_off, count, score = _prog_pairs(be, d_bufs, 1, X[grp], Y[grp], merge)
        ops = be.download(d_ops, np.uint8, ops_bytes)
        for i, k in enumerate(grp.tolist()):
            out[k] = (ops[ops_off[i]:ops_off[i] + count[i]][::-1].tobytes(), int(score[i]))
    return out


def _pair_dist_how(chunk: Chunk, n_leaves, cap: int) -> list:
    """The spec's Pair distances, Which loci: per locus of the chunk "pairs", "cap" (more leaves than the cap), "limit" (a pair with
    n + C >= 10^6: the two longest leaves decide) or None (fewer than 3 leaves)."""
    how = []
    for l in range(chunk.n_loci):
        ln = np.sort(chunk.lens[chunk.first[l]:chunk.first[l] + chunk.counts[l]])
        how.append(None if n_leaves[l] < PAIR_DIST_MIN_LEAVES else "cap" if n_leaves[l] > cap else
                   "limit" if int(ln[-1] + ln[-2]) >= pa.MAX_LEN else "pairs")
    return how


def _pair_dist_report(counters, reports: Reports, how, n_leaves, spent, band=None):
    """The spec's Pair distances in the counters and in the caller's list: per locus (leaves, pairs run, how)."""
    add_to(counters, "pair_dist_s", float(spent))
    for key in ("pair_dist_pairs", "pair_dist_cells") + (("pair_dist_second_passes", "pair_dist_full_pairs") if band is not None else ()):
        add_to(counters, key, 0)
    for key, word in (("pair_dist_loci", "pairs"), ("pair_dist_above_cap", "cap"), ("pair_dist_limit", "limit")):
        add_to(counters, key, sum(1 for h in how if h == word))
    reports.add("pair_distancing", ((int(n), int(n) * (int(n) - 1) // 2 if h == "pairs" else 0, h) for n, h in zip(n_leaves, how)))


def _seq_weight_counters(counters, n_loci, q, spent):
    """The spec's Sequence weights in the counters: the loci weighted, the smallest q of any leaf, the stage's wall seconds."""
    add_to(counters, "seq_weight_loci", int(n_loci))
    add_to(counters, "seq_weight_s", float(spent))
    if counters is not None and len(q):
        counters["seq_weight_min_q"] = min(int(counters.get("seq_weight_min_q", SEQ_WEIGHT_UNIT)), int(q.min()))


def _progressive(be, chunk: Chunk, opts: Options, laps: _Laps, reports: Reports, classes: Optional[Classes] = None):
    """The spec's Progressive over one chunk, on the (oriented) sequences in chunk.d_codes.  Returns what the star pass leaves: the
    device buffer of the MSAs' ASCII text, its bytes, each locus's offset in it and its width.  classes: the spec's Collapse: the
    tree and the merges over the representatives with their weights, the root's rows written for every member.  Of opts:
    device_tree: the trees by mprg_prog_tree (_prog_trees) instead of prog_tree; pair_dist: their tables from the pair scores;
    seq_weights: q per leaf from the trees, after the plan, as the rows' weights in every merge; retree, then refine_tree, on the
    roots' texts before they are written out (progression then reports the trees that built the texts that are written);
    position_gaps and free_end_gaps in every merge of these three stages (the pair DPs of pair_dist keep the fixed open; their
    ends are free with free_end_distances alone)."""
    laps.lap()
    budget_bytes, band, device_tree, seq_weights, pair_dist = opts.budget_bytes, opts.band, opts.device_tree, opts.seq_weights, opts.pair_dist
    lens, first, counts = chunk.lens, chunk.first, chunk.counts
    acgt = _acgt(chunk) if pair_dist is not None else None
    n_leaves = np.add.reduceat((lens > 0).astype(np.int64), first)          # (every locus has a record)
    for l in np.nonzero(n_leaves == 0)[0]:
        raise StarAlignError(f"locus {chunk.names[l]}: every sequence is empty")
    weights = expand = None
    if classes is not None:
        # the chunk's tables with the representatives only (an empty record is one): what the distances, the tree and the rounds see
        keep = np.nonzero(classes.weight > 0)[0]
        kept = np.add.reduceat((classes.weight > 0).astype(np.int64), first)
        slot = np.cumsum(classes.weight > 0) - 1                # a representative's index in those tables
        expand = (counts, first, slot[classes.rep])
        chunk = chunk._replace(lens=lens[keep], seq_off=chunk.seq_off[keep], first=exclusive_sum(kept), counts=kept)
        lens, first, counts, weights = chunk.lens, chunk.first, chunk.counts, classes.weight[keep]
        acgt = None if acgt is None else acgt[keep]
        n_leaves = np.add.reduceat((lens > 0).astype(np.int64), first)
    # the trees: distances on the device for the loci with three or more leaves (two leaves have one tree), UPGMA on the host or,
    # with device_tree, on the device
    sel = np.nonzero(n_leaves >= 3)[0]
    # the spec's Pair distances: the loci of `sel` within the cap and the DP's limit take their tables from the pair scores, the
    # others (and every locus without the flag) from the 6-mer counts; parts: (loci, the source of their tables)
    parts = [(sel, None)]
    if pair_dist is not None:
        how = _pair_dist_how(chunk, n_leaves, int(pair_dist))
        by_pairs = np.array([how[l] == "pairs" for l in sel.tolist()], bool)
        pair_tables = _PairTables(band, laps.timings, acgt, budget_bytes, keep=seq_weights and not device_tree,
                                  free_ends=opts.free_end_distances)
        parts = [(sel[~by_pairs], None), (sel[by_pairs], pair_tables)]
    lw = _LeafWeights(be, chunk) if seq_weights and device_tree and len(sel) else None
    if device_tree:
        merges = {}
        for part, tables in parts:
            if len(part):
                merges.update(_prog_trees(be, chunk, part, budget_bytes, weights, lw, tables))
        add_to(laps.timings, "tree_device_loci", len(sel))
        t0 = time.perf_counter()
        plan = _prog_plan(lens, first, counts, None, weights, merges)
    else:
        shared = {}
        for part, tables in parts:
            if len(part):
                shared.update(_prog_shared(be, chunk, part, budget_bytes, tables))
        t0 = time.perf_counter()
        plan = _prog_plan(lens, first, counts, shared, weights)
    add_to(laps.timings, "tree_plan_s", time.perf_counter() - t0)
    laps.lap("tree_s")
    # the spec's Sequence weights: q per leaf of the loci that have a tree (fewer than three leaves need none: their q are equal)
    align = None
    if seq_weights:
        align = np.ones(len(lens), np.int64)
        if len(sel):
            for part, tables in () if device_tree else parts:
                if len(part):
                    lw = _prog_weights(be, chunk, part, plan.trees, budget_bytes, weights, tables, lw)
            rec = _ranges(first[sel], counts[sel])
            align[rec] = np.maximum(lw.q()[rec], 1)            # (an empty record has no row: its entry is never read)
            _seq_weight_counters(laps.timings, len(sel), align[rec][lens[rec] > 0], lw.spent)
        laps.lap("tree_s")
    if pair_dist is not None:
        _pair_dist_report(laps.timings, reports, how, n_leaves, pair_tables.spent, band)
    texts = _prog_rounds(be, chunk, plan, opts.merge(laps.timings), weights, align=align)
    laps.lap("progressive_s")
    if opts.retree:
        plan, result = _retree(be, chunk, plan, texts, weights, opts, laps.timings, align)
        reports.add("retreeing", result)
        laps.lap("retree_s")
    reports.add("progression", plan.progression)
    order = plan.order
    if opts.refine_tree:
        order, result = _tree_refine(be, chunk, plan, texts, weights, opts, laps.timings, align)
        reports.add("tree_refinement", result)
        laps.lap("tree_refine_s")
    text = _prog_output(be, chunk, plan.root, order, texts, expand)
    laps.lap("progressive_s")
    return text


def _prog_parents(be, d_bufs, n_bufs, Xg, Yg, d_ops, ops_bytes, ops_off, count):
    """The texts of a group of merges (Xg, Yg: the sides' {buffer, offset, R, W}; the ops as _prog_pairs left them) into a new
    buffer, one mprg_prog_rows launch: Y's rows, then X's, each through the merge's ops.  Returns (the buffer, its bytes, each
    parent's offset in it, its rows; its width is the op count)."""
    RY, RX = Yg[:, 2], Xg[:, 2]
    R = RY + RX
    poff = exclusive_sum(R * count)
    new_bytes = int((R * count).sum())
    rows = np.zeros((int(R.sum()), PG_ROW_FIELDS), np.int64)
    of = np.repeat(np.arange(len(R)), R)
    rank = np.arange(len(rows)) - np.repeat(exclusive_sum(R), R)
    is_x = rank >= RY[of]
    src = np.where(is_x[:, None], Xg[of], Yg[of])
    rows[:, 0] = src[:, 0]
    rows[:, 1] = src[:, 1] + (rank - np.where(is_x, RY[of], 0)) * src[:, 3]
    rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = src[:, 3], ops_off[of], count[of], is_x
    rows[:, 6], rows[:, 7] = poff[of] + rank * count[of], count[of]
    d_rows, d_new, d_status = be.upload(rows), be.empty(new_bytes), be.empty(4 * len(rows))
    be.call("mprg_prog_rows", be.ptr(d_bufs), n_bufs, be.ptr(d_ops), ops_bytes, be.ptr(d_rows), len(rows), be.ptr(d_new), new_bytes,
            0, be.ptr(d_status), be.stream, work=float(2 * new_bytes))
    _check(be.download(d_status, np.int32, len(rows)), "mprg_prog_rows", PG_STATUS)
    return d_new, new_bytes, poff, R


def _prog_rounds(be, chunk: Chunk, plan: Plan, merge: _Merge, weights=None, beyond=None, align=None) -> _Texts:
    """_progressive's device part: the plan's rounds (every node of a round, over all loci of the chunk, in one set of launches
    per budget group, _Merge.group).  Returns the texts as the last round left them: of every locus only its root is in where.
    A group's parents go into a buffer of their own; a buffer (but 0) is dropped when its last node has been merged into a parent.
    weights (the spec's Collapse): the chunk's tables hold the representatives only, weights per record of them; rw[locus, node]
    then is the weights of the node's rows.
    beyond (the spec's Retree): a set that receives the loci with a merge beyond Tree refinement's Limit (_tree_step_fits) instead
    of an error: such a locus takes no further merge and none of its nodes stays in where.
    align (the spec's Sequence weights): per record of the chunk's tables the weight q its row has in a merge, in place of the
    multiplicities, which keep their role in the plan."""
    first, n_loci = chunk.first, chunk.n_loci
    texts = _Texts(chunk, plan.leaves)
    where = texts.where
    row_w = weights if align is None else align
    rw = {} if row_w is None else {(l, a): row_w[first[l] + a:first[l] + a + 1] for l in range(n_loci) for a in plan.leaves[l]}
    for _, todo in sorted(plan.by_round.items()):
        if beyond is not None:
            todo = [t for t in todo if t[0] not in beyond]
            fits = _tree_step_fits(np.array([where[l, x][3] for l, _, x, _ in todo], np.int64),
                                   np.array([where[l, y][3] for l, y, _, _ in todo], np.int64), max(64, int(merge.budget_bytes) // 4))
            beyond.update(t[0] for t, ok in zip(todo, fits.tolist()) if not ok)
            for key in [key for key in where if key[0] in beyond]:
                texts.merged(*key)
            todo = [t for t in todo if t[0] not in beyond]
            if not todo:
                continue
        Y = np.array([where[l, y] for l, y, _, _ in todo], np.int64)
        X = np.array([where[l, x] for l, _, x, _ in todo], np.int64)
        for grp in _prog_groups(X[:, 3], Y[:, 3], merge):
            wg = None
            if row_w is not None:
                wg = ([rw[todo[k][0], todo[k][2]] for k in grp.tolist()], [rw[todo[k][0], todo[k][1]] for k in grp.tolist()])
            if weights is not None:
                add_to(merge.counters, "collapse_merges", len(grp))
            for k, parent_text in zip(grp.tolist(), merge.group(be, texts, X[grp], Y[grp], wg, reuse=False)):
                l, y, x, parent = todo[k]
                texts.place(l, parent, parent_text)
                if row_w is not None:
                    rw[l, parent] = np.concatenate([rw.pop((l, y)), rw.pop((l, x))])
                texts.merged(l, y)
                texts.merged(l, x)
    return texts


def _prog_output(be, chunk: Chunk, root, root_members, texts: _Texts, expand=None):
    """The roots' rows into input order, as ASCII; an empty record is a row of '-': one more mprg_prog_rows launch.  root_members:
    per locus the records of the root's rows, in row order.  expand (the spec's Collapse): (records per locus, each locus's first
    record, per record its representative's index in the chunk's tables) of the output: every record gets its representative's
    row.  Returns what the star pass leaves: (the buffer, its bytes, each locus's offset in it, its width)."""
    first, counts, n_loci, where = chunk.first, chunk.counts, chunk.n_loci, texts.where
    W = np.array([where[l, root[l]][3] for l in range(n_loci)], np.int64)
    o_counts, o_first, slot = (counts, first, None) if expand is None else expand
    base = exclusive_sum(o_counts * W)
    out_bytes = int((o_counts * W).sum())
    rows = np.zeros((int(o_counts.sum()), PG_ROW_FIELDS), np.int64)
    rows[:, 4] = -1
    rows[:, 6] = np.repeat(base, o_counts) + (np.arange(len(rows)) - np.repeat(o_first, o_counts)) * np.repeat(W, o_counts)
    rows[:, 7] = np.repeat(W, o_counts)
    for l in range(n_loci):
        b, off, _, w = where[l, root[l]]
        rec = first[l] + np.array(root_members[l], np.int64)
        at = np.arange(len(rec))
        if slot is not None:                                    # every record whose representative has a row of the root: that row
            at_of = np.full(int(counts[l]), -1, np.int64)
            at_of[root_members[l]] = at
            rec = np.arange(o_first[l], o_first[l] + o_counts[l])
            at = at_of[slot[rec] - first[l]]
            rec, at = rec[at >= 0], at[at >= 0]
        rows[rec, 0], rows[rec, 1], rows[rec, 2] = b, off + at * w, w
    d_bufs = texts.table(be)
    d_rows, d_out, d_status = be.upload(rows), be.empty(max(out_bytes, 1)), be.empty(4 * len(rows))
    be.call("mprg_prog_rows", be.ptr(d_bufs), len(texts.bufs), be.ptr(d_out), 0, be.ptr(d_rows), len(rows), be.ptr(d_out), max(out_bytes, 1), 1,
            be.ptr(d_status), be.stream, work=float(2 * out_bytes))
    _check(be.download(d_status, np.int32, len(rows)), "mprg_prog_rows", PG_STATUS)
    return d_out, out_bytes, base, W


# ---- retree
def _identities_launch(be, d_bufs, n_bufs: int, texts: np.ndarray, leaf: Sequence[np.ndarray], first: np.ndarray, m: np.ndarray, n_seqs: int):
    """One mprg_prog_identities launch: texts (n, 4) int64 {buffer, offset, R, W}, per text the record of each of its rows (an index
    within its locus), per text its locus's first sequence and sequence count m.  The tables are laid out as _distances_launch lays
    them out.  Returns (each table's offset, the tables' words, the tables, nw and the status words on the device, the work items)."""
    n = len(texts)
    R = texts[:, 2]
    toff, words = exclusive_sum(m * m), int((m * m).sum())
    items = np.stack([texts[:, 0], texts[:, 1], R, texts[:, 3], exclusive_sum(R), first, m, toff], 1).astype(np.int64)
    blocks = -(-R // PI_BLOCK_ROWS)
    work = np.stack([np.repeat(np.arange(n), blocks), _ranges(np.zeros(n, np.int64), blocks)], 1).astype(np.int32)
    flat = np.concatenate(leaf).astype(np.int32)
    d_items, d_work, d_leaf = be.upload(items), be.upload(work), be.upload(flat)
    d_shared, d_nw, d_status = be.zeros(4 * words), be.zeros(8 * n_seqs), be.empty(4 * len(work))
    be.call("mprg_prog_identities", be.ptr(d_bufs), n_bufs, be.ptr(d_items), n, be.ptr(d_work), len(work), be.ptr(d_leaf), len(flat),
            be.ptr(d_shared), words, be.ptr(d_nw), n_seqs, be.ptr(d_status), be.stream, work=float((R * R * texts[:, 3]).sum() / 2.0))
    return toff, words, d_shared, d_nw, d_status, len(work)


def prog_identities(backend, texts: Sequence[np.ndarray], leaf: Optional[Sequence[Sequence[int]]] = None, m: Optional[Sequence[int]] = None):
    """mprg_prog_identities on texts (per item an R x W matrix of cell codes), one launch: per item (s, nw): s an (m, m) int64 array
    whose part above the diagonal holds s' of the records a < b, nw the records' nw' (the spec's Retree, Distance).  leaf: per item
    the record of each row (default: row r is record r); m: per item its locus's records (default: R).  What no row stands for is 0."""
    be = backend
    mats = [np.ascontiguousarray(t, np.uint8) for t in texts]
    off = exclusive_sum(np.array([t.size for t in mats], np.int64))
    flat = np.concatenate([t.reshape(-1) for t in mats])
    tab = np.array([[0, off[k], *t.shape] for k, t in enumerate(mats)], np.int64).reshape(-1, 4)
    leaf = [np.arange(len(t)) for t in mats] if leaf is None else [np.asarray(x, np.int64) for x in leaf]
    m = np.array([len(t) for t in mats] if m is None else m, np.int64)
    first = exclusive_sum(m)
    d_text = be.upload(flat)
    toff, words, d_shared, d_nw, d_status, n_work = _identities_launch(be, _bufs_table(be, [(d_text, len(flat))]), 1, tab, leaf, first, m, int(m.sum()))
    _check(be.download(d_status, np.int32, n_work), "mprg_prog_identities", PG_STATUS)
    shared, nw = be.download(d_shared, np.uint32, words).astype(np.int64), be.download(d_nw, np.int64, int(m.sum()))
    return [(shared[toff[k]:toff[k] + m[k] * m[k]].reshape(int(m[k]), int(m[k])), nw[first[k]:first[k] + m[k]]) for k in range(len(mats))]


def _retree_trees(be, chunk: Chunk, sel, texts, order, bufs, weights, budget_bytes, on_device, lw=None):
    """The spec's Retree, Distance and Tree, for the loci `sel` of a chunk: texts[l] {buffer, offset, R, W} is the locus's current
    MSA, order[l] the records of its rows.  In _prog_trees' groups: one mprg_prog_identities launch, then with on_device the tree
    launch over the tables where they are (the merges and the status words come back), without it the tables downloaded and
    prog_tree on the host.  Per locus its merges as prog_tree gives them.  lw (a _LeafWeights; the spec's Sequence
    weights): every group's trees (uploaded, where the host built them) go through mprg_prog_leaf_weights over the group's
    identity tables, which are still on the device."""
    lens, first, counts = chunk.lens, chunk.first, chunk.counts
    out = {}
    n_leaves = np.add.reduceat((lens > 0).astype(np.int64), first)
    tables_stay = on_device or lw is not None
    d_seqs = be.upload(np.stack([chunk.seq_off, lens], 1).reshape(-1)) if tables_stay else None
    d_weights = None if weights is None or not tables_stay else be.upload(np.asarray(weights, np.int32))
    for grp, entry, table in _tree_groups(chunk, sel, budget_bytes, weights if on_device else None):
        loci = grp.tolist()
        toff, words, d_shared, d_nw, d_status, n_work = _identities_launch(
            be, _bufs_table(be, bufs), len(bufs), np.array([texts[l] for l in loci], np.int64), [order[l] for l in loci], first[grp], counts[grp],
            len(lens))
        if on_device:
            launched = _tree_launch(be, chunk, grp, entry, d_seqs, d_weights, n_leaves, toff, words, d_shared, d_nw)
            if lw is not None:
                lw.launch(grp, d_seqs, d_weights, toff, words, d_shared, d_nw, *launched[1:])
            _check(be.download(d_status, np.int32, n_work), "mprg_prog_identities", PG_STATUS)
            out.update(_tree_merges(be, grp, entry, table, *launched))
            continue
        _check(be.download(d_status, np.int32, n_work), "mprg_prog_identities", PG_STATUS)
        shared = be.download(d_shared, np.uint32, words).astype(np.int64)
        nw = be.download(d_nw, np.int64, len(lens))
        for k, l in enumerate(loci):
            mk, rec = int(counts[l]), slice(first[l], first[l] + counts[l])
            lv = np.nonzero(lens[rec] > 0)[0]
            out[l] = prog_tree(prog_distance_matrix(shared[toff[k]:toff[k] + mk * mk].reshape(mk, mk), nw[rec]), lv,
                               None if weights is None else weights[rec][lv])
        if lw is not None:
            lw.upload_and_launch(grp, out, d_seqs, d_weights, toff, words, d_shared, d_nw)
    return out


def _retree(be, chunk: Chunk, plan: Plan, texts: _Texts, weights, opts: Options, counters, align=None):
    """The spec's Retree over one chunk, on the roots' texts as _prog_rounds left them (texts, kept up here as _tree_refine keeps
    them up), opts.retree times.  Per iteration all loci that are still iterating go together: the identities and the trees
    (_retree_trees), _prog_plan and _prog_rounds for the loci whose tree changed, from the leaves, into buffers of their own, one
    objective launch, S downloaded; the text that loses goes with its buffer.  Returns (the plan with the accepted trees, their
    row orders and progression tuples in place of the first ones, per locus (iterations, accepted, why it stopped, S before, S
    after)).  align (the spec's Sequence weights): per record its q; a rebuild runs with the q of the rebuilt tree on D', and an
    accepted locus's entries of align are replaced by them, in place."""
    lens, first, counts, n_loci = chunk.lens, chunk.first, chunk.counts, chunk.n_loci
    leaves, root, where = plan.leaves, plan.root, texts.where
    order, trees, progression = [np.array(x, np.int64) for x in plan.order], list(plan.trees), list(plan.progression)
    wl, empty, in_bound, S = _root_objectives(be, chunk, plan, order, texts, weights)
    add_to(counters, "retree_over_bound", int((~in_bound).sum()))
    out = [[0, 0, None if in_bound[l] else "bound", int(S[l]), int(S[l])] for l in range(n_loci)]
    active = [l for l in np.nonzero(in_bound)[0].tolist() if len(leaves[l]) >= 3]
    add_to(counters, "retree_loci", len(active))
    for _ in range(opts.retree):
        if not active:
            break
        lw = None if align is None else _LeafWeights(be, chunk)
        merges = _retree_trees(be, chunk, np.array(active, np.int64), {l: where[l, root[l]] for l in active}, order, texts.bufs, weights,
                               opts.budget_bytes, opts.device_tree, lw)
        align2 = None
        if lw is not None:                                      # every active locus's q on the tree just built
            align2, rec = align.copy(), _ranges(first[active], counts[active])
            align2[rec] = np.maximum(lw.q()[rec], 1)
            _seq_weight_counters(counters, 0, align2[rec][lens[rec] > 0], lw.spent)
        for l in active:
            out[l][0] += 1
            if merges[l] == trees[l]:                           # a rebuild would reproduce the bytes
                out[l][2] = "same"
        todo = [l for l in active if out[l][2] is None]
        add_to(counters, "retree_same_tree", len(active) - len(todo))
        add_to(counters, "retree_rebuilds", len(todo))
        active = []
        if not todo:
            break
        # the rebuild: the changed loci as a chunk of their own over the same tables, from the leaves in buffer 0
        part = chunk._replace(first=first[todo], counts=counts[todo])
        plan2 = _prog_plan(lens, part.first, part.counts, None, weights, [merges[l] for l in todo])
        beyond = set()
        texts2 = _prog_rounds(be, part, plan2, opts.merge(counters), weights, beyond, align2)
        made, new = {}, {}
        for k, l in enumerate(todo):
            if k in beyond:
                out[l][2] = "limit"
                continue
            b, off, R, W = texts2.where[k, plan2.root[k]]
            if b not in made:
                made[b] = texts.add(*texts2.bufs[b])
            new[l] = (made[b], off, R, W, k)
        ks = sorted(new)
        S2 = (tree_objective(be, texts.table(be), len(texts.bufs), np.array([new[l][:4] for l in ks], np.int64),
                             [wl[l][np.array(plan2.order[new[l][4]], np.int64)] for l in ks], empty[ks]) if ks else [])
        used = list(made.values())
        for l, s2 in zip(ks, S2):
            k = new[l][4]
            if int(s2) > out[l][4]:                             # accepted: the locus's text is the new one, its tree the new tree
                used.append(where[l, root[l]][0])
                texts.place(l, root[l], new[l][:4])
                order[l], trees[l], progression[l] = np.array(plan2.order[k], np.int64), merges[l], plan2.progression[k]
                out[l][1], out[l][4] = out[l][1] + 1, int(s2)
                if align is not None:
                    align[first[l]:first[l] + counts[l]] = align2[first[l]:first[l] + counts[l]]
                active.append(l)
            else:
                out[l][2] = "refused"
        texts.drop_unused(used)
    add_to(counters, "retree_accepted", sum(o[1] for o in out))
    add_to(counters, "retree_refused", sum(o[2] == "refused" for o in out))
    return plan._replace(order=[o.tolist() for o in order], trees=trees, progression=progression), [tuple(o) for o in out]


# ---- tree refinement
def tree_steps(merges: Sequence[Tuple[int, int]]) -> List[np.ndarray]:
    """The spec's Steps of a tree given as prog_tree's merges: per step G = L_t, the leaves under node t (ascending)."""
    m = len(merges) + 1
    at, under, kids = {}, [], []
    for t, (u, v) in enumerate(merges):
        a, b = at.get(u, -1), at.get(v, -1)                      # (-1: a leaf)
        kids.append((a, b))
        under.append((under[a] if a >= 0 else [u]) + (under[b] if b >= 0 else [v]))
        at[u] = t
    twin = min(kids[-1]) if m >= 3 and min(kids[-1]) >= 0 else -1     # both children of the root are inner nodes: one split
    return [np.array(sorted(under[t]), np.int64) for t in range(m - 2) if m - len(under[t]) >= 2 and t != twin]


def tree_split(be, d_bufs, n_bufs: int, texts: np.ndarray, sides: Sequence[np.ndarray]):
    """mprg_tree_split: texts (n, 4) int64 {buffer, offset, R, W}, per text its side bytes (0: Y, 1: X).  One launch into a new
    buffer, the widths and the status words downloaded: (the buffer, its bytes, each item's offset in it, the widths (n, 2):
    W_Y, W_X).  Y's text is at the item's offset, X's R_Y W_Y bytes behind it."""
    n = len(texts)
    R, W = texts[:, 2], texts[:, 3]
    tiles = -(-W // 256) + 1
    ooff, out_bytes, n_cols, n_tiles = exclusive_sum(R * W), int((R * W).sum()), int(W.sum()), int(tiles.sum())
    items = np.stack([texts[:, 0], texts[:, 1], R, W, exclusive_sum(R), ooff, exclusive_sum(W), exclusive_sum(tiles)], 1).astype(np.int64)
    work = _tile_work(W)
    flat = np.concatenate(sides).astype(np.uint8)
    d_items, d_work, d_sides = be.upload(items), be.upload(work), be.upload(flat)
    d_flags, d_tiles, d_out, d_got = be.empty(n_cols), be.empty(8 * n_tiles), be.empty(out_bytes), be.empty(20 * n)
    be.call("mprg_tree_split", be.ptr(d_bufs), n_bufs, be.ptr(d_items), n, be.ptr(d_work), len(work), be.ptr(d_sides), len(flat),
            be.ptr(d_flags), n_cols, be.ptr(d_tiles), n_tiles, be.ptr(d_out), out_bytes, be.ptr(d_got), be.ptr(d_got) + 16 * n, be.stream,
            work=float(3 * out_bytes))
    got = be.download(d_got, np.uint8, 20 * n)                  # {W_Y, W_X} per item, then the status words
    _check(got[16 * n:].view(np.int32), "mprg_tree_split", PG_STATUS)
    return d_out, out_bytes, ooff, got[:16 * n].view(np.int64).reshape(-1, 2).copy()


def tree_objective(be, d_bufs, n_bufs: int, texts: np.ndarray, weights: Sequence[np.ndarray], empty: np.ndarray) -> np.ndarray:
    """mprg_tree_objective: the spec's Objective of texts (n, 4) int64 {buffer, offset, R, W} whose rows count weights[k][r] times,
    with empty[k] all-gap rows more; one launch, S per text downloaded."""
    n = len(texts)
    flat = np.concatenate(weights).astype(np.int32)
    items = np.zeros((n, TS_OBJ_FIELDS), np.int64)
    items[:, :4], items[:, 4], items[:, 5], items[:, 6] = texts, exclusive_sum(texts[:, 2]), [int(w.sum()) for w in weights], empty
    work = _tile_work(items[:, 3])
    d_items, d_work, d_weights = be.upload(items), be.upload(work), be.upload(flat)
    d_sums, d_status = be.zeros(8 * n), be.empty(4 * len(work))
    be.call("mprg_tree_objective", be.ptr(d_bufs), n_bufs, be.ptr(d_items), n, be.ptr(d_work), len(work), be.ptr(d_weights), len(flat),
            be.ptr(d_sums), be.ptr(d_status), be.stream, work=float((items[:, 2] * items[:, 3]).sum()))
    _check(be.download(d_status, np.int32, len(work)), "mprg_tree_objective", PG_STATUS)
    return be.download(d_sums, np.int64, n)


def _tree_step_fits(WX, WY, budget_words):
    """The spec's Limit of a step: the full DP can take it (the int32 score limit) within the workspace budget (with or without band:
    a merge the band does not help goes to the full DP)."""
    return (WX + WY < pa.MAX_LEN) & (pa.workspace_words_v(WX, WY) <= budget_words)


def _root_objectives(be, chunk: Chunk, plan: Plan, order, texts: _Texts, weights):
    """What _retree and _tree_refine start from, per locus: its records' multiplicities (all 1 without weights, the spec's Collapse),
    its empty records, whether mprg_tree_objective's bound, rows^2 W <= 2^58, holds for its root's text (only a locus of the spec's
    Large loci can miss it: 4 096 rows do not, below the DP's 10^6 columns; the caller leaves it out and reports it) and S of that
    text, 0 out of bound: one mprg_tree_objective launch.  order: per locus the records of its text's rows."""
    first, counts, n_loci = chunk.first, chunk.counts, chunk.n_loci
    roots = [texts.where[l, plan.root[l]] for l in range(n_loci)]
    wl = [np.ones(int(counts[l]), np.int64) if weights is None else weights[first[l]:first[l] + counts[l]] for l in range(n_loci)]
    empty = np.array([counts[l] - len(plan.leaves[l]) for l in range(n_loci)], np.int64)
    in_bound = np.array([(int(wl[l][order[l]].sum()) + int(empty[l])) ** 2 * roots[l][3] <= 1 << 58 for l in range(n_loci)], bool)
    known = np.nonzero(in_bound)[0].tolist()
    S = np.zeros(n_loci, np.int64)
    if known:
        S[known] = tree_objective(be, texts.table(be), len(texts.bufs), np.array([roots[l] for l in known], np.int64),
                                  [wl[l][order[l]] for l in known], empty[known])
    return wl, empty, in_bound, S


def _tree_refine(be, chunk: Chunk, plan: Plan, texts: _Texts, weights, opts: Options, counters, align=None):
    """The spec's Tree refinement over one chunk, on the roots' texts as _prog_rounds left them (texts, kept up here: where[locus,
    root] names the locus's current text; weights: per record of the chunk's tables, the spec's Collapse), opts.refine_tree passes
    over the loci of at most opts.tree_refine_max_leaves leaves.  Step s of every locus that still has one goes together: one
    split launch, the widths downloaded, the merges in _prog_groups' groups through _Merge.group, one objective launch, S
    downloaded.  Returns (per locus the records of its text's rows in row order, per locus (steps tried, accepted, skipped, S
    before, S after)).  align (the spec's Sequence weights): per record the q its row has in a realignment, in place of the
    multiplicities, which keep the choice of Y and the objective."""
    first, counts, n_loci = chunk.first, chunk.counts, chunk.n_loci
    leaves, root, where, merge = plan.leaves, plan.root, texts.where, opts.merge(counters)
    order = [np.array(x, np.int64) for x in plan.order]
    wl, empty, in_bound, S = _root_objectives(be, chunk, plan, order, texts, weights)
    al = wl if align is None else [align[first[l]:first[l] + counts[l]] for l in range(n_loci)]
    budget_words = max(64, int(opts.budget_bytes) // 4)
    if not in_bound.all():                                      # (such a locus is left out of the stage: no step and S = 0)
        add_to(counters, "tree_refine_over_bound", int((~in_bound).sum()))
    out = [[0, 0, 0, int(S[l]), int(S[l])] for l in range(n_loci)]
    n_lv = np.array([len(x) for x in leaves], np.int64)
    add_to(counters, "tree_refine_above_cap", int((n_lv > opts.tree_refine_max_leaves).sum()))
    steps = {}                                                  # per refinable locus, per step: is the record a leaf of G?
    for l in np.nonzero((n_lv >= TREE_REFINE_MIN_LEAVES) & (n_lv <= opts.tree_refine_max_leaves) & in_bound)[0].tolist():
        groups = tree_steps(plan.trees[l])
        steps[l] = np.zeros((len(groups), int(counts[l])), bool)
        for s, g in enumerate(groups):
            steps[l][s, g] = True
    active = [l for l in steps if len(steps[l])]
    add_to(counters, "tree_refine_loci", len(active))
    for _ in range(opts.refine_tree):
        moved = set()
        for s in range(max((len(steps[l]) for l in active), default=0)):
            its = [l for l in active if s < len(steps[l])]
            n = len(its)
            # the sides: Y the heavier of G and the rest, on equal weight sums the one with the locus's lowest leaf
            sides = []
            for l in its:
                o = order[l]
                in_g, w = steps[l][s][o], wl[l][o]
                wg, wo = int(w[in_g].sum()), int(w[~in_g].sum())
                g_is_y = wg > wo or (wg == wo and bool(in_g[np.argmin(o)]))
                sides.append((in_g != g_is_y).astype(np.uint8))
            split = np.array([where[l, root[l]] for l in its], np.int64)
            d_split, split_bytes, soff, widths = tree_split(be, texts.table(be), len(texts.bufs), split, sides)
            RY = np.array([int((sd == 0).sum()) for sd in sides], np.int64)
            WY, WX = widths[:, 0], widths[:, 1]
            b = texts.add(d_split, split_bytes)
            Y = np.stack([np.full(n, b), soff, RY, WY], 1).astype(np.int64)
            X = np.stack([np.full(n, b), soff + RY * WY, split[:, 2] - RY, WX], 1).astype(np.int64)
            fits = _tree_step_fits(WX, WY, budget_words)           # (a step beyond the limit is skipped: it counts as refused)
            sel = np.nonzero(fits)[0]
            new, made = {}, [b]
            for grp in _prog_groups(X[sel, 3], Y[sel, 3], merge):
                g = sel[grp]
                wg = None
                if weights is not None or align is not None:
                    wg = ([al[its[k]][order[its[k]][sides[k] == 1]] for k in g.tolist()], [al[its[k]][order[its[k]][sides[k] == 0]] for k in g.tolist()])
                new.update(zip(g.tolist(), merge.group(be, texts, X[g], Y[g], wg)))
                made.append(new[int(g[0])][0])
            ks = sorted(new)
            rows2 = {k: np.concatenate([order[its[k]][sides[k] == 0], order[its[k]][sides[k] == 1]]) for k in ks}     # Y's rows, then X's
            S2 = (tree_objective(be, texts.table(be), len(texts.bufs), np.array([new[k] for k in ks], np.int64),
                                 [wl[its[k]][rows2[k]] for k in ks], empty[[its[k] for k in ks]]) if ks else [])
            for k in range(n):
                out[its[k]][0] += 1
                out[its[k]][2] += int(not fits[k])
            for k, s2 in zip(ks, S2):
                l = its[k]
                if int(s2) > out[l][4]:                             # accepted: the locus's text is the new one
                    made.append(where[l, root[l]][0])
                    texts.place(l, root[l], new[k])
                    order[l] = rows2[k]
                    out[l][1], out[l][4] = out[l][1] + 1, int(s2)
                    moved.add(l)
            texts.drop_unused(made)
        active = [l for l in active if l in moved]
        if not active:
            break
    for key, i in (("tree_refine_steps", 0), ("tree_refine_accepted", 1), ("tree_refine_skipped", 2)):
        add_to(counters, key, sum(o[i] for o in out))
    return [o.tolist() for o in order], [tuple(o) for o in out]


# ---- refinement
def refine_counts(be, d_text, text_bytes: int, toff: np.ndarray, R: np.ndarray, W: np.ndarray):
    """mprg_refine_counts over MSAs on the device (per locus its offset in d_text, rows and columns): (the locus table with
    the column offsets filled in, the counts buffer, the keep flags, the columns, S per locus, the kept columns per locus)."""
    n = len(W)
    n_cols = int(W.sum())
    rtab = np.stack([toff, R, W, exclusive_sum(W)], 1).astype(np.int64)
    work = _tile_work(W)
    d_counts, d_keep, d_sums, d_status = be.empty(20 * n_cols), be.empty(n_cols), be.zeros(16 * n), be.empty(4 * len(work))
    d_rtab, d_work = be.upload(rtab), be.upload(work)
    be.call("mprg_refine_counts", be.ptr(d_text), text_bytes, be.ptr(d_rtab), n, be.ptr(d_work), len(work),
            be.ptr(d_counts), be.ptr(d_keep), n_cols, be.ptr(d_sums), be.ptr(d_status), be.stream, work=float((R * W).sum()))
    _check(be.download(d_status, np.int32, len(work)), "mprg_refine_counts", RF_STATUS)
    sums = be.download(d_sums, np.int64, 2 * n).reshape(-1, 2)
    return rtab, d_counts, d_keep, n_cols, sums[:, 0].copy(), sums[:, 1].copy()


def refine_profiles(be, d_text, text_bytes: int, rtab: np.ndarray, d_counts, n_cols: int, row_locus: np.ndarray, row_in_locus: np.ndarray):
    """mprg_refine_profiles: the leave-one-out profiles of the given rows (locus: an index into rtab) into one buffer:
    (the buffer, each row's offset in it in int32 elements, its size in int32 elements)."""
    Wr = rtab[row_locus, 2]
    poff = exclusive_sum(6 * Wr)
    words = int((6 * Wr).sum())
    work = _tile_work(Wr)
    d_prof, d_status = be.empty(4 * words), be.empty(4 * len(work))
    rows = np.stack([row_locus, row_in_locus, poff], 1).astype(np.int64)
    d_rtab, d_rows, d_work = be.upload(rtab), be.upload(rows), be.upload(work)
    be.call("mprg_refine_profiles", be.ptr(d_text), text_bytes, be.ptr(d_rtab), len(rtab), be.ptr(d_counts), n_cols,
            be.ptr(d_rows), len(rows), be.ptr(d_work), len(work), be.ptr(d_prof), words, be.ptr(d_status), be.stream,
            work=float(24 * words))
    _check(be.download(d_status, np.int32, len(work)), "mprg_refine_profiles", RF_STATUS)
    return d_prof, poff, words


def refine_compact(be, d_text, text_bytes: int, rtab: np.ndarray, d_keep, n_cols: int, out_off: np.ndarray, out_bytes: int):
    """mprg_refine_compact: every locus of rtab without its dropped columns, locus k's rows at out_off[k] of a new buffer of
    out_bytes (row stride: its kept columns).  Returns the buffer."""
    R = rtab[:, 1]
    rows = np.stack([np.repeat(np.arange(len(rtab)), R), _ranges(np.zeros(len(R), np.int64), R), np.repeat(out_off, R)], 1).astype(np.int64)
    d_dest, d_nw, d_out, d_status = be.empty(4 * n_cols), be.empty(8 * len(rtab)), be.empty(out_bytes), be.empty(4 * len(rows))
    d_rtab, d_rows = be.upload(rtab), be.upload(rows)
    be.call("mprg_refine_compact", be.ptr(d_text), text_bytes, be.ptr(d_rtab), len(rtab), be.ptr(d_keep), n_cols, be.ptr(d_dest),
            be.ptr(d_nw), be.ptr(d_rows), len(rows), be.ptr(d_out), out_bytes, be.ptr(d_status), be.stream,
            work=float(2 * (R * rtab[:, 2]).sum()))
    _check(be.download(d_status, np.int32, len(rows)), "mprg_refine_compact", RF_STATUS)
    return d_out


def _refine(be, chunk: Chunk, text, rounds, budget_bytes, band, counters, free_ends: bool = False):
    """The spec's Refinement over one chunk, on the MSA text the star or progressive pass left on the device (text: what they
    return).  Per locus: (rounds accepted, S of the star MSA, S of the result, None or where its new text is: (device buffer, its
    bytes, offset, width)).  free_ends: the spec's Free end pairs: every realignment as an overlap alignment."""
    lens, seq_off, first = chunk.lens, chunk.seq_off, chunk.first
    d_text, text_bytes, base, W = text
    text_bytes = max(text_bytes, 1)
    rtab, d_counts, _, n_cols, S0, _ = refine_counts(be, d_text, text_bytes, base, chunk.counts, W)
    out = [[0, int(S0[l]), int(S0[l]), None] for l in range(chunk.n_loci)]
    n_filled = np.add.reduceat((lens > 0).astype(np.int64), first)           # (every locus has a record)
    longest = np.maximum.reduceat(lens, first)
    todo = np.nonzero(n_filled >= 3)[0]
    budget_words = max(64, int(budget_bytes) // 4)
    # groups whose profiles of a round (24 W bytes per non-empty row) fit the budget
    for lo, hi in pa.budget_groups(24 * W[todo] * n_filled[todo], budget_bytes):
        act = todo[lo:hi]
        # the active loci's current MSAs: rows of `tab` {offset in buf, R, W, offset in the column tables of cnt}, S
        buf, buf_bytes, tab, cnt, cols, S = d_text, text_bytes, rtab[act], d_counts, n_cols, S0[act]
        for _ in range(rounds):
            # a locus whose longest row against its W columns the full DP cannot take (the int32 score limit, or more traceback
            # than the workspace budget: the band falls back to the full DP on sparse profiles) keeps the MSA it has
            fits = (longest[act] + tab[:, 2] < pa.MAX_LEN) & (pa.workspace_words_v(longest[act], tab[:, 2]) <= budget_words)
            act, tab, S = act[fits], tab[fits], S[fits]
            if not len(act):
                break
            R, Wc = tab[:, 1], tab[:, 2]
            all_rows = _ranges(first[act], R)                # the loci's rows in the chunk's sequence table
            of_locus = np.repeat(np.arange(len(act)), R)
            q = np.nonzero(lens[all_rows] > 0)[0]               # the non-empty ones: a leave-one-out profile and a pair each
            row_locus, grow = of_locus[q], all_rows[q]
            d_prof, poff, _ = refine_profiles(be, buf, buf_bytes, tab, cnt, cols, row_locus, grow - first[act][row_locus])
            prepared = pa.PreparedProfiles(d_prof, np.stack([R[row_locus] - 1, Wc[row_locus]], 1), poff, chunk.d_codes, seq_off[grow], lens[grow])
            dp = pa.pairs_on_device(be, None, None, budget_bytes, band, counters, prepared, free_ends=free_ends)
            if free_ends:
                add_to(counters, "free_end_pair_alignments", len(q))
            # the merge over the W columns: every non-empty row has ops, an empty one stays all gaps (count -1, n = 0)
            rows = np.zeros((len(all_rows), ROW_FIELDS), np.int64)
            rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4] = of_locus, seq_off[all_rows], lens[all_rows], -1
            rows[q, 3], rows[q, 4] = dp.ops_off, dp.count
            d_new, new_bytes, off2, W2 = _star_merge(be, chunk, dp.d_ops, dp.ops_bytes, rows, exclusive_sum(R), R, Wc)
            tab2, cnt2, keep2, cols2, S2, kept = refine_counts(be, d_new, new_bytes, off2, R, W2)
            if (kept < W2).any():                               # a column emptied: drop it, count again (runs may have joined)
                d_new = refine_compact(be, d_new, new_bytes, tab2, keep2, cols2, off2, new_bytes)
                tab2, cnt2, keep2, cols2, S2, kept = refine_counts(be, d_new, new_bytes, off2, R, kept)
            ok = S2 > S
            for k in np.nonzero(ok)[0]:
                o = out[act[k]]
                o[0], o[2], o[3] = o[0] + 1, int(S2[k]), (d_new, new_bytes, int(off2[k]), int(tab2[k, 2]))
            act, buf, buf_bytes, tab, cnt, cols, S = act[ok], d_new, new_bytes, tab2[ok], cnt2, cols2, S2[ok]
    return [tuple(o) for o in out]


# ---- files
def read_unaligned(path) -> List[Tuple[str, str]]:
    """The records of an unaligned FASTA(.gz) file as (title: the header line without '>', sequence: its lines joined, white
    space removed), in file order."""
    import gzip
    from ..msa import _parse_fasta
    path = str(path)
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as fh:
        return list(_parse_fasta(fh.read()))


def msa_fasta(msa: MSA) -> str:
    """One header line (the record's title) and one sequence line per row."""
    return "".join(f">{t}\n{msa.data[i].tobytes().decode()}\n" for i, t in enumerate(msa.descriptions))
