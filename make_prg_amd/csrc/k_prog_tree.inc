// ---------------------------------------------------------------------------------------------------------------
// K-T  the guide tree of `from_msa --unaligned --progressive --device-tree` (make_prg_amd/from_msa/star_align.py holds the spec,
//      "Progressive": Tree, and "Collapse": the weighted form; DESIGN.md §3b, "Device tree").  Integers only.  A kernel of its own:
//      every kernel of k_prog.inc, k_prog_band.inc and k_collapse.inc stays what it was.
//
// k_prog_tree: one workgroup per locus, exact UPGMA over the locus's leaves (its records of length > 0), a slot per RECORD (a
//   record that is no leaf, and a cluster merged into another, has size 0).  S, the m x m int64 sums of w_a w_b D(a, b) between
//   the clusters (symmetric, both halves kept so that a row is read coalesced), lives in the locus's workspace; per slot the
//   cluster's size (weight sum), the row's best partner among the LATER keys and that partner's sum live in LDS up to TR_LDS_M
//   records (8 KB) and behind S in the workspace above (the same code, instantiated for either address space).
//   A merge step: (1) every row marked for a rescan is scanned by one wavefront (lanes on consecutive later keys, a wave
//   reduction); (2) a block reduction over the rows' best pairs names (U, V); (3) row and column U of S take row V's sums, and
//   thread x decides in O(1) what the merge means for row x: its best partner was U or V: marked for a rescan; x < U: the new
//   cluster U against the row's best; U < x: nothing (a row only looks at later keys).  Three barriers per merge.
//   Averages are compared by cross-multiplication in int64 (below 2^60: sums <= 65 536 |U| |V|, |U| + |V| <= 4 096); equal
//   averages go to the smaller key, in the rescan (the partner's key) as in the reduction (the row's key): the pair the plain
//   statement's strict "smaller" keeps while it walks (key(U), key(V)) in ascending order.
//   All averages equal: row a's best is the next live key, one row is rescanned per merge: O(m^2) in all.
//   The body is the text of tr_upgma.inc, which k_prog_tree_wide.inc includes too; the candidate types and the compare are here.
// ---------------------------------------------------------------------------------------------------------------
#define TR_LDS_M 512                           // records whose per-slot state is kept in LDS
#define TR_MAX_WEIGHT 4096                     // the spec's PROG_MAX_LEAVES: the largest weight sum of a locus
#define TR_SCALE 65536                         // the spec's PROG_SCALE
#define TR_NONE (-1)                           // best partner: no live later key
#define TR_RESCAN (-2)                         // best partner: to be found again

// the average num / den of the pair named by idx (the partner's key within a row, the row's key among rows); idx < 0: none
struct TrCand { long long num; int den, idx; };
// what the block reduction hands every thread: the winning row u, its partner v, their sizes
struct TrPick { long long num; int den, u, v, su, sv; };

MPRG_DEV bool tr_less(const TrCand a, const TrCand b) {
  if (a.idx < 0) return false;
  if (b.idx < 0) return true;
  const long long l = a.num * b.den, r = b.num * a.den;
  return l < r || (l == r && a.idx < b.idx);
}

#define TR_CAND TrCand
#define TR_PICK TrPick
#define TR_LESS tr_less
#define TR_DEN(a, b) a * b
#define TR_WEIGHT_TOP TR_MAX_WEIGHT
#define TR_LEAF_TOP TR_MAX_WEIGHT
#define TR_WAVE_MIN tr_wave_min
#define TR_BUILD tr_build
#define TR_KERNEL k_prog_tree
#include "tr_upgma.inc"
#undef TR_CAND
#undef TR_PICK
#undef TR_LESS
#undef TR_DEN
#undef TR_WEIGHT_TOP
#undef TR_LEAF_TOP
#undef TR_WAVE_MIN
#undef TR_BUILD
#undef TR_KERNEL
