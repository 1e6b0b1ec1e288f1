// ---------------------------------------------------------------------------------------------------------------
// K-TW the guide tree of `from_msa --unaligned --progressive --collapse-identical --large-loci --device-tree`
//      (make_prg_amd/from_msa/star_align.py holds the spec, "Large loci"; DESIGN.md §3b, "Large loci").  Integers only.  A kernel of
//      its own: k_prog_tree and every other kernel stay what they were.
//
// k_prog_tree_wide: k_prog_tree (k_prog_tree.inc; the body is the same text, tr_upgma.inc) for weight sums up to
//   TRW_MAX_WEIGHT = 2^20 over at most TR_MAX_WEIGHT = 4 096 leaves.  With |U| + |V| <= 2^20 a sum of w_a w_b D(a, b) between two
//   clusters is at most 65 536 |U| |V| <= 2^54 (an entry of S too: w_a + w_b <= 2^20), so S stays int64; a denominator |U| |V| is
//   at most 2^38, so it is 64-bit here; a cross product is at most 2^92, so the compare multiplies in 128 bits.
// ---------------------------------------------------------------------------------------------------------------
#define TRW_MAX_WEIGHT (1 << 20)               // the spec's PROG_MAX_RECORDS: the largest weight sum of a locus

struct TrCandW { long long num, den; int idx; };
struct TrPickW { long long num, den; int u, v, su, sv; };

MPRG_DEV bool tr_less_wide(const TrCandW a, const TrCandW b) {
  if (a.idx < 0) return false;
  if (b.idx < 0) return true;
  const unsigned __int128 l = (unsigned __int128)(unsigned long long)a.num * (unsigned long long)b.den;     // (num >= 0, den >= 1)
  const unsigned __int128 r = (unsigned __int128)(unsigned long long)b.num * (unsigned long long)a.den;
  return l < r || (l == r && a.idx < b.idx);
}

#define TR_CAND TrCandW
#define TR_PICK TrPickW
#define TR_LESS tr_less_wide
#define TR_DEN(a, b) (long long)a * b
#define TR_WEIGHT_TOP TRW_MAX_WEIGHT
#define TR_LEAF_TOP TR_MAX_WEIGHT
#define TR_WAVE_MIN tr_wave_min_wide
#define TR_BUILD tr_build_wide
#define TR_KERNEL k_prog_tree_wide
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
