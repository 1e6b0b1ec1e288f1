// ---------------------------------------------------------------------------------------------------------------
// K-A scores (`from_msa --unaligned --progressive --pair-distances`; the spec: make_prg_amd/from_msa/star_align.py, "Pair
// distances"; DESIGN.md §3b): the score of the pair DP alone, for guide trees built from all pairs of a locus.
//
// k_align_scores: k_align_pairs' sweep without the traceback and without the walk back: the same argument checks, row 0, 128-column
//   LDS ring per wavefront, 64-row strips, row above by __shfl_up, H[i][0] by al_hb, and the same cell (al_cell.inc, as text: its
//   `cell` word is computed and dropped).  A pair's workspace is the row buffer alone, ((2 (C + 1) + 63) / 64) * 64 words.  Lane 0
//   writes out[2 p] = {status, score} and, where the pair's dst >= 0, tab[dst] = max(score, 0) >> 6: an entry of the table s'' the
//   tree kernels read.  A dst outside the table is MPRG_AL_NO_SPACE before anything is written.
// k_align_scores_banded: the same relation to k_align_pairs_banded: W = dhi - dlo + 1 slots of row buffer, strips from
//   max(0, i0 + dlo), everything outside the band AL_NEG.  A later pass over a wider band overwrites out and tab[dst] of its pair.
// k_align_scores_endgap, k_align_scores_endgap_banded (`--free-end-distances`; star_align.py, "Free end distances"): the two with
//   the free ends of k_align_pairs_endgap: row 0 and column 0 are 0, the last row's D ops and the last column's I ops are free; the
//   same checks, workspace and writes.  The kernels' texts are al_scores.inc and al_scores_band.inc, each included twice below.
// ---------------------------------------------------------------------------------------------------------------
MPRG_DEV long long al_score_ws_words(long long C) { return ((2 * (C + 1) + 63) / 64) * 64; }
MPRG_DEV long long al_score_band_ws_words(long long dlo, long long dhi) { return ((2 * (dhi - dlo + 1) + 63) / 64) * 64; }

// k_align_scores and k_align_scores_endgap: one text (al_scores.inc), the second with the free ends of "Free end distances"
#define AL_SCORES_KERNEL k_align_scores
#define AL_ENDGAP 0
#include "al_scores.inc"
#undef AL_SCORES_KERNEL
#undef AL_ENDGAP
#define AL_SCORES_KERNEL k_align_scores_endgap
#define AL_ENDGAP 1
#include "al_scores.inc"
#undef AL_SCORES_KERNEL
#undef AL_ENDGAP

// k_align_scores_banded and k_align_scores_endgap_banded: one text (al_scores_band.inc)
#define AL_SCORES_KERNEL k_align_scores_banded
#define AL_ENDGAP 0
#include "al_scores_band.inc"
#undef AL_SCORES_KERNEL
#undef AL_ENDGAP
#define AL_SCORES_KERNEL k_align_scores_endgap_banded
#define AL_ENDGAP 1
#include "al_scores_band.inc"
#undef AL_SCORES_KERNEL
#undef AL_ENDGAP
