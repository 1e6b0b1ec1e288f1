// k_align_scores (k_align_scores.inc's header) and its form with free ends, k_align_scores_endgap (star_align.py, "Free end
// distances"): one text, included twice (DESIGN.md §3a).  The includer provides AL_SCORES_KERNEL, the kernel's name, and AL_ENDGAP:
// 0 expands to the tokens the kernel had when it stood in k_align_scores.inc.  1 is al_pairs.inc's AL_ENDGAP without the traceback:
// row 0 is written as zeros, so Dc is not scanned; H[i][0] is 0 in place of al_hb; the lane of the last row (r == ni - 1, fixed
// over a strip) extends and opens a run of D ops for 0, every lane a run of I ops for 0 in the last column (c == Ci - 1): plain
// selects in front of al_cell.inc, which stays as it is.
#if AL_ENDGAP
#define AL_HB(i) 0
#else
#define AL_HB(i) al_hb(i)
#endif
__global__ void __launch_bounds__(AL_THREADS) AL_SCORES_KERNEL(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                             const uint8_t *seqs, const int64_t *pairs, int n_pairs, int32_t *ws,
                                                             long long ws_words, uint32_t *tab, long long tab_words, int32_t *out) {
  SHARED(int32_t, ring_all, AL_WAVES * 6 * AL_RING);
  const int lane = wave_lane();
  const long long p = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (p >= n_pairs) return;                                   // (a whole wavefront: nothing below waits for the others)
  int32_t *ring = ring_all + wave_id() * 6 * AL_RING;
  const int64_t *PT = pairs + MPRG_AL_SCORE_PAIR_FIELDS * p;
  const long long leaf = PT[0], soff = PT[1], n = PT[2], wsoff = PT[3], dst = PT[4];
  int32_t *o = out + 2 * p;
  int status = MPRG_AL_OK;
  long long C = 0, poff = 0;
  if (leaf < 0 || leaf >= n_leaves) status = MPRG_AL_BAD_INPUT;
  else {
    C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
    poff = leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
    if (C < 1 || n < 0 || leaves[MPRG_AL_LEAF_FIELDS * leaf + 1] < 1) status = MPRG_AL_BAD_INPUT;
    else if (n + C >= AL_MAX_CELLS_SUM) status = MPRG_AL_TOO_LONG;
    else if (wsoff < 0 || (wsoff & 63) || wsoff + al_score_ws_words(C) > ws_words || dst >= tab_words) status = MPRG_AL_NO_SPACE;
  }
  if (status != MPRG_AL_OK) {
    if (lane == 0) { o[0] = status; o[1] = 0; }
    return;
  }
  const int32_t *P = profile + al_uniform(poff);
  const int Ci = (int)al_uniform(C), ni = (int)al_uniform(n);
  const long long soff_u = al_uniform(soff);
  int32_t *row = ws + al_uniform(wsoff);                     // row[2J] = H, row[2J + 1] = I of the row above the strip, column J
#if AL_ENDGAP
  // row 0: H[0][J] = D[0][J] = 0, the leaf's leading columns alone are free
  for (int c0 = 0; c0 < Ci; c0 += 64) {
    const int c = c0 + lane;
    if (c < Ci) { row[2 * (c + 1)] = 0; row[2 * (c + 1) + 1] = AL_NEG; }
  }
#else
  // row 0: H[0][J] = D[0][J] = open + the gap costs of columns < J
  int carry = 0;
  for (int c0 = 0; c0 < Ci; c0 += 64) {
    const int c = c0 + lane;
    const int incl = wave_scan_incl(c < Ci ? (P + 5LL * Ci)[(unsigned)c] : 0) + carry;
    if (c < Ci) { row[2 * (c + 1)] = AL_OPEN + incl; row[2 * (c + 1) + 1] = AL_NEG; }
    carry = __shfl(incl, 63);
  }
#endif
  if (lane == 0) { row[0] = 0; row[1] = AL_NEG; }
  WAVE_SYNC_GLOBAL();
  int score = AL_NEG;
  const int n_strips = (ni + 63) / 64;
  for (int s = 0; s < n_strips; ++s) {
    const int i0 = s * 64, r = i0 + lane, rows = ni - i0 < 64 ? ni - i0 : 64;
    const bool valid = r < ni;
    const unsigned code = valid ? (seqs + soff_u)[(unsigned)r] : 0u;
    const int cls = code < 4 ? (int)code : 4;
#if AL_ENDGAP
    const bool last_row = r == ni - 1;                      // its D ops are the trailing ones: free
#endif
    int h_left = AL_HB(r + 1), d_left = AL_NEG;            // H, D of this lane's row, the column to the left
    int h_out = h_left, i_out = AL_NEG;                     // what the lane below reads next step (before the first column: H[i][0])
    int h_up_prev = AL_HB(i0);                               // (lane 0) H of the row above, one column to the left: the diagonal
    const int T = Ci + rows - 1;
    for (int t = 0; t < T; ++t) {
      if ((t & 63) == 0) {                                   // the ring takes columns [t, t + 64): the block of columns t - 128 is done with
        WAVE_SYNC();
#pragma unroll
        for (int k = 0; k < 6; ++k)
          ring[k * AL_RING + ((t + lane) & (AL_RING - 1))] = t + lane < Ci ? (P + (long long)k * Ci)[(unsigned)(t + lane)] : 0;
        WAVE_SYNC();
      }
      int h_up = __shfl_up(h_out, 1), i_up = __shfl_up(i_out, 1);
      if (lane == 0 && t < Ci) { h_up = row[2 * (t + 1)]; i_up = row[2 * (t + 1) + 1]; }
      const int h_diag = h_up_prev;
      h_up_prev = h_up;
      const int c = t - lane;
      unsigned cell = 0;
      if (valid && c >= 0 && c < Ci) {
        const int slot = c & (AL_RING - 1);
#if AL_ENDGAP
        const int dc = last_row ? 0 : ring[5 * AL_RING + slot];
        const int diag = h_diag + ring[cls * AL_RING + slot];
        const bool last_col = c == Ci - 1;                   // its I ops are the trailing ones: free
        const int xcost = last_col ? 0 : AL_INS;
#define AL_OPEN_D (last_row ? 0 : AL_OPEN) + dc
#define AL_OPEN_I (last_col ? 0 : AL_OPEN) + xcost
#else
        const int dc = ring[5 * AL_RING + slot];
        const int diag = h_diag + ring[cls * AL_RING + slot];
        const int xcost = AL_INS;
#define AL_OPEN_D AL_OPEN + dc
#define AL_OPEN_I AL_OPEN + xcost
#endif
#include "al_cell.inc"
#undef AL_OPEN_D
#undef AL_OPEN_I
        if (lane == 63 && s + 1 < n_strips) { row[2 * (c + 1)] = h; row[2 * (c + 1) + 1] = ii; }
      }
      (void)cell;                                            // no traceback: the score is all that leaves
    }
    WAVE_SYNC_GLOBAL();                                      // the row buffer, written by lane 63, read by lane 0
  }
  score = ni > 0 ? __shfl(score, (ni - 1) & 63) : row[2 * Ci];
  if (lane == 0) {
    o[0] = MPRG_AL_OK; o[1] = score;
    if (dst >= 0) tab[dst] = (uint32_t)((score > 0 ? score : 0) >> 6);
  }
}
#undef AL_HB
