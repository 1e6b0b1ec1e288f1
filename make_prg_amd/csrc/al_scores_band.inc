// k_align_scores_banded (k_align_scores.inc's header) and its form with free ends, k_align_scores_endgap_banded (star_align.py,
// "Free end distances"): one text, included twice (DESIGN.md §3a).  The includer provides AL_SCORES_KERNEL, the kernel's name, and
// AL_ENDGAP: 0 expands to the tokens the kernel had when it stood in k_align_scores.inc; 1 is al_scores.inc's: row 0 and column 0 are
// 0 where the band holds them, the last row's D ops and the last column's I ops are free; everything outside the band stays AL_NEG.
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
  const int64_t *PT = pairs + MPRG_AL_SCORE_BAND_PAIR_FIELDS * p;
  const long long leaf = PT[0], soff = PT[1], n = PT[2], wsoff = PT[3], dst = PT[4];
  long long blo = PT[5], bhi = PT[6];
  int32_t *o = out + 2 * p;
  int status = MPRG_AL_OK;
  long long C = 0, poff = 0;
  if (leaf < 0 || leaf >= n_leaves) status = MPRG_AL_BAD_INPUT;
  else {
    C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
    poff = leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
    if (C < 1 || n < 0 || leaves[MPRG_AL_LEAF_FIELDS * leaf + 1] < 1) status = MPRG_AL_BAD_INPUT;
    else if (n + C >= AL_MAX_CELLS_SUM) status = MPRG_AL_TOO_LONG;
    else if (blo > 0 || blo > C - n || bhi < 0 || bhi < C - n) status = MPRG_AL_BAD_INPUT;      // the band must hold both corners
    else {
      blo = blo < -n ? -n : blo;
      bhi = bhi > C ? C : bhi;
      if (wsoff < 0 || (wsoff & 63) || wsoff + al_score_band_ws_words(blo, bhi) > ws_words || dst >= tab_words) status = MPRG_AL_NO_SPACE;
    }
  }
  if (status != MPRG_AL_OK) {
    if (lane == 0) { o[0] = status; o[1] = 0; }
    return;
  }
  const int32_t *P = profile + al_uniform(poff);
  const int Ci = (int)al_uniform(C), ni = (int)al_uniform(n), dlo = (int)al_uniform(blo), dhi = (int)al_uniform(bhi);
  const int W = dhi - dlo + 1;
  const long long soff_u = al_uniform(soff);
  int32_t *row = ws + al_uniform(wsoff);                     // row[2k] = H, row[2k + 1] = I of the row above the strip (row i0), column i0 + dlo + k
#if AL_ENDGAP
  // row 0, columns 0 .. dhi: H[0][J] = D[0][J] = 0, the leaf's leading columns alone are free
  for (int c0 = 0; c0 < dhi; c0 += 64) {
    const int c = c0 + lane;
    if (c < dhi) { row[2 * (c + 1 - dlo)] = 0; row[2 * (c + 1 - dlo) + 1] = AL_NEG; }
  }
#else
  // row 0, columns 0 .. dhi: H[0][J] = D[0][J] = open + the gap costs of columns < J
  int carry = 0;
  for (int c0 = 0; c0 < dhi; c0 += 64) {
    const int c = c0 + lane;
    const int incl = wave_scan_incl(c < dhi ? (P + 5LL * Ci)[(unsigned)c] : 0) + carry;
    if (c < dhi) { row[2 * (c + 1 - dlo)] = AL_OPEN + incl; row[2 * (c + 1 - dlo) + 1] = AL_NEG; }
    carry = __shfl(incl, 63);
  }
#endif
  if (lane == 0) { row[2 * (-dlo)] = 0; row[2 * (-dlo) + 1] = AL_NEG; }
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
    const int cs = i0 + dlo > 0 ? i0 + dlo : 0;             // the strip's first column, 0-based
    const int jtop = i0 + dhi < Ci ? i0 + dhi : Ci;         // the last column of row i0 inside the band
    const int jend = i0 + rows + dhi < Ci ? i0 + rows + dhi : Ci;   // the strip's last column, 1-based
    const int d0 = cs - r - dlo;                            // 0-based column c = cs + t - lane of this lane's row (r + 1) lies on diagonal c - r:
                                                            // inside the band where 0 <= d0 + t - lane <= dhi - dlo (and 0 <= c < C)
    const bool col0 = r + 1 + dlo <= 0;                     // column 0 of this lane's row lies inside the band
    int h_left = col0 ? AL_HB(r + 1) : AL_NEG, d_left = AL_NEG;     // H, D of this lane's row, the column to the left of its first one
    int h_out = col0 && cs == lane ? AL_HB(r + 1) : AL_NEG, i_out = AL_NEG;   // what the lane below reads next step: here of column cs - 1 - lane
    int h_up_prev = AL_NEG;                                  // H of the row above, one column to the left: the diagonal
    if (lane == 0) h_up_prev = cs == 0 ? AL_HB(i0) : row[0];   // (cs > 0: column cs = i0 + dlo of row i0, its first inside the band)
    const int T = jend - cs + rows - 1;
    for (int t = 0; t < T; ++t) {
      if ((t & 63) == 0) {                                   // the ring takes columns cs + [t, t + 64): the block 128 before is done with
        WAVE_SYNC();
#pragma unroll
        for (int k = 0; k < 6; ++k)
          ring[k * AL_RING + ((t + lane) & (AL_RING - 1))] = cs + t + lane < Ci ? (P + (long long)k * Ci)[(unsigned)(cs + t + lane)] : 0;
        WAVE_SYNC();
      }
      int h_up = __shfl_up(h_out, 1), i_up = __shfl_up(i_out, 1);
      if (lane == 0) {
        const int j = cs + t + 1, k = j - (i0 + dlo);         // (1 <= k; k <= W - 1 where j <= jtop)
        h_up = j <= jtop ? row[(unsigned)(2 * k)] : AL_NEG;
        i_up = j <= jtop ? row[(unsigned)(2 * k + 1)] : AL_NEG;
      }
      const int h_diag = h_up_prev;
      h_up_prev = h_up;
      const int c = cs + t - lane;
      unsigned cell = 0;
      if (valid && (unsigned)c < (unsigned)Ci && (unsigned)(d0 + t - lane) < (unsigned)W) {
        const int slot = (t - lane) & (AL_RING - 1);
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
        if (lane == 63 && s + 1 < n_strips) { const int k = c + 1 - (i0 + 64 + dlo); row[(unsigned)(2 * k)] = h; row[(unsigned)(2 * k + 1)] = ii; }
      } else {
        h_out = c == -1 && r + 1 + dlo <= 0 ? AL_HB(r + 1) : AL_NEG;   // outside the band: minus infinity, never a stale or an accumulated value
        i_out = AL_NEG;
      }
      (void)cell;                                            // no traceback: the score is all that leaves
    }
    WAVE_SYNC_GLOBAL();                                      // the row buffer, written by lane 63, read by lane 0
  }
  score = ni > 0 ? __shfl(score, (ni - 1) & 63) : row[2 * (Ci - dlo)];
  if (lane == 0) {
    o[0] = MPRG_AL_OK; o[1] = score;
    if (dst >= 0) tab[dst] = (uint32_t)((score > 0 ? score : 0) >> 6);
  }
}
#undef AL_HB
