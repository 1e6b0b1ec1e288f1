// k_align_profile_pairs (k_prog.inc's header) and its form with position-specific opens, k_align_profile_pairs_posgap
// (star_align.py, "Position gaps"): one text, included twice (DESIGN.md §3a).  The includer provides PG_PAIRS_KERNEL, the kernel's
// name, and PG_POSGAP: 0 expands to the tokens the kernel had when it stood in k_prog.inc.  1: Y's profile has a seventh plane
// Oc (k_prog_columns' kind 2), the ring a seventh plane Oc[j] + Dc[j], so that opening a run of D ops at column j is one LDS
// read and one addition; a lane keeps Ox + Ic of its X column, Ox = (-704 (R_X - g)) / R_X by pg_div (|v| <= 704 R_X, inside its
// proven range); row 0 opens with Oc[0], column 0 with Ox[0].
// PG_ENDGAP (star_align.py, "Free end gaps"; both values of PG_POSGAP): 0 expands to the tokens above.  1: row 0 and column 0 are
// 0, so neither the prefix sums nor Oc[0] / Ox[0] are taken; the lane of the last row (r == ni - 1, fixed over a strip) extends and
// opens a run of D ops for 0, every lane a run of I ops for 0 in the last column (c == Ci - 1): plain selects in front of
// al_cell.inc, which stays as it is.  The cell's score keeps Y's real Dc.
#if PG_POSGAP
#define PG_RING_PLANES 7
#define PG_OPEN_ROW0 oc0
#define PG_OPEN_COL0 ox0
#else
#define PG_RING_PLANES 6
#define PG_OPEN_ROW0 AL_OPEN
#define PG_OPEN_COL0 AL_OPEN
#endif
__global__ void __launch_bounds__(AL_THREADS) PG_PAIRS_KERNEL(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                                    const int32_t *xcols, long long xcols_words, const int64_t *pairs,
                                                                    int n_pairs, int32_t *ws, long long ws_words, uint8_t *ops,
                                                                    long long ops_bytes, int32_t *out) {
  SHARED(int32_t, ring_all, AL_WAVES * PG_RING_PLANES * AL_RING);
  const int lane = wave_lane();
  const long long p = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (p >= n_pairs) return;                                   // (a whole wavefront: nothing below waits for the others)
  int32_t *ring = ring_all + wave_id() * PG_RING_PLANES * AL_RING;
  const int64_t *PT = pairs + MPRG_PG_PAIR_FIELDS * p;
  const long long leaf = PT[0], xoff = PT[1], n = PT[2], wsoff = PT[3], opoff = PT[4], RX = PT[5];
  int32_t *o = out + 3 * p;
  int status = MPRG_AL_OK;
  long long C = 0, poff = 0;
  if (leaf < 0 || leaf >= n_leaves) status = MPRG_AL_BAD_INPUT;
  else {
    C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
    poff = leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
    if (C < 1 || n < 0 || leaves[MPRG_AL_LEAF_FIELDS * leaf + 1] < 1 || RX < 1 || RX > PG_MAX_ROWS) status = MPRG_AL_BAD_INPUT;
    else if (n + C >= AL_MAX_CELLS_SUM) status = MPRG_AL_TOO_LONG;
    else if (wsoff < 0 || (wsoff & 63) || wsoff + al_ws_words(n, C) > ws_words || opoff < 0 || opoff + n + C > ops_bytes ||
             xoff < 0 || xoff > xcols_words || 7 * n > xcols_words - xoff)
      status = MPRG_AL_NO_SPACE;
  }
  if (status != MPRG_AL_OK) {
    if (lane == 0) { o[0] = status; o[1] = 0; o[2] = 0; }
    return;
  }
  const int32_t *P = profile + al_uniform(poff);
  const int Ci = (int)al_uniform(C), ni = (int)al_uniform(n);
  const int32_t *X = xcols + al_uniform(xoff);
  const PgDiv dv = pg_div_make(al_uniform(RX));
  const long long wsoff_u = al_uniform(wsoff);
  int32_t *row = ws + wsoff_u;                               // row[2J] = H, row[2J + 1] = I of the row above the strip, column J
  uint32_t *tb = (uint32_t *)(ws + wsoff_u + ((2 * ((long long)Ci + 1) + 63) / 64) * 64);
  const long long nst8 = ((long long)Ci + 63 + 7) / 8;
#if PG_POSGAP
  const int RXi = (int)al_uniform(RX);
#endif
#if PG_ENDGAP
  // row 0: H[0][J] = D[0][J] = 0, Y's leading columns alone are free
  for (int c0 = 0; c0 < Ci; c0 += 64) {
    const int c = c0 + lane;
    if (c < Ci) { row[2 * (c + 1)] = 0; row[2 * (c + 1) + 1] = AL_NEG; }
  }
  if (lane == 0) { row[0] = 0; row[1] = AL_NEG; }
  WAVE_SYNC_GLOBAL();
  int score = AL_NEG;
#else
#if PG_POSGAP
  const int oc0 = (P + 6LL * Ci)[0];                          // what a run that starts at Y's first column pays: row 0
  const int ox0 = ni > 0 ? pg_div(AL_OPEN * (RXi - (X + 5LL * ni)[0]), dv) : 0;   // ... at X's first column: column 0
#endif
  // row 0: H[0][J] = D[0][J] = open + the gap costs of columns < J
  int carry = 0;
  for (int c0 = 0; c0 < Ci; c0 += 64) {
    const int c = c0 + lane;
    const int incl = wave_scan_incl(c < Ci ? (P + 5LL * Ci)[(unsigned)c] : 0) + carry;
    if (c < Ci) { row[2 * (c + 1)] = PG_OPEN_ROW0 + incl; row[2 * (c + 1) + 1] = AL_NEG; }
    carry = __shfl(incl, 63);
  }
  if (lane == 0) { row[0] = 0; row[1] = AL_NEG; }
  WAVE_SYNC_GLOBAL();
  int score = AL_NEG;
  int ic_before = 0;                                         // the Ic of all rows above the strip
#endif
  const int n_strips = (ni + 63) / 64;
  for (int s = 0; s < n_strips; ++s) {
    const int i0 = s * 64, r = i0 + lane, rows = ni - i0 < 64 ? ni - i0 : 64;
    const bool valid = r < ni;
    // this lane's X column: the counts of A C G T, of the ambiguity codes, of '-', and what the column alone costs
    const int x0 = valid ? X[(unsigned)r] : 0, x1 = valid ? (X + (long long)ni)[(unsigned)r] : 0;
    const int x2 = valid ? (X + 2LL * ni)[(unsigned)r] : 0, x3 = valid ? (X + 3LL * ni)[(unsigned)r] : 0;
    const int xa = valid ? (X + 4LL * ni)[(unsigned)r] : 0, xg = valid ? (X + 5LL * ni)[(unsigned)r] : 0;
    const int ic = valid ? (X + 6LL * ni)[(unsigned)r] : 0;
#if PG_POSGAP
    const int oxic = pg_div(AL_OPEN * (RXi - xg), dv) + ic;  // opening a run of I ops with this column: Ox + Ic
#endif
#if PG_ENDGAP
    const bool last_row = r == ni - 1;                      // its D ops are the trailing ones: free
    int h_left = 0, d_left = AL_NEG;                        // H, D of this lane's row, the column to the left: H[r + 1][0] = 0
    int h_out = 0, i_out = AL_NEG;                          // what the lane below reads next step (before the first column: H[i][0])
    int h_up_prev = 0;                                      // (lane 0) H of the row above, one column to the left: the diagonal
#else
    const int ic_incl = wave_scan_incl(ic) + ic_before;     // the Ic of rows 1 .. r + 1
    int h_left = PG_OPEN_COL0 + ic_incl, d_left = AL_NEG;  // H, D of this lane's row, the column to the left: H[r + 1][0]
    int h_out = h_left, i_out = AL_NEG;                     // what the lane below reads next step (before the first column: H[i][0])
    int h_up_prev = i0 == 0 ? 0 : PG_OPEN_COL0 + ic_before; // (lane 0) H of the row above, one column to the left: the diagonal
    ic_before = __shfl(ic_incl, 63);
#endif
    uint32_t acc = 0;
    uint32_t *tbs = tb + (long long)s * nst8 * 64;
    int h_row = AL_NEG, i_row = AL_NEG;                      // H, I of the row above the strip, column t0 + 1 + lane of the 64-step block
    const int T = Ci + rows - 1;
    for (int t = 0; t < T; ++t) {
      if ((t & 63) == 0) {                                   // the ring takes columns [t, t + 64): the block of columns t - 128 is done with
        WAVE_SYNC();
#pragma unroll
        for (int k = 0; k < 6; ++k) ring[k * AL_RING + ((t + lane) & (AL_RING - 1))] = t + lane < Ci ? (P + (long long)k * Ci)[(unsigned)(t + lane)] : 0;
#if PG_POSGAP
        ring[6 * AL_RING + ((t + lane) & (AL_RING - 1))] =
            t + lane < Ci ? (P + 6LL * Ci)[(unsigned)(t + lane)] + (P + 5LL * Ci)[(unsigned)(t + lane)] : 0;
#endif
        // ... and the row above for the block's 64 steps in one coalesced read: a load per step would put the memory latency into
        // every step of the chain (lane 63 writes the next strip's column c + 1 = t - 62 at step t: after this read of it)
        h_row = t + lane < Ci ? row[(unsigned)(2 * (t + lane + 1))] : AL_NEG;
        i_row = t + lane < Ci ? row[(unsigned)(2 * (t + lane + 1) + 1)] : AL_NEG;
        WAVE_SYNC();
      }
      int h_up = __shfl_up(h_out, 1), i_up = __shfl_up(i_out, 1);
      const int h_top = __shfl(h_row, t & 63), i_top = __shfl(i_row, t & 63);
      if (lane == 0 && t < Ci) { h_up = h_top; i_up = i_top; }
      const int h_diag = h_up_prev;
      h_up_prev = h_up;
      const int c = t - lane;
      unsigned cell = 0;
      if (valid && c >= 0 && c < Ci) {
        const int slot = c & (AL_RING - 1);
#if PG_ENDGAP
        const int dc_y = ring[5 * AL_RING + slot];           // Y's column alone, for the cell's score; dc: what extending a run of D ops costs here
        const int dc = last_row ? 0 : dc_y;
#define PG_DC_Y dc_y
#else
        const int dc = ring[5 * AL_RING + slot];
#define PG_DC_Y dc
#endif
        const int num = x0 * ring[slot] + x1 * ring[AL_RING + slot] + x2 * ring[2 * AL_RING + slot] + x3 * ring[3 * AL_RING + slot] +
                        xa * ring[4 * AL_RING + slot] + xg * PG_DC_Y;
#undef PG_DC_Y
        const int diag = h_diag + pg_div(num, dv);
#if PG_ENDGAP
        const bool last_col = c == Ci - 1;                   // its I ops are the trailing ones: free
        const int xcost = last_col ? 0 : ic;
#if PG_POSGAP
#define AL_OPEN_D (last_row ? 0 : ring[6 * AL_RING + slot])
#define AL_OPEN_I (last_col ? 0 : oxic)
#else
#define AL_OPEN_D (last_row ? 0 : AL_OPEN) + dc
#define AL_OPEN_I (last_col ? 0 : AL_OPEN) + xcost
#endif
#else
        const int xcost = ic;
#if PG_POSGAP
#define AL_OPEN_D ring[6 * AL_RING + slot]
#define AL_OPEN_I oxic
#else
#define AL_OPEN_D AL_OPEN + dc
#define AL_OPEN_I AL_OPEN + xcost
#endif
#endif
#include "al_cell.inc"
#undef AL_OPEN_D
#undef AL_OPEN_I
        if (lane == 63 && s + 1 < n_strips) { row[2 * (c + 1)] = h; row[2 * (c + 1) + 1] = ii; }
      }
      acc |= cell << (4 * (t & 7));
      if ((t & 7) == 7 || t == T - 1) { tbs[(unsigned)((t >> 3) * 64 + lane)] = acc; acc = 0; }
    }
    WAVE_SYNC_GLOBAL();                                      // the row buffer and the traceback, written by every lane, read by lane 0
  }
  score = ni > 0 ? __shfl(score, (ni - 1) & 63) : row[2 * Ci];
  constexpr bool kBand = false;                              // (the full matrix: every strip starts at column 0)
  constexpr int dlo = 0;
#include "al_walk.inc"
}
#undef PG_RING_PLANES
#undef PG_OPEN_ROW0
#undef PG_OPEN_COL0
