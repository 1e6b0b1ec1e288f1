// k_prog_band_widths (k_prog_band.inc's header) and its form for position-specific opens, k_prog_band_widths_posgap (star_align.py,
// "Position gaps", band): one text, included twice (DESIGN.md §3a).  The includer provides PG_WIDTHS_KERNEL, the kernel's name, and
// PG_POSGAP: 0 expands to the tokens the kernel had when it stood in k_prog_band.inc.  1: a path that leaves the band pays at most
// oy = max_j Oc[j] (Y's seventh plane) and ox = max_i Ox[i] (pg_div over X's gap plane; 0 when n = 0) for its two runs, both
// reduced like SB, in place of 2 * AL_OPEN.
// PG_ENDGAP (with PG_POSGAP 0 only: k_prog_band_widths_endgap; star_align.py, "Free end gaps", band): 0 expands to those tokens.
// 1: B'_j = max(B_j, 0) is both the column's share of SB' and its loss (0 .. 1 280), X's side and the opens do not count:
// U(w) = SB' - LY'(max(0, D) + w + 1).  Only the first six planes of Y's profile are read, so profiles of kind 0 and 2 both serve.
__global__ void __launch_bounds__(PG_THREADS) PG_WIDTHS_KERNEL(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                                 const int32_t *xcols, long long xcols_words, const int64_t *pairs,
                                                                 int n_pairs, const int32_t *out, int64_t *bounds, int32_t *status) {
  SHARED(uint32_t, hy, PB_LOSS_BINS);
  SHARED(long long, sy, PB_LOSS_BINS);
#if !PG_ENDGAP
  SHARED(uint32_t, hx, PB_INS_BINS);
  SHARED(long long, sx, PB_INS_BINS);
#endif
  SHARED(long long, part, 2 * PG_WAVES);
#if PG_POSGAP
  SHARED(int, opens, 2 * PG_WAVES);
#endif
  const long long p = BLOCK_ID;
  const int64_t *PT = pairs + MPRG_PG_BAND_PAIR_FIELDS * p;
  const long long leaf = PT[0], xoff = PT[1], n = PT[2], RX = PT[5];
  int st = MPRG_AL_OK;
  long long C = 0, poff = 0;
  if (leaf < 0 || leaf >= n_leaves) st = MPRG_AL_BAD_INPUT;
  else {
    C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
    poff = leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
    if (C < 1 || n < 0 || leaves[MPRG_AL_LEAF_FIELDS * leaf + 1] < 1 || RX < 1 || RX > PG_MAX_ROWS || out[3 * p] != MPRG_AL_OK)
      st = MPRG_AL_BAD_INPUT;                                // (pass 1 refused the merge: there is no S0)
    else if (n + C >= AL_MAX_CELLS_SUM) st = MPRG_AL_TOO_LONG;
    else if (xoff < 0 || xoff > xcols_words || 7 * n > xcols_words - xoff) st = MPRG_AL_NO_SPACE;
  }
  ONE_THREAD status[p] = st;
  if (st != MPRG_AL_OK) return;                              // (the whole workgroup)
  PAR_FOR(k, PB_LOSS_BINS) hy[k] = 0;
#if !PG_ENDGAP
  PAR_FOR(k, PB_INS_BINS) hx[k] = 0;
#endif
  BARRIER();
  const int32_t *P = profile + poff;
  long long sb = 0;
#if PG_POSGAP
  int oy = AL_OPEN, ox = n > 0 ? AL_OPEN : 0;                // (every Oc and Ox is at least AL_OPEN)
  const PgDiv dv = pg_div_make(RX);
#endif
  PAR_FOR(j, C) {
    const int dc = P[5 * C + j];
    int b = dc;
#pragma unroll
    for (int x = 0; x < 5; ++x) { const int v = P[x * C + j]; b = v > b ? v : b; }
#if PG_ENDGAP
    b = b > 0 ? b : 0;
    sb += b;
    const int loss = b;                                      // 0 .. 1 280: a skipped column, charged or free, contributes at most 0
#else
    sb += b;
    const int loss = b - dc;                                 // 0 .. 1 920 for the planes k_prog_columns writes
#endif
    ATOMIC_ADD(&hy[loss < 0 ? 0 : loss > 1920 ? 1920 : loss], 1u);
#if PG_POSGAP
    const int oc = P[6 * C + j];
    oy = oc > oy ? oc : oy;
#endif
  }
#if !PG_ENDGAP
  PAR_FOR(i, n) {
    const int ins = -xcols[xoff + 6 * n + i];                // 0 .. 640
    ATOMIC_ADD(&hx[ins < 0 ? 0 : ins > 640 ? 640 : ins], 1u);
#if PG_POSGAP
    const int oi = pg_div(AL_OPEN * ((int)RX - xcols[xoff + 5 * n + i]), dv);
    ox = oi > ox ? oi : ox;
#endif
  }
#endif
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sb += __shfl_xor(sb, d);
#if PG_POSGAP
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int y = __shfl_xor(oy, d), x = __shfl_xor(ox, d);
    oy = y > oy ? y : oy;
    ox = x > ox ? x : ox;
  }
  if (wave_lane() == 0) { opens[2 * wave_id()] = oy; opens[2 * wave_id() + 1] = ox; }   // (read behind the barriers below)
#endif
  BARRIER();                                                 // the histograms are complete
  pb_cumulate<PB_LOSS_BINS / PG_THREADS>(hy, sy, part);
#if !PG_ENDGAP
  pb_cumulate<PB_INS_BINS / PG_THREADS>(hx, sx, part);
#endif
  if (wave_lane() == 0) part[wave_id()] = sb;                // (part was last read before pb_cumulate's closing barrier)
  BARRIER();
  ONE_THREAD {
    long long SB = 0;
    for (int w = 0; w < PG_WAVES; ++w) SB += part[w];
#if PG_POSGAP
    int open2 = 0;                                           // oy + ox: at most 0, at least 2 * AL_OPEN
    {
      int my = opens[0], mx = opens[1];
      for (int w = 1; w < PG_WAVES; ++w) { my = opens[2 * w] > my ? opens[2 * w] : my; mx = opens[2 * w + 1] > mx ? opens[2 * w + 1] : mx; }
      open2 = my + mx;
    }
#define PG_TWO_OPENS open2
#else
#define PG_TWO_OPENS 2 * AL_OPEN
#endif
    const long long S0 = out[3 * p + 1], delta = C - n, dpos = delta > 0 ? delta : 0, dneg = delta < 0 ? delta : 0;
    long long lo = 0, hi = n < C ? n : C;                    // the smallest w with U(w) < S0; none: min(n, C), both sides at the edge
    while (lo < hi) {
      const long long w = (lo + hi) >> 1;
#if PG_ENDGAP
      const long long U = SB - pb_smallest(hy, sy, PB_LOSS_BINS, dpos + w + 1);
#else
      const long long U = SB - pb_smallest(hy, sy, PB_LOSS_BINS, dpos + w + 1) - pb_smallest(hx, sx, PB_INS_BINS, w + 1 - dneg) + PG_TWO_OPENS;
#endif
      if (U < S0) hi = w; else lo = w + 1;
    }
#undef PG_TWO_OPENS
    bounds[2 * p] = SB;
    bounds[2 * p + 1] = lo;
  }
}
