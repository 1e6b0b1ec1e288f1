// ---------------------------------------------------------------------------------------------------------------
// K-P banded (`from_msa --unaligned --progressive --band`; the spec, the certificate and its proof:
//      make_prg_amd/from_msa/star_align.py, "Progressive, band"; DESIGN.md §3b): the profile-profile DP of a merge over the cells
//      of the diagonals dlo <= j - i <= dhi only, and the certified half-width of every merge of a launch, found on the device.
//
// k_align_profile_pairs_banded: k_align_profile_pairs' cell (X's six counts and Ic in registers, six multiply-adds, pg_div) with
//   k_align_pairs_banded's geometry, a kernel of its own but for the cell and the walk back (al_cell.inc, al_walk.inc).  Strip s (rows
//   i0 + 1 .. i0 + rows) sweeps columns cs + 1 .. min(C, i0 + rows + dhi), cs = max(0, i0 + dlo); a lane computes only where its
//   row's band holds its column and hands AL_NEG to the lane below everywhere else (H[i][0] = open + the Ic of rows 1 .. i where
//   column 0 is in the row's band).  Row buffer: W = dhi - dlo + 1 (H, I) slots, row i0 keeps column j at slot j - (i0 + dlo).
//   Ring and traceback are indexed by the STEP: ring slot (t - l) & 127, traceback dword (s * nst8 + t / 8) * 64 + l with nst8 =
//   ceil((min(C, W + 63) + 63) / 8).  The AL_NEG argument is k_align_pairs_banded's: Ic and Dc are >= -640 like its penalties, and
//   the H of every in-band cell is a real score (its diagonal predecessor lies on the same diagonal).
// k_prog_band_widths: one workgroup per merge over the planes k_prog_columns wrote.  Two LDS histograms: loss_j = B_j - Dc[j]
//   (0 .. 1 920) over Y's columns with B_j = max(P[j][A, C, G, T, amb], Dc[j]), ins_i = -Ic[i] (0 .. 640) over X's; both turned
//   into cumulative counts and sums (eight, three bins per thread, a wave scan, four partial sums through LDS), SB = sum_j B_j in
//   int64.  LY(k), the sum of the k smallest losses, is then cs[v - 1] + (k - cc[v - 1]) v for the bin v that holds the k-th
//   smallest (a binary search over the cumulative counts); LX likewise.  U(w) = SB - LY(max(0, D) + w + 1) - LX(w + 1 - min(0, D))
//   - 1 408 falls with w, so thread 0 finds w* = the smallest w in [0, min(n, C)] with U(w) < S0 by bisection (min(n, C) when
//   there is none: both sides at the matrix's edge).  {SB, w*} per merge is all the host downloads.
// ---------------------------------------------------------------------------------------------------------------
#define PB_LOSS_BINS 2048                      // loss_j <= 1 280 + 640 = 1 920; eight bins per thread
#define PB_INS_BINS 768                        // ins_i <= 640; three bins per thread

__global__ void __launch_bounds__(AL_THREADS) k_align_profile_pairs_banded(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                                           const int32_t *xcols, long long xcols_words,
                                                                           const int64_t *pairs, int n_pairs, int32_t *ws,
                                                                           long long ws_words, uint8_t *ops, long long ops_bytes,
                                                                           int32_t *out) {
  SHARED(int32_t, ring_all, AL_WAVES * 6 * AL_RING);
  const int lane = wave_lane();
  const long long p = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (p >= n_pairs) return;                                   // (a whole wavefront: nothing below waits for the others)
  int32_t *ring = ring_all + wave_id() * 6 * AL_RING;
  const int64_t *PT = pairs + MPRG_PG_BAND_PAIR_FIELDS * p;
  const long long leaf = PT[0], xoff = PT[1], n = PT[2], wsoff = PT[3], opoff = PT[4], RX = PT[5];
  long long blo = PT[6], bhi = PT[7];
  int32_t *o = out + 3 * p;
  int status = MPRG_AL_OK;
  long long C = 0, poff = 0;
  if (leaf < 0 || leaf >= n_leaves) status = MPRG_AL_BAD_INPUT;
  else {
    C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
    poff = leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
    if (C < 1 || n < 0 || leaves[MPRG_AL_LEAF_FIELDS * leaf + 1] < 1 || RX < 1 || RX > PG_MAX_ROWS) status = MPRG_AL_BAD_INPUT;
    else if (n + C >= AL_MAX_CELLS_SUM) status = MPRG_AL_TOO_LONG;
    else if (blo > 0 || blo > C - n || bhi < 0 || bhi < C - n) status = MPRG_AL_BAD_INPUT;      // the band must hold both corners
    else {
      blo = blo < -n ? -n : blo;
      bhi = bhi > C ? C : bhi;
      if (wsoff < 0 || (wsoff & 63) || wsoff + al_band_ws_words(n, C, blo, bhi) > ws_words || opoff < 0 || opoff + n + C > ops_bytes ||
          xoff < 0 || xoff > xcols_words || 7 * n > xcols_words - xoff)
        status = MPRG_AL_NO_SPACE;
    }
  }
  if (status != MPRG_AL_OK) {
    if (lane == 0) { o[0] = status; o[1] = 0; o[2] = 0; }
    return;
  }
  const int32_t *P = profile + al_uniform(poff);
  const int Ci = (int)al_uniform(C), ni = (int)al_uniform(n), dlo = (int)al_uniform(blo), dhi = (int)al_uniform(bhi);
  const int W = dhi - dlo + 1;
  const int32_t *X = xcols + al_uniform(xoff);
  const PgDiv dv = pg_div_make(al_uniform(RX));
  const long long wsoff_u = al_uniform(wsoff);
  int32_t *row = ws + wsoff_u;                               // row[2k] = H, row[2k + 1] = I of the row above the strip (row i0), column i0 + dlo + k
  uint32_t *tb = (uint32_t *)(ws + wsoff_u + ((2 * (long long)W + 63) / 64) * 64);
  const long long nst8 = ((W + 63 < Ci ? W + 63 : Ci) + 63 + 7) / 8;
  // row 0, columns 0 .. dhi: H[0][J] = D[0][J] = open + the gap costs of columns < J
  int carry = 0;
  for (int c0 = 0; c0 < dhi; c0 += 64) {
    const int c = c0 + lane;
    const int incl = wave_scan_incl(c < dhi ? P[(unsigned)(5 * Ci + c)] : 0) + carry;
    if (c < dhi) { row[2 * (c + 1 - dlo)] = AL_OPEN + incl; row[2 * (c + 1 - dlo) + 1] = AL_NEG; }
    carry = __shfl(incl, 63);
  }
  if (lane == 0) { row[2 * (-dlo)] = 0; row[2 * (-dlo) + 1] = AL_NEG; }
  WAVE_SYNC_GLOBAL();
  int score = AL_NEG;
  int ic_before = 0;                                         // the Ic of all rows above the strip
  const int n_strips = (ni + 63) / 64;
  for (int s = 0; s < n_strips; ++s) {
    const int i0 = s * 64, r = i0 + lane, rows = ni - i0 < 64 ? ni - i0 : 64;
    const bool valid = r < ni;
    // this lane's X column: the counts of A C G T, of the ambiguity codes, of '-', and what the column alone costs
    // (one base and 32-bit offsets, 7 n < 7 * 10^6: a base per plane would hold seven scalar register pairs through the sweep)
    const int x0 = valid ? X[(unsigned)r] : 0, x1 = valid ? X[(unsigned)(ni + r)] : 0;
    const int x2 = valid ? X[(unsigned)(2 * ni + r)] : 0, x3 = valid ? X[(unsigned)(3 * ni + r)] : 0;
    const int xa = valid ? X[(unsigned)(4 * ni + r)] : 0, xg = valid ? X[(unsigned)(5 * ni + r)] : 0;
    const int ic = valid ? X[(unsigned)(6 * ni + r)] : 0;
    const int hb = AL_OPEN + wave_scan_incl(ic) + ic_before;  // H[r + 1][0]: open + the Ic of rows 1 .. r + 1
    const int cs = i0 + dlo > 0 ? i0 + dlo : 0;             // the strip's first column, 0-based
    const int jtop = i0 + dhi < Ci ? i0 + dhi : Ci;         // the last column of row i0 inside the band
    const int jend = i0 + rows + dhi < Ci ? i0 + rows + dhi : Ci;   // the strip's last column, 1-based
    const int d0 = cs - r - dlo;                            // 0-based column c = cs + t - lane of this lane's row (r + 1) lies on diagonal c - r:
                                                            // inside the band where 0 <= d0 + t - lane <= dhi - dlo (and 0 <= c < C)
    const bool col0 = r + 1 + dlo <= 0;                     // column 0 of this lane's row lies inside the band
    int h_left = col0 ? hb : AL_NEG, d_left = AL_NEG;       // H, D of this lane's row, the column to the left of its first one
    int h_out = col0 && cs == lane ? hb : AL_NEG, i_out = AL_NEG;   // what the lane below reads next step: here of column cs - 1 - lane
    int h_up_prev = AL_NEG;                                  // H of the row above, one column to the left: the diagonal
    if (lane == 0) h_up_prev = cs == 0 ? (i0 == 0 ? 0 : AL_OPEN + ic_before) : row[0];   // (cs > 0: column cs = i0 + dlo of row i0, its first inside the band)
    ic_before = __shfl(hb, 63) - AL_OPEN;
    uint32_t acc = 0;
    uint32_t *tbs = tb + (long long)s * nst8 * 64;           // the strip's traceback: wave-uniform bases, 32-bit lane offsets
    const int T = jend - cs + rows - 1;
    for (int t = 0; t < T; ++t) {
      if ((t & 63) == 0) {                                   // the ring takes columns cs + [t, t + 64): the block 128 before is done with
        WAVE_SYNC();
#pragma unroll
        for (int k = 0; k < 6; ++k)
          ring[k * AL_RING + ((t + lane) & (AL_RING - 1))] = cs + t + lane < Ci ? P[(unsigned)(k * Ci + cs + t + lane)] : 0;
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
        const int dc = ring[5 * AL_RING + slot];
        const int num = x0 * ring[slot] + x1 * ring[AL_RING + slot] + x2 * ring[2 * AL_RING + slot] + x3 * ring[3 * AL_RING + slot] +
                        xa * ring[4 * AL_RING + slot] + xg * dc;
        const int diag = h_diag + pg_div(num, dv);
        const int xcost = ic;
#include "al_cell.inc"
        if (lane == 63 && s + 1 < n_strips) { const int k = c + 1 - (i0 + 64 + dlo); row[(unsigned)(2 * k)] = h; row[(unsigned)(2 * k + 1)] = ii; }
      } else {
        h_out = c == -1 && col0 ? hb : AL_NEG;               // outside the band: minus infinity, never a stale or an accumulated value
        i_out = AL_NEG;
      }
      acc |= cell << (4 * (t & 7));
      if ((t & 7) == 7 || t == T - 1) { tbs[(unsigned)((t >> 3) * 64 + lane)] = acc; acc = 0; }
    }
    WAVE_SYNC_GLOBAL();                                      // the row buffer and the traceback, written by every lane, read by lane 0
  }
  score = ni > 0 ? __shfl(score, (ni - 1) & 63) : row[2 * (Ci - dlo)];
  constexpr bool kBand = true;
#include "al_walk.inc"
}

// cnt[0 .. PER * PG_THREADS) (a histogram over values = bin indices) into cumulative counts, in place, and cumulative sums of
// count * value; every thread of the workgroup calls it; part: 2 * PG_WAVES long long of LDS
template <int PER> MPRG_DEV void pb_cumulate(uint32_t *cnt, long long *sum, long long *part) {
  const int b0 = (int)threadIdx.x * PER;
  long long c = 0, s = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) { c += cnt[b0 + q]; s += (long long)cnt[b0 + q] * (b0 + q); }
  const long long ci = wave_scan_incl_ll(c), si = wave_scan_incl_ll(s);
  if (wave_lane() == WAVE - 1) { part[2 * wave_id()] = ci; part[2 * wave_id() + 1] = si; }
  BARRIER();
  long long cb = ci - c, sb = si - s;
  for (int w = 0; w < wave_id(); ++w) { cb += part[2 * w]; sb += part[2 * w + 1]; }
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const long long x = cnt[b0 + q];
    cb += x; sb += x * (b0 + q);
    cnt[b0 + q] = (uint32_t)cb; sum[b0 + q] = sb;
  }
  BARRIER();
}
// the sum of the k smallest values of a histogram pb_cumulate went over (cc: cumulative counts, cs: cumulative sums, `bins` of
// them); k clamped to the number of values
MPRG_DEV long long pb_smallest(const uint32_t *cc, const long long *cs, int bins, long long k) {
  const long long total = cc[bins - 1];
  k = k > total ? total : k;
  if (k <= 0) return 0;
  int lo = 0, hi = bins - 1;                                 // the first bin v with cc[v] >= k: it holds the k-th smallest
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)cc[mid] >= k) hi = mid; else lo = mid + 1;
  }
  return lo == 0 ? 0 : cs[lo - 1] + (k - (long long)cc[lo - 1]) * lo;
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_band_widths(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                                 const int32_t *xcols, long long xcols_words, const int64_t *pairs,
                                                                 int n_pairs, const int32_t *out, int64_t *bounds, int32_t *status) {
  SHARED(uint32_t, hy, PB_LOSS_BINS);
  SHARED(long long, sy, PB_LOSS_BINS);
  SHARED(uint32_t, hx, PB_INS_BINS);
  SHARED(long long, sx, PB_INS_BINS);
  SHARED(long long, part, 2 * PG_WAVES);
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
  PAR_FOR(k, PB_INS_BINS) hx[k] = 0;
  BARRIER();
  const int32_t *P = profile + poff;
  long long sb = 0;
  PAR_FOR(j, C) {
    const int dc = P[5 * C + j];
    int b = dc;
#pragma unroll
    for (int x = 0; x < 5; ++x) { const int v = P[x * C + j]; b = v > b ? v : b; }
    sb += b;
    const int loss = b - dc;                                 // 0 .. 1 920 for the planes k_prog_columns writes
    ATOMIC_ADD(&hy[loss < 0 ? 0 : loss > 1920 ? 1920 : loss], 1u);
  }
  PAR_FOR(i, n) {
    const int ins = -xcols[xoff + 6 * n + i];                // 0 .. 640
    ATOMIC_ADD(&hx[ins < 0 ? 0 : ins > 640 ? 640 : ins], 1u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sb += __shfl_xor(sb, d);
  BARRIER();                                                 // the histograms are complete
  pb_cumulate<PB_LOSS_BINS / PG_THREADS>(hy, sy, part);
  pb_cumulate<PB_INS_BINS / PG_THREADS>(hx, sx, part);
  if (wave_lane() == 0) part[wave_id()] = sb;                // (part was last read before pb_cumulate's closing barrier)
  BARRIER();
  ONE_THREAD {
    long long SB = 0;
    for (int w = 0; w < PG_WAVES; ++w) SB += part[w];
    const long long S0 = out[3 * p + 1], delta = C - n, dpos = delta > 0 ? delta : 0, dneg = delta < 0 ? delta : 0;
    long long lo = 0, hi = n < C ? n : C;                    // the smallest w with U(w) < S0; none: min(n, C), both sides at the edge
    while (lo < hi) {
      const long long w = (lo + hi) >> 1;
      const long long U = SB - pb_smallest(hy, sy, PB_LOSS_BINS, dpos + w + 1) - pb_smallest(hx, sx, PB_INS_BINS, w + 1 - dneg) + 2 * AL_OPEN;
      if (U < S0) hi = w; else lo = w + 1;
    }
    bounds[2 * p] = SB;
    bounds[2 * p + 1] = lo;
  }
}
