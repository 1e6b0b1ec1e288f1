// ---------------------------------------------------------------------------------------------------------------
// K-R  leave-one-out refinement of `from_msa --unaligned --refine` (make_prg_amd/from_msa/star_align.py holds the spec,
//      "Refinement"; DESIGN.md §3b).  The realignment itself is k_align_pairs' / k_align_pairs_banded's (K-A) over the profiles
//      written here, the merge k_star_merge_*'s (K-S) with C = W.  Integers only.
//
// All four kernels read an MSA as mprg_star_merge_rows left it: R rows of W ASCII bytes (ACGT-RYKMSWN), row-major.
// k_refine_counts: one workgroup per (locus, 256-column tile), thread = column, the rows walked in order (a row of the tile is
//   256 contiguous bytes: coalesced; the access pattern of k_align_profiles), the five counts A C G T '-' in registers.  The left
//   neighbour of a cell (is it a run start?) comes from the lane below by a shuffle, for lane 0 of a wavefront from memory.
//   Writes the counts (5 planes of W int32), the keep flag (g < R), and adds the tile's part of the objective S and its kept
//   columns to the locus's two int64: a reduction over the workgroup, then ONE 64-bit integer atomic each (order-independent).
// k_refine_profiles: one workgroup per (row, 256-column tile): the profile of the MSA WITHOUT that row from the counts and the
//   row's own cell, with k_align_profiles' formulas and its truncating division, by R - 1.  6 planes of W int32.
// k_refine_scan: one wavefront per locus: dest[c] = kept columns before c, new_width = their number.
// k_refine_compact_rows: one wavefront per row: the kept cells of the row to their new places; every output byte written once.
// ---------------------------------------------------------------------------------------------------------------
#define RF_THREADS 256
#define RF_WAVES (RF_THREADS / 64)

// a locus's fields against the buffers: R x W cells inside the text, W columns inside the column tables
MPRG_DEV bool rf_locus_ok(const int64_t *loci, int n_loci, long long l, long long text_bytes, long long n_cols, long long &toff,
                          long long &R, long long &W, long long &coff) {
  if (l < 0 || l >= n_loci) return false;
  const int64_t *L = loci + MPRG_RF_LOCUS_FIELDS * l;
  toff = L[0]; R = L[1]; W = L[2]; coff = L[3];
  if (R < 1 || W < 1 || R > 0x7fffffffLL || W > 0x7fffffffLL || toff < 0 || toff > text_bytes || coff < 0 || coff > n_cols) return false;
  return R <= (text_bytes - toff) / W && W <= n_cols - coff;
}

__global__ void __launch_bounds__(RF_THREADS) k_refine_counts(const uint8_t *text, long long text_bytes, const int64_t *loci, int n_loci,
                                                              const int32_t *work, int32_t *counts, uint8_t *keep, long long n_cols,
                                                              int64_t *sums, int32_t *status) {
  SHARED(long long, red, 2 * RF_WAVES);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long l = wk[0], tile = wk[1];
  long long toff = 0, R = 0, W = 0, coff = 0;
  const bool ok = rf_locus_ok(loci, n_loci, l, text_bytes, n_cols, toff, R, W, coff) && tile >= 0 && tile * 256 < W;
  if (threadIdx.x == 0) status[BLOCK_ID] = ok ? MPRG_RF_OK : MPRG_RF_BAD_LOCUS;
  if (!ok) return;                                           // (the whole workgroup)
  const long long c = tile * 256 + (long long)threadIdx.x;
  const bool in = c < W;
  const int lane = wave_lane();
  int cnt[5] = {0, 0, 0, 0, 0};
  long long starts = 0;
  for (long long r = 0; r < R; ++r) {
    const uint8_t *row = text + toff + r * W;
    const unsigned ch = in ? (unsigned)row[c] : (unsigned)'A';
    unsigned left = __shfl_up(ch, 1);
    if (lane == 0) left = in && c > 0 ? (unsigned)row[c - 1] : (unsigned)'A';
    cnt[0] += ch == 'A'; cnt[1] += ch == 'C'; cnt[2] += ch == 'G'; cnt[3] += ch == 'T'; cnt[4] += ch == '-';
    starts += in && ch == '-' && left != '-';
  }
  long long part = 0, kept = 0;
  if (in) {
    const long long a = cnt[0], b = cnt[1], g = cnt[2], t = cnt[3], gap = cnt[4];
    const long long same = (a * (a - 1) + b * (b - 1) + g * (g - 1) + t * (t - 1)) / 2;
    const long long diff = a * b + a * g + a * t + b * g + b * t + g * t;
    part = 2 * (20 * same - 9 * diff - 10 * gap * (R - gap));
    kept = gap < R;
    int32_t *o = counts + 5 * coff + c;
#pragma unroll
    for (int x = 0; x < 5; ++x) o[(long long)x * W] = cnt[x];
    keep[coff + c] = (uint8_t)kept;
  }
  part -= 11 * (R - 1) * starts;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { part += __shfl_xor(part, d); kept += __shfl_xor(kept, d); }
  if (lane == 0) { red[2 * wave_id()] = part; red[2 * wave_id() + 1] = kept; }
  BARRIER();
  if (threadIdx.x == 0) {
    long long s = 0, k = 0;
    for (int w = 0; w < RF_WAVES; ++w) { s += red[2 * w]; k += red[2 * w + 1]; }
    ATOMIC_ADD((unsigned long long *)(sums + 2 * l), (unsigned long long)s);
    ATOMIC_ADD((unsigned long long *)(sums + 2 * l + 1), (unsigned long long)k);
  }
}

__global__ void __launch_bounds__(RF_THREADS) k_refine_profiles(const uint8_t *text, long long text_bytes, const int64_t *loci, int n_loci,
                                                                const int32_t *counts, long long n_cols, const int64_t *rows, int n_rows,
                                                                const int32_t *work, int32_t *profile, long long profile_words,
                                                                int32_t *status) {
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long q = wk[0], tile = wk[1];
  long long toff = 0, R = 0, W = 0, coff = 0, r = 0, poff = 0;
  int st = MPRG_RF_OK;
  if (q < 0 || q >= n_rows) st = MPRG_RF_BAD_ROW;
  else {
    const int64_t *Q = rows + MPRG_RF_ROW_FIELDS * q;
    r = Q[1]; poff = Q[2];
    if (!rf_locus_ok(loci, n_loci, Q[0], text_bytes, n_cols, toff, R, W, coff)) st = MPRG_RF_BAD_LOCUS;
    else if (R < 2 || r < 0 || r >= R || tile < 0 || tile * 256 >= W) st = MPRG_RF_BAD_ROW;
    else if (poff < 0 || poff > profile_words || 6 * W > profile_words - poff) st = MPRG_RF_NO_SPACE;
  }
  if (threadIdx.x == 0) status[BLOCK_ID] = st;
  if (st != MPRG_RF_OK) return;                              // (the whole workgroup)
  const long long c = tile * 256 + (long long)threadIdx.x;
  if (c >= W) return;
  const unsigned ch = text[toff + r * W + c];
  const int32_t *in = counts + 5 * coff + c;
  long long cnt[5];
#pragma unroll
  for (int x = 0; x < 5; ++x) cnt[x] = in[(long long)x * W];
  cnt[0] -= ch == 'A'; cnt[1] -= ch == 'C'; cnt[2] -= ch == 'G'; cnt[3] -= ch == 'T'; cnt[4] -= ch == '-';
  const long long acgt = cnt[0] + cnt[1] + cnt[2] + cnt[3], gap = cnt[4], pl_rows = R - 1, pl_stride = W;
  constexpr int kind = 0;                                    // (the MSA without the row is a Y side)
  int32_t *o = profile + poff + c;
#include "al_planes.inc"
}

__global__ void __launch_bounds__(RF_THREADS) k_refine_scan(const int64_t *loci, int n_loci, long long text_bytes, const uint8_t *keep,
                                                            long long n_cols, int32_t *dest, int64_t *new_width) {
  const long long l = (long long)BLOCK_ID * RF_WAVES + wave_id();
  if (l >= n_loci) return;                                   // (a whole wavefront)
  long long toff = 0, R = 0, W = 0, coff = 0;
  if (!rf_locus_ok(loci, n_loci, l, text_bytes, n_cols, toff, R, W, coff)) { if (wave_lane() == 0) new_width[l] = -1; return; }
  int carry = 0;
  for (long long c0 = 0; c0 < W; c0 += WAVE) {
    const long long c = c0 + wave_lane();
    const int v = c < W ? (keep[coff + c] != 0) : 0;
    const int incl = wave_scan_incl(v);
    if (c < W) dest[coff + c] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (wave_lane() == 0) new_width[l] = carry;
}

__global__ void __launch_bounds__(RF_THREADS) k_refine_compact_rows(const uint8_t *text, long long text_bytes, const int64_t *loci,
                                                                    int n_loci, const uint8_t *keep, long long n_cols, const int32_t *dest,
                                                                    const int64_t *new_width, const int64_t *rows, int n_rows, uint8_t *out,
                                                                    long long out_bytes, int32_t *status) {
  const long long q = (long long)BLOCK_ID * RF_WAVES + wave_id();
  if (q >= n_rows) return;                                   // (a whole wavefront)
  const int64_t *Q = rows + MPRG_RF_ROW_FIELDS * q;
  const long long r = Q[1], ooff = Q[2];
  long long toff = 0, R = 0, W = 0, coff = 0;
  int st = MPRG_RF_OK;
  if (!rf_locus_ok(loci, n_loci, Q[0], text_bytes, n_cols, toff, R, W, coff)) st = MPRG_RF_BAD_LOCUS;
  else {
    const long long Wn = new_width[Q[0]];
    if (r < 0 || r >= R || Wn < 0 || Wn > W) st = MPRG_RF_BAD_ROW;
    else if (ooff < 0 || ooff > out_bytes || (Wn > 0 && R > (out_bytes - ooff) / Wn)) st = MPRG_RF_NO_SPACE;
    else {
      const uint8_t *src = text + toff + r * W;
      uint8_t *o = out + ooff + r * Wn;
      for (long long c = wave_lane(); c < W; c += WAVE)
        if (keep[coff + c]) {
          const long long d = dest[coff + c];
          if (d >= 0 && d < Wn) o[d] = src[c];               // (the scan's dest is always in range; a foreign table cannot write outside)
        }
    }
  }
  if (wave_lane() == 0) status[q] = st;
}
