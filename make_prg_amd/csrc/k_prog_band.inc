// ---------------------------------------------------------------------------------------------------------------
// K-P banded (`from_msa --unaligned --progressive --band`; the spec, the certificate and its proof:
//      make_prg_amd/from_msa/star_align.py, "Progressive, band"; DESIGN.md §3b): the profile-profile DP of a merge over the cells
//      of the diagonals dlo <= j - i <= dhi only, and the certified half-width of every merge of a launch, found on the device.
//
// (The three kernels' texts are pg_pairs_band.inc and pg_band_widths.inc, each included twice: as the kernels below and as their
//   _posgap forms, the merges with position-specific opens; the pair kernel twice more as the _endgap forms of both and the widths
//   kernel once more as k_prog_band_widths_endgap, the merges with free end gaps.)
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

#define PG_ENDGAP 0
#define PG_PAIRS_KERNEL k_align_profile_pairs_banded
#define PG_POSGAP 0
#include "pg_pairs_band.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#define PG_PAIRS_KERNEL k_align_profile_pairs_posgap_banded
#define PG_POSGAP 1
#include "pg_pairs_band.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#undef PG_ENDGAP
// ... and with free end gaps (star_align.py, "Free end gaps"), for both forms of the open
#define PG_ENDGAP 1
#define PG_PAIRS_KERNEL k_align_profile_pairs_endgap_banded
#define PG_POSGAP 0
#include "pg_pairs_band.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#define PG_PAIRS_KERNEL k_align_profile_pairs_posgap_endgap_banded
#define PG_POSGAP 1
#include "pg_pairs_band.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#undef PG_ENDGAP

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

#define PG_ENDGAP 0
#define PG_WIDTHS_KERNEL k_prog_band_widths
#define PG_POSGAP 0
#include "pg_band_widths.inc"
#undef PG_WIDTHS_KERNEL
#undef PG_POSGAP
#define PG_WIDTHS_KERNEL k_prog_band_widths_posgap
#define PG_POSGAP 1
#include "pg_band_widths.inc"
#undef PG_WIDTHS_KERNEL
#undef PG_POSGAP
#undef PG_ENDGAP
// ... and for free end gaps: no open enters its bound, so one kernel serves both forms of the open
#define PG_ENDGAP 1
#define PG_WIDTHS_KERNEL k_prog_band_widths_endgap
#define PG_POSGAP 0
#include "pg_band_widths.inc"
#undef PG_WIDTHS_KERNEL
#undef PG_POSGAP
#undef PG_ENDGAP
