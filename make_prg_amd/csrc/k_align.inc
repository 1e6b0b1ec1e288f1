// ---------------------------------------------------------------------------------------------------------------
// K-A  built-in profile aligner of `update --aligner builtin` (make_prg_amd/update/profile_align.py holds the spec;
//      DESIGN.md §Built-in aligner): new sequences aligned one by one against the profile of a leaf's alignment, a
//      global three-state (Gotoh) DP in int32, scores in 1/64 row.
//
// k_align_profiles: one workgroup per (leaf, 256-column tile), thread = column, the leaf's rows walked in order (a row of
//   the tile is 256 contiguous bytes: coalesced), the five counts A C G T '-' in registers.  Writes the leaf's profile as
//   6 x C int32 at profile + poff: rows 0-3 the score of A C G T against the column, row 4 that of R Y K M S W N, row 5 the
//   cost Dc of a gap in the new sequence there.
// k_align_pairs: one wavefront per (leaf, new sequence) pair, AL_WAVES pairs per workgroup, no barriers between them.  The
//   64 lanes own 64 consecutive residues of the sequence (a strip); at step t lane l fills cell (i0 + l, column t - l): the
//   row above comes from lane l - 1 by a shuffle (lane 0: from the strip above, a row buffer in the workspace that lane 63
//   of that strip wrote), the profile of the columns in flight from a 128-column LDS ring per wavefront (consecutive lanes
//   on consecutive columns).  A cell's traceback is 4 bits, a lane packs eight steps per dword, so every store is a 256-byte
//   row.  Lane 0 then walks the traceback back from (n, C) and writes the ops (reversed) and the score.
//   The cell's recurrence (al_cell.inc; its two open terms are AL_OPEN_D and AL_OPEN_I, here the fixed open and the column) and
//   the walk back (al_walk.inc) are written once for the sweep kernels (this one,
//   k_align_pairs_banded below, k_align_profile_pairs in k_prog.inc, k_align_profile_pairs_banded in k_prog_band.inc), a column's
//   counts (al_counts.inc) and its planes (al_planes.inc) once for the kernels that write profiles (k_align_profiles,
//   k_prog_columns, k_prog_columns_weighted, and k_refine_profiles for the planes).  All are included as text: an inlined function
//   body shared between kernels compiles them to other instructions, text that expands to the same tokens cannot (DESIGN.md §3a).
//   The kernel's own text is al_pairs.inc, included below once as k_align_pairs and once, with AL_ENDGAP 1, as k_align_pairs_endgap
//   (star_align.py, "Free end pairs"); k_align_pairs_banded's is al_pairs_band.inc, likewise.
// ---------------------------------------------------------------------------------------------------------------
#define AL_THREADS 256
#define AL_WAVES (AL_THREADS / 64)
#define AL_RING 128
#define AL_NEG (-2147483647 - 1 + 65536)      // "minus infinity": one penalty below it still fits int32, every real score is above it
#define AL_OPEN (-704)
#define AL_INS (-640)
#define AL_MAX_CELLS_SUM 1000000               // n + C must stay below this: |score| < (n + C) * (640 + 704) < 2^31

KERNEL(k_align_profiles, const uint8_t *cells, const int64_t *leaves, const int32_t *work, int32_t *profile) {
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const int64_t *L = leaves + MPRG_AL_LEAF_FIELDS * (long long)wk[0];
  const long long off = L[0], poff = L[3];
  const int R = (int)L[1], C = (int)L[2];
  PAR_FOR(tt, 256) {
    const int c = wk[1] * 256 + (int)tt;
    if (c >= C) continue;
#define AL_CELL(r) cells[off + (long long)(r) * C + c]
#define AL_WEIGHT(r) 1
#include "al_counts.inc"
#undef AL_CELL
#undef AL_WEIGHT
    const int pl_rows = R, pl_stride = C;
    constexpr int kind = 0;                                  // (a leaf is a Y side)
    int32_t *o = profile + poff + c;
#include "al_planes.inc"
  }
}

// int32 words of workspace a pair needs: the row buffer (H, I of C + 1 columns, rounded up to 64 words) + the traceback
// (ceil(n / 64) strips x ceil((C + 63) / 8) dwords x 64 lanes)
MPRG_DEV long long al_ws_words(long long n, long long C) {
  return ((2 * (C + 1) + 63) / 64) * 64 + ((n + 63) / 64) * ((C + 63 + 7) / 8) * 64;
}
MPRG_DEV int al_hb(long long i) { return i == 0 ? 0 : (int)(AL_OPEN + AL_INS * i); }     // H[i][0]

// k_align_pairs and k_align_pairs_endgap: one text (al_pairs.inc), the second with the free ends of "Free end pairs"
#define AL_PAIRS_KERNEL k_align_pairs
#define AL_ENDGAP 0
#include "al_pairs.inc"
#undef AL_PAIRS_KERNEL
#undef AL_ENDGAP
#define AL_PAIRS_KERNEL k_align_pairs_endgap
#define AL_ENDGAP 1
#include "al_pairs.inc"
#undef AL_PAIRS_KERNEL
#undef AL_ENDGAP

// ---------------------------------------------------------------------------------------------------------------
// K-A banded (`from_msa --unaligned --band`; the spec, the certificate and its proof: make_prg_amd/update/profile_align.py,
// "Band"): the same DP over the cells of the diagonals dlo <= j - i <= dhi only.  Every cell outside the band is AL_NEG in all
// three states and is never computed; the band holds (0, 0) and (n, C) (dlo <= min(0, C - n), dhi >= max(0, C - n): anything
// else is MPRG_AL_BAD_INPUT) and is clamped to the matrix ([-n, C]) before anything is sized by it.
//
// k_align_bounds: one wavefront per leaf over the profile k_align_profiles wrote: SB = sum_j B_j, B_j = max(max_x P[j][x], Dc[j]),
//   and min_j (B_j - Dc[j]), both int64: what the host's certificate needs.
// k_align_pairs_banded: k_align_pairs' wavefront-per-pair, 64-row-strip, anti-diagonal sweep, a kernel of its own but for the
//   cell and the walk back (al_cell.inc, al_walk.inc).  Strip s (rows i0 + 1 .. i0 + rows) sweeps columns cs + 1 .. min(C, i0 + rows +
//   dhi), cs = max(0, i0 + dlo): at step t lane l is at 0-based column cs + t - l and computes only where its row's band holds that
//   column; everywhere else it hands AL_NEG to the lane below (H[i][0] where column 0 is in the row's band), so no lane ever
//   reads a stale value.  Along a row the first in-band cell starts from (H[i][0], AL_NEG) or (AL_NEG, AL_NEG).  A gap state whose
//   two predecessors are outside the band is AL_NEG plus one open and one extension at most (>= AL_NEG - 1 344, int32 holds
//   AL_NEG - 65 536); the H of every in-band cell is a real score (its diagonal predecessor is on the same diagonal), so the next
//   cell's gap state is real again: no chain of penalties on AL_NEG.
//   Row buffer: W = dhi - dlo + 1 (H, I) slots; the row above strip s (row i0) keeps column j at slot j - (i0 + dlo).  Lane 0 reads
//   slot cs + t + 1 - (i0 + dlo) at step t (AL_NEG beyond min(C, i0 + dhi): the columns the strip above did not write), lane 63
//   writes the next strip's slot 127 below it in the same step: a slot is written only after its last read.
//   Traceback and ring are indexed by the STEP, not the column: ring slot (t - l) & 127, traceback dword (s * nst8 + t / 8) * 64 + l
//   with nst8 = ceil((min(C, W + 63) + 63) / 8), so the stores stay 256-byte rows whatever column a strip starts at; lane 0 walks
//   back through t = j - 1 - cs(strip of i) + l.
// ---------------------------------------------------------------------------------------------------------------
// a value every lane of the wavefront holds alike (a field of the pair's table row: the compiler cannot know), moved to scalar
// registers, so that what is derived from it (loop bounds, bases) stays there too
#if defined(__HIP_DEVICE_COMPILE__)
MPRG_DEV long long al_uniform(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
#else
MPRG_DEV long long al_uniform(long long v) { return v; }
#endif
// int32 words of workspace a banded pair needs, dlo and dhi already clamped to [-n, C]
MPRG_DEV long long al_band_ws_words(long long n, long long C, long long dlo, long long dhi) {
  const long long W = dhi - dlo + 1, nc = W + 63 < C ? W + 63 : C;
  return ((2 * W + 63) / 64) * 64 + ((n + 63) / 64) * ((nc + 63 + 7) / 8) * 64;
}

__global__ void __launch_bounds__(AL_THREADS) k_align_bounds(const int32_t *profile, const int64_t *leaves, int n_leaves, int64_t *bounds) {
  const int lane = wave_lane();
  const long long leaf = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (leaf >= n_leaves) return;
  const long long C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
  const int32_t *P = profile + leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
  long long sb = 0;
  int lmin = 2147483647;
  for (long long c = lane; c < C; c += 64) {
    const int dc = P[5 * C + c];
    int b = dc;
#pragma unroll
    for (int x = 0; x < 5; ++x) { const int v = P[x * C + c]; b = v > b ? v : b; }
    sb += b;
    lmin = b - dc < lmin ? b - dc : lmin;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sb += __shfl_xor(sb, d);
    const int y = __shfl_xor(lmin, d);
    lmin = y < lmin ? y : lmin;
  }
  if (lane == 0) { bounds[2 * leaf] = sb; bounds[2 * leaf + 1] = lmin; }
}

// k_align_bounds_endgap (star_align.py, "Free end pairs", band): k_align_bounds' wavefront per leaf for the counted bound of the
//   pairs with free ends: with B'_j = max(B_j, 0) and the threshold T = AL_BOUND_T, three int64 per leaf: SB' = sum_j B'_j, m' = the
//   smallest B'_j >= T (0 if there is none) and z = the number of columns with B'_j < T.
#define AL_BOUND_T 640
__global__ void __launch_bounds__(AL_THREADS) k_align_bounds_endgap(const int32_t *profile, const int64_t *leaves, int n_leaves, int64_t *bounds) {
  const int lane = wave_lane();
  const long long leaf = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (leaf >= n_leaves) return;
  const long long C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
  const int32_t *P = profile + leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
  long long sb = 0, z = 0;
  int mmin = 2147483647;
  for (long long c = lane; c < C; c += 64) {
    int b = P[5 * C + c];
#pragma unroll
    for (int x = 0; x < 5; ++x) { const int v = P[x * C + c]; b = v > b ? v : b; }
    b = b > 0 ? b : 0;
    sb += b;
    if (b < AL_BOUND_T) ++z;
    else mmin = b < mmin ? b : mmin;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sb += __shfl_xor(sb, d);
    z += __shfl_xor(z, d);
    const int y = __shfl_xor(mmin, d);
    mmin = y < mmin ? y : mmin;
  }
  if (lane == 0) { bounds[3 * leaf] = sb; bounds[3 * leaf + 1] = mmin == 2147483647 ? 0 : mmin; bounds[3 * leaf + 2] = z; }
}

// k_align_pairs_banded and k_align_pairs_endgap_banded: one text (al_pairs_band.inc)
#define AL_PAIRS_KERNEL k_align_pairs_banded
#define AL_ENDGAP 0
#include "al_pairs_band.inc"
#undef AL_PAIRS_KERNEL
#undef AL_ENDGAP
#define AL_PAIRS_KERNEL k_align_pairs_endgap_banded
#define AL_ENDGAP 1
#include "al_pairs_band.inc"
#undef AL_PAIRS_KERNEL
#undef AL_ENDGAP
