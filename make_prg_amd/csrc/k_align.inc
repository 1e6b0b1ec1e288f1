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

__global__ void __launch_bounds__(AL_THREADS) k_align_pairs(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                            const uint8_t *seqs, const int64_t *pairs, int n_pairs, int32_t *ws,
                                                            long long ws_words, uint8_t *ops, long long ops_bytes, int32_t *out) {
  SHARED(int32_t, ring_all, AL_WAVES * 6 * AL_RING);
  const int lane = wave_lane();
  const long long p = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (p >= n_pairs) return;                                   // (a whole wavefront: nothing below waits for the others)
  int32_t *ring = ring_all + wave_id() * 6 * AL_RING;
  const int64_t *PT = pairs + MPRG_AL_PAIR_FIELDS * p;
  const long long leaf = PT[0], soff = PT[1], n = PT[2], wsoff = PT[3], opoff = PT[4];
  int32_t *o = out + 3 * p;
  int status = MPRG_AL_OK;
  long long C = 0, poff = 0;
  if (leaf < 0 || leaf >= n_leaves) status = MPRG_AL_BAD_INPUT;
  else {
    C = leaves[MPRG_AL_LEAF_FIELDS * leaf + 2];
    poff = leaves[MPRG_AL_LEAF_FIELDS * leaf + 3];
    if (C < 1 || n < 0 || leaves[MPRG_AL_LEAF_FIELDS * leaf + 1] < 1) status = MPRG_AL_BAD_INPUT;
    else if (n + C >= AL_MAX_CELLS_SUM) status = MPRG_AL_TOO_LONG;
    else if (wsoff < 0 || (wsoff & 63) || wsoff + al_ws_words(n, C) > ws_words || opoff < 0 || opoff + n + C > ops_bytes)
      status = MPRG_AL_NO_SPACE;
  }
  if (status != MPRG_AL_OK) {
    if (lane == 0) { o[0] = status; o[1] = 0; o[2] = 0; }
    return;
  }
  const int32_t *P = profile + poff;
  const int Ci = (int)C, ni = (int)n;
  int32_t *row = ws + wsoff;                                 // row[2J] = H, row[2J + 1] = I of the row above the strip, column J
  uint32_t *tb = (uint32_t *)(ws + wsoff + ((2 * (C + 1) + 63) / 64) * 64);
  const long long nst8 = (C + 63 + 7) / 8;
  // row 0: H[0][J] = D[0][J] = open + the gap costs of columns < J
  int carry = 0;
  for (int c0 = 0; c0 < Ci; c0 += 64) {
    const int c = c0 + lane;
    const int incl = wave_scan_incl(c < Ci ? P[5LL * C + c] : 0) + carry;
    if (c < Ci) { row[2 * (c + 1)] = AL_OPEN + incl; row[2 * (c + 1) + 1] = AL_NEG; }
    carry = __shfl(incl, 63);
  }
  if (lane == 0) { row[0] = 0; row[1] = AL_NEG; }
  WAVE_SYNC_GLOBAL();
  int score = AL_NEG;
  const int n_strips = (ni + 63) / 64;
  for (int s = 0; s < n_strips; ++s) {
    const int i0 = s * 64, r = i0 + lane, rows = ni - i0 < 64 ? ni - i0 : 64;
    const bool valid = r < ni;
    const unsigned code = valid ? seqs[soff + r] : 0u;
    const int cls = code < 4 ? (int)code : 4;
    int h_left = al_hb(r + 1), d_left = AL_NEG;            // H, D of this lane's row, the column to the left
    int h_out = h_left, i_out = AL_NEG;                     // what the lane below reads next step (before the first column: H[i][0])
    int h_up_prev = al_hb(i0);                               // (lane 0) H of the row above, one column to the left: the diagonal
    uint32_t acc = 0;
    const int T = Ci + rows - 1;
    for (int t = 0; t < T; ++t) {
      if ((t & 63) == 0) {                                   // the ring takes columns [t, t + 64): the block of columns t - 128 is done with
        WAVE_SYNC();
#pragma unroll
        for (int k = 0; k < 6; ++k) ring[k * AL_RING + ((t + lane) & (AL_RING - 1))] = t + lane < Ci ? P[(long long)k * C + t + lane] : 0;
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
        const int dc = ring[5 * AL_RING + slot];
        const int diag = h_diag + ring[cls * AL_RING + slot];
        const int xcost = AL_INS;
#define AL_OPEN_D AL_OPEN + dc
#define AL_OPEN_I AL_OPEN + xcost
#include "al_cell.inc"
#undef AL_OPEN_D
#undef AL_OPEN_I
        if (lane == 63 && s + 1 < n_strips) { row[2 * (c + 1)] = h; row[2 * (c + 1) + 1] = ii; }
      }
      acc |= cell << (4 * (t & 7));
      if ((t & 7) == 7 || t == T - 1) { tb[((long long)s * nst8 + (t >> 3)) * 64 + lane] = acc; acc = 0; }
    }
    WAVE_SYNC_GLOBAL();                                      // the row buffer and the traceback, written by every lane, read by lane 0
  }
  score = ni > 0 ? __shfl(score, (ni - 1) & 63) : row[2 * C];
  constexpr bool kBand = false;                              // (the full matrix: every strip starts at column 0)
  constexpr int dlo = 0;
#include "al_walk.inc"
}

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

__global__ void __launch_bounds__(AL_THREADS) k_align_pairs_banded(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                                   const uint8_t *seqs, const int64_t *pairs, int n_pairs, int32_t *ws,
                                                                   long long ws_words, uint8_t *ops, long long ops_bytes, int32_t *out) {
  SHARED(int32_t, ring_all, AL_WAVES * 6 * AL_RING);
  const int lane = wave_lane();
  const long long p = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (p >= n_pairs) return;                                   // (a whole wavefront: nothing below waits for the others)
  int32_t *ring = ring_all + wave_id() * 6 * AL_RING;
  const int64_t *PT = pairs + MPRG_AL_BAND_PAIR_FIELDS * p;
  const long long leaf = PT[0], soff = PT[1], n = PT[2], wsoff = PT[3], opoff = PT[4];
  long long blo = PT[5], bhi = PT[6];
  int32_t *o = out + 3 * p;
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
      if (wsoff < 0 || (wsoff & 63) || wsoff + al_band_ws_words(n, C, blo, bhi) > ws_words || opoff < 0 || opoff + n + C > ops_bytes)
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
  const long long wsoff_u = al_uniform(wsoff), soff_u = al_uniform(soff);
  int32_t *row = ws + wsoff_u;                               // row[2k] = H, row[2k + 1] = I of the row above the strip (row i0), column i0 + dlo + k
  uint32_t *tb = (uint32_t *)(ws + wsoff_u + ((2 * (long long)W + 63) / 64) * 64);
  const long long nst8 = ((W + 63 < Ci ? W + 63 : Ci) + 63 + 7) / 8;
  // row 0, columns 0 .. dhi: H[0][J] = D[0][J] = open + the gap costs of columns < J
  int carry = 0;
  for (int c0 = 0; c0 < dhi; c0 += 64) {
    const int c = c0 + lane;
    const int incl = wave_scan_incl(c < dhi ? (P + 5LL * Ci)[(unsigned)c] : 0) + carry;
    if (c < dhi) { row[2 * (c + 1 - dlo)] = AL_OPEN + incl; row[2 * (c + 1 - dlo) + 1] = AL_NEG; }
    carry = __shfl(incl, 63);
  }
  if (lane == 0) { row[2 * (-dlo)] = 0; row[2 * (-dlo) + 1] = AL_NEG; }
  WAVE_SYNC_GLOBAL();
  int score = AL_NEG;
  const int n_strips = (ni + 63) / 64;
  for (int s = 0; s < n_strips; ++s) {
    const int i0 = s * 64, r = i0 + lane, rows = ni - i0 < 64 ? ni - i0 : 64;
    const bool valid = r < ni;
    const unsigned code = valid ? (seqs + soff_u)[(unsigned)r] : 0u;
    const int cls = code < 4 ? (int)code : 4;
    const int cs = i0 + dlo > 0 ? i0 + dlo : 0;             // the strip's first column, 0-based
    const int jtop = i0 + dhi < Ci ? i0 + dhi : Ci;         // the last column of row i0 inside the band
    const int jend = i0 + rows + dhi < Ci ? i0 + rows + dhi : Ci;   // the strip's last column, 1-based
    const int d0 = cs - r - dlo;                            // 0-based column c = cs + t - lane of this lane's row (r + 1) lies on diagonal c - r:
                                                            // inside the band where 0 <= d0 + t - lane <= dhi - dlo (and 0 <= c < C)
    const bool col0 = r + 1 + dlo <= 0;                     // column 0 of this lane's row lies inside the band
    int h_left = col0 ? al_hb(r + 1) : AL_NEG, d_left = AL_NEG;     // H, D of this lane's row, the column to the left of its first one
    int h_out = col0 && cs == lane ? al_hb(r + 1) : AL_NEG, i_out = AL_NEG;   // what the lane below reads next step: here of column cs - 1 - lane
    int h_up_prev = AL_NEG;                                  // H of the row above, one column to the left: the diagonal
    if (lane == 0) h_up_prev = cs == 0 ? al_hb(i0) : row[0];   // (cs > 0: column cs = i0 + dlo of row i0, its first inside the band)
    uint32_t acc = 0;
    uint32_t *tbs = tb + (long long)s * nst8 * 64;           // the strip's traceback: wave-uniform bases, 32-bit lane offsets
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
        const int dc = ring[5 * AL_RING + slot];
        const int diag = h_diag + ring[cls * AL_RING + slot];
        const int xcost = AL_INS;
#define AL_OPEN_D AL_OPEN + dc
#define AL_OPEN_I AL_OPEN + xcost
#include "al_cell.inc"
#undef AL_OPEN_D
#undef AL_OPEN_I
        if (lane == 63 && s + 1 < n_strips) { const int k = c + 1 - (i0 + 64 + dlo); row[(unsigned)(2 * k)] = h; row[(unsigned)(2 * k + 1)] = ii; }
      } else {
        h_out = c == -1 && r + 1 + dlo <= 0 ? al_hb(r + 1) : AL_NEG;   // outside the band: minus infinity, never a stale or an accumulated value
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
