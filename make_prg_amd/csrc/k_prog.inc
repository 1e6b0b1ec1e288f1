// ---------------------------------------------------------------------------------------------------------------
// K-P  progressive MSAs of `from_msa --unaligned --progressive` (make_prg_amd/from_msa/star_align.py holds the spec,
//      "Progressive"; DESIGN.md §3b): the guide tree's distances, the profile-profile DP of a merge, the children's rows written
//      through a merge's ops.  Integers only.  The tree itself is built on the host, or by k_prog_tree.inc.
//
// A node's text is its R x W matrix of CELL CODES (0..11, '-' = 4), row-major; a leaf's text is its sequence in the code buffer.
// Texts of different rounds live in different device buffers: the kernels that read texts take a table `bufs` of
// {address, bytes} and every text names its buffer by index, its range is checked against that buffer's size.
//
// k_prog_distances: one workgroup per (locus, sequence a).  c_a, the 4 096 6-mer counts of a, is built once in 16 KB of LDS and
//   then only read; for every b > a the workgroup builds c_b in a second 16 KB (zero, one LDS atomic per window), then every
//   thread takes 16 bins of sum_k min(c_a[k], c_b[k]); a wave reduction, four partial sums through LDS, thread 0 writes
//   s(a, b) at row a, column b of the locus's m x m table (only b > a is written).  nw_a comes out of the first pass.
// k_prog_columns: one workgroup per (item, 256-column tile), thread = column, the text's rows walked in order (k_align_profiles'
//   access pattern).  Kind 0 writes exactly k_align_profiles' 6 planes (Y's profile), kind 1 the 7 planes of an X side: the
//   counts of A C G T, of R Y K M S W N, of '-', and Ic.
// k_align_profile_pairs: k_align_pairs' structure with a profile on both sides, a kernel of its own but for the cell and the
//   walk back (al_cell.inc, al_walk.inc): one wavefront per merge, 64-column strips of X on the anti-diagonal, the row above
//   by shuffle, Y's six planes in the 128-column LDS ring, 4-bit traceback, lane 0 walking back.  A lane keeps its X column's six
//   counts and Ic in registers; a cell's score is six multiply-adds and the truncating division by R_X as a multiplication by a
//   per-merge constant and a shift (pg_div below).  H[i][0] = open + the Ic before row i: a wave scan per strip.  The row above a
//   strip is read 64 columns at a time with the ring's refill and handed to lane 0 by a shuffle, not loaded step by step.
// k_prog_rows: one wavefront per output row: a child's row through the merge's ops (stored reversed, read forward in 64-op
//   chunks; one wave scan gives each op the source cell it consumes), or a plain copy padded with '-' (op count < 0: the root's
//   rows into input order, empty records); cell codes, or ASCII for the final text.  Every output byte is written once.
// ---------------------------------------------------------------------------------------------------------------
#define PG_THREADS 256
#define PG_WAVES (PG_THREADS / 64)
#define PG_BINS ST_BINS                        // (a window is k_star.inc's: st_window.inc)
#define PG_K ST_K
#define PG_MAX_ROWS (1 << 20)                  // R_X up to here: pg_div stays exact and its operands stay in 32 bits

__global__ void __launch_bounds__(PG_THREADS) k_prog_distances(const uint8_t *codes, long long codes_bytes, const int64_t *seqs,
                                                               long long n_seqs, const int64_t *loci, int n_loci, const int32_t *work,
                                                               uint32_t *shared, long long shared_words, int64_t *nw, int32_t *status) {
  SHARED(uint32_t, ha, PG_BINS);
  SHARED(uint32_t, hb, PG_BINS);
  SHARED(long long, red, PG_WAVES);
  SHARED(int, bad, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long l = wk[0], a = wk[1];
  long long first = 0, m = 0, toff = 0;
  bool ok = l >= 0 && l < n_loci;
  if (ok) {
    const int64_t *L = loci + MPRG_ST_LOCUS_FIELDS * l;
    first = L[0]; m = L[1]; toff = L[3];
    ok = first >= 0 && m >= 1 && m <= 0x7fffffffLL && first <= n_seqs - m && a >= 0 && a < m && toff >= 0 && toff <= shared_words &&
         m <= (shared_words - toff) / m;
  }
#include "st_seqs_par.inc"
  ONE_THREAD status[BLOCK_ID] = bad[0] ? MPRG_PG_BAD_ITEM : MPRG_PG_OK;
  if (bad[0]) return;                                        // (the whole workgroup)
  PAR_FOR(k, PG_BINS) ha[k] = 0;
  BARRIER();
  {
    const long long off = seqs[2 * (first + a)], n = seqs[2 * (first + a) + 1];
    long long part = 0;
    PAR_FOR(w, n - (PG_K - 1)) {
#include "st_window.inc"
      if (valid) { ATOMIC_ADD(&ha[k], 1u); ++part; }
    }
#include "wg_sum.inc"                                        // (behind its barrier ha is read-only)
    ONE_THREAD {
      WG_TOTAL(s, PG_WAVES);
      nw[first + a] = s;
    }
  }
  for (long long b = a + 1; b < m; ++b) {
    const long long off = seqs[2 * (first + b)], n = seqs[2 * (first + b) + 1];
    if (n < PG_K) {                                          // (workgroup-uniform) no window: nothing shared
      ONE_THREAD shared[toff + a * m + b] = 0u;
      continue;
    }
    PAR_FOR(k, PG_BINS) hb[k] = 0;
    BARRIER();
    PAR_FOR(w, n - (PG_K - 1)) {
#include "st_window.inc"
      if (valid) ATOMIC_ADD(&hb[k], 1u);
    }
    BARRIER();
    long long part = 0;
    PAR_FOR(k, PG_BINS) part += ha[k] < hb[k] ? ha[k] : hb[k];
#include "wg_sum.inc"
    ONE_THREAD {
      WG_TOTAL(s, PG_WAVES);
      shared[toff + a * m + b] = (uint32_t)s;
    }                                                        // (red is written again only after the next two barriers)
  }
}

// a text's fields against the buffer table: the buffer exists and holds R x W cells at `off`
MPRG_DEV bool pg_text_ok(const int64_t *bufs, int n_bufs, long long buf, long long off, long long R, long long W) {
  if (buf < 0 || buf >= n_bufs || R < 1 || W < 1 || R > 0x7fffffffLL || W > 0x7fffffffLL) return false;
  const long long bytes = bufs[2 * buf + 1];
  return off >= 0 && off <= bytes && R <= (bytes - off) / W;
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_columns(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items,
                                                             const int32_t *work, int32_t *cols, long long cols_words, int32_t *status) {
  long long buf = 0, off = 0, R = 0, W = 0, kind = 0, coff = 0;
#define PG_ITEM_STRIDE MPRG_PG_ITEM_FIELDS
#define PG_ITEM_READ_MORE
#define PG_ITEM_ALSO_BAD false
#include "pg_item.inc"
#undef PG_ITEM_STRIDE
#undef PG_ITEM_READ_MORE
#undef PG_ITEM_ALSO_BAD
  if (threadIdx.x == 0) status[BLOCK_ID] = st;
  if (st != MPRG_PG_OK) return;                              // (the whole workgroup)
  const long long c = tile * 256 + (long long)threadIdx.x;
  if (c >= W) return;
  const uint8_t *text = (const uint8_t *)(uintptr_t)bufs[2 * buf] + off;
#define AL_CELL(r) text[(r) * W + c]
#define AL_WEIGHT(r) 1
#include "al_counts.inc"
#undef AL_CELL
#undef AL_WEIGHT
  const long long pl_rows = R, pl_stride = W;
  int32_t *o = cols + coff + c;
#include "al_planes.inc"
}

// C's truncating v / R for |v| <= 1 280 R, R <= PG_MAX_ROWS, as a multiplication and a shift: with s = ceil(log2 R) and
// M = floor(2^(31 + s) / R) + 1 (< 2^32), floor(|v| / R) = (2 |v| M) >> (32 + s): M R - 2^(31 + s) = e with 0 < e <= R, so
// |v| M / 2^(31 + s) = |v| / R + |v| e / (R 2^(31 + s)), and the excess is below 1 / R because |v| e <= 1 280 R^2 < 2^(31 + s).
struct PgDiv { unsigned mul; int shift; };
MPRG_DEV PgDiv pg_div_make(long long R) {
  PgDiv d;
  d.shift = R <= 1 ? 0 : 32 - __builtin_clz((unsigned)(R - 1));
  d.mul = (unsigned)((1ull << (31 + d.shift)) / (unsigned long long)R + 1ull);
  return d;
}
MPRG_DEV int pg_div(int v, const PgDiv d) {
  const unsigned av = (unsigned)(v < 0 ? -v : v);
  const int q = (int)((unsigned)(((unsigned long long)(av << 1) * d.mul) >> 32) >> d.shift);
  return v < 0 ? -q : q;
}

__global__ void __launch_bounds__(AL_THREADS) k_align_profile_pairs(const int32_t *profile, const int64_t *leaves, int n_leaves,
                                                                    const int32_t *xcols, long long xcols_words, const int64_t *pairs,
                                                                    int n_pairs, int32_t *ws, long long ws_words, uint8_t *ops,
                                                                    long long ops_bytes, int32_t *out) {
  SHARED(int32_t, ring_all, AL_WAVES * 6 * AL_RING);
  const int lane = wave_lane();
  const long long p = (long long)BLOCK_ID * AL_WAVES + wave_id();
  if (p >= n_pairs) return;                                   // (a whole wavefront: nothing below waits for the others)
  int32_t *ring = ring_all + wave_id() * 6 * AL_RING;
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
  // row 0: H[0][J] = D[0][J] = open + the gap costs of columns < J
  int carry = 0;
  for (int c0 = 0; c0 < Ci; c0 += 64) {
    const int c = c0 + lane;
    const int incl = wave_scan_incl(c < Ci ? (P + 5LL * Ci)[(unsigned)c] : 0) + carry;
    if (c < Ci) { row[2 * (c + 1)] = AL_OPEN + incl; row[2 * (c + 1) + 1] = AL_NEG; }
    carry = __shfl(incl, 63);
  }
  if (lane == 0) { row[0] = 0; row[1] = AL_NEG; }
  WAVE_SYNC_GLOBAL();
  int score = AL_NEG;
  int ic_before = 0;                                         // the Ic of all rows above the strip
  const int n_strips = (ni + 63) / 64;
  for (int s = 0; s < n_strips; ++s) {
    const int i0 = s * 64, r = i0 + lane, rows = ni - i0 < 64 ? ni - i0 : 64;
    const bool valid = r < ni;
    // this lane's X column: the counts of A C G T, of the ambiguity codes, of '-', and what the column alone costs
    const int x0 = valid ? X[(unsigned)r] : 0, x1 = valid ? (X + (long long)ni)[(unsigned)r] : 0;
    const int x2 = valid ? (X + 2LL * ni)[(unsigned)r] : 0, x3 = valid ? (X + 3LL * ni)[(unsigned)r] : 0;
    const int xa = valid ? (X + 4LL * ni)[(unsigned)r] : 0, xg = valid ? (X + 5LL * ni)[(unsigned)r] : 0;
    const int ic = valid ? (X + 6LL * ni)[(unsigned)r] : 0;
    const int ic_incl = wave_scan_incl(ic) + ic_before;     // the Ic of rows 1 .. r + 1
    int h_left = AL_OPEN + ic_incl, d_left = AL_NEG;       // H, D of this lane's row, the column to the left: H[r + 1][0]
    int h_out = h_left, i_out = AL_NEG;                     // what the lane below reads next step (before the first column: H[i][0])
    int h_up_prev = i0 == 0 ? 0 : AL_OPEN + ic_before;      // (lane 0) H of the row above, one column to the left: the diagonal
    ic_before = __shfl(ic_incl, 63);
    uint32_t acc = 0;
    uint32_t *tbs = tb + (long long)s * nst8 * 64;
    int h_row = AL_NEG, i_row = AL_NEG;                      // H, I of the row above the strip, column t0 + 1 + lane of the 64-step block
    const int T = Ci + rows - 1;
    for (int t = 0; t < T; ++t) {
      if ((t & 63) == 0) {                                   // the ring takes columns [t, t + 64): the block of columns t - 128 is done with
        WAVE_SYNC();
#pragma unroll
        for (int k = 0; k < 6; ++k) ring[k * AL_RING + ((t + lane) & (AL_RING - 1))] = t + lane < Ci ? (P + (long long)k * Ci)[(unsigned)(t + lane)] : 0;
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
        const int dc = ring[5 * AL_RING + slot];
        const int num = x0 * ring[slot] + x1 * ring[AL_RING + slot] + x2 * ring[2 * AL_RING + slot] + x3 * ring[3 * AL_RING + slot] +
                        xa * ring[4 * AL_RING + slot] + xg * dc;
        const int diag = h_diag + pg_div(num, dv);
        const int xcost = ic;
#include "al_cell.inc"
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

__global__ void __launch_bounds__(PG_THREADS) k_prog_rows(const int64_t *bufs, int n_bufs, const uint8_t *ops, long long ops_bytes,
                                                          const int64_t *rows, int n_rows, uint8_t *out, long long out_bytes, int ascii,
                                                          int32_t *status) {
  const long long q = (long long)BLOCK_ID * PG_WAVES + wave_id();
  if (q >= n_rows) return;                                   // (a whole wavefront)
  const int lane = wave_lane();
  const int64_t *Q = rows + MPRG_PG_ROW_FIELDS * q;
  const long long buf = Q[0], soff = Q[1], n = Q[2], ops_off = Q[3], k = Q[4], side = Q[5], ooff = Q[6], W = Q[7];
  int st = MPRG_PG_OK;
  if (buf < 0 || buf >= n_bufs || n < 0 || soff < 0 || soff > bufs[2 * buf + 1] || n > bufs[2 * buf + 1] - soff || (side != 0 && side != 1))
    st = MPRG_PG_BAD_ITEM;
  else if (W < 0 || ooff < 0 || ooff > out_bytes || W > out_bytes - ooff) st = MPRG_PG_NO_SPACE;
  else if (k < 0 ? n > W : (k != W || ops_off < 0 || ops_off > ops_bytes || k > ops_bytes - ops_off)) st = MPRG_PG_BAD_OPS;
  if (st != MPRG_PG_OK) { if (lane == 0) status[q] = st; return; }
  const char *abc = "ACGT-RYKMSWN";
  const uint8_t *src = (const uint8_t *)(uintptr_t)bufs[2 * buf] + soff;
  uint8_t *o = out + ooff;
  bool bad = false;
  if (k < 0) {
    for (long long c = lane; c < W; c += WAVE) {
      const unsigned ch = c < n ? (unsigned)src[c] : (unsigned)C_GAP;
      o[c] = ascii ? (uint8_t)abc[ch < 12u ? ch : (unsigned)C_GAP] : (uint8_t)ch;
    }
  } else {
    long long used = 0;                                      // source cells consumed by the ops before the chunk
    for (long long q0 = 0; q0 < k; q0 += WAVE) {
      const long long x = q0 + lane;
      const bool valid = x < k;
      const unsigned op = valid ? (unsigned)ops[ops_off + k - 1 - x] : (unsigned)'M';
      if (op != 'M' && op != 'I' && op != 'D') bad = true;
      const int take = valid && (side == 0 ? op != 'I' : op != 'D');
      const int incl = wave_scan_incl(take);
      const long long idx = used + incl - take;
      used += __shfl(incl, 63);
      if (!valid) continue;
      unsigned ch = C_GAP;
      if (take) { if (idx < n) ch = src[idx]; else bad = true; }
      o[x] = ascii ? (uint8_t)abc[ch < 12u ? ch : (unsigned)C_GAP] : (uint8_t)ch;
    }
    if (used != n) bad = true;
  }
  bad = __ballot(bad) != 0ull;
  if (lane == 0) status[q] = bad ? MPRG_PG_BAD_OPS : MPRG_PG_OK;
}
