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
//   counts of A C G T, of R Y K M S W N, of '-', and Ic.  Kind 2 (only where max_kind = 2: mprg_prog_columns_posgap) writes kind 0's
//   six planes and Oc, the open of a run that starts at the column.
// k_align_profile_pairs (its text: pg_pairs.inc, included four times: as k_align_profile_pairs_posgap, the merge with
//   position-specific opens, and as the _endgap forms of both, the merges with free end gaps): k_align_pairs' structure with a profile on both sides, a kernel of its own but for the cell and the
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
                                                             const int32_t *work, int max_kind, int32_t *cols, long long cols_words, int32_t *status) {
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

#define PG_ENDGAP 0
#define PG_PAIRS_KERNEL k_align_profile_pairs
#define PG_POSGAP 0
#include "pg_pairs.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#define PG_PAIRS_KERNEL k_align_profile_pairs_posgap
#define PG_POSGAP 1
#include "pg_pairs.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#undef PG_ENDGAP
// ... and with free end gaps (star_align.py, "Free end gaps"), for both forms of the open
#define PG_ENDGAP 1
#define PG_PAIRS_KERNEL k_align_profile_pairs_endgap
#define PG_POSGAP 0
#include "pg_pairs.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#define PG_PAIRS_KERNEL k_align_profile_pairs_posgap_endgap
#define PG_POSGAP 1
#include "pg_pairs.inc"
#undef PG_PAIRS_KERNEL
#undef PG_POSGAP
#undef PG_ENDGAP

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
