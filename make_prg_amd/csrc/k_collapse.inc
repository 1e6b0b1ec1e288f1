// ---------------------------------------------------------------------------------------------------------------
// K-C  `from_msa --unaligned --collapse-identical` (make_prg_amd/from_msa/star_align.py holds the spec, "Collapse"; DESIGN.md
//      §3b): the classes of identical sequences of a locus, and the column tables of a text whose rows count w times.
//      Integers only.  Kernels of their own, so that every kernel of k_star.inc and k_prog.inc stays what it was; what they have in
//      common with those is one text, included in both (st_seqs_par.inc, pg_item.inc, al_counts.inc, al_planes.inc; DESIGN.md §3a).
//
// k_star_identical: one workgroup per locus, a wavefront per sequence (the wavefronts take the sequences round-robin), lanes on
//   consecutive bytes.  A sequence's hash is the SUM over its positions of a mix of (position, code): a sum does not depend on
//   which lane took which position, so the wave reduction may add the lanes' parts in any order.  The sequences are taken in
//   tiles of ID_TILE: the tile's hashes and lengths go to LDS (8 KB), then every sequence a at or behind the tile's start is
//   scanned against the tile's b < a, 64 candidates per step, one ballot; the candidates of equal (hash bits, length) are
//   compared byte by byte in ascending order and the first equal one is rep[a].  A later tile is only scanned for a sequence no
//   earlier tile settled (rep[a] == a still), so rep[a] is the smallest equal b.  A locus of more than ID_TILE sequences costs
//   one hash of a per earlier tile more; nothing is kept per sequence but rep itself: no scratch, any record count.
//   The hash only filters: filter_bits of it are compared (0: every pair of equal length goes to the byte comparison).
// k_prog_columns_weighted: k_prog_columns' texts (item fields, counts, planes) with row r counted weights[r] times and the divisor
//   the weight sum: the planes of the text with every row written w_r times.  The workgroup first adds up the weights (every
//   thread a stride of rows, wg_sum.inc) and refuses the item when one is below 1 or the sum is not the stated one.
// ---------------------------------------------------------------------------------------------------------------
#define ID_THREADS 256
#define ID_WAVES (ID_THREADS / 64)
#define ID_TILE 512                            // sequences whose hashes and lengths are in LDS at once (a multiple of ID_WAVES)

// what position i holding code c adds to a sequence's hash
MPRG_DEV unsigned long long id_mix(long long i, unsigned c) {
  unsigned long long x = ((unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull ^ ((unsigned long long)c + 1ull) * 0xC2B2AE3D27D4EB4Full;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  return x;
}

// the hash of codes[off .. off + n), by one wavefront: the same value in every lane
MPRG_DEV unsigned long long id_hash(const uint8_t *codes, long long off, long long n) {
  unsigned long long h = 0;
  for (long long i = wave_lane(); i < n; i += WAVE) h += id_mix(i, codes[off + i]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) h += __shfl_xor(h, d);
  return h;
}

__global__ void __launch_bounds__(ID_THREADS) k_star_identical(const uint8_t *codes, long long codes_bytes, const int64_t *seqs,
                                                               long long n_seqs, const int64_t *loci, int filter_bits, int32_t *rep,
                                                               int32_t *status) {
  SHARED(unsigned long long, hash, ID_TILE);
  SHARED(long long, len, ID_TILE);
  SHARED(int, bad, 1);
  const int64_t *L = loci + MPRG_ST_LOCUS_FIELDS * (long long)BLOCK_ID;
  const long long first = L[0], m = L[1];
  const bool ok = first >= 0 && m >= 0 && m <= 0x7fffffffLL && first <= n_seqs - m;
#include "st_seqs_par.inc"
  ONE_THREAD status[BLOCK_ID] = bad[0] ? MPRG_ST_CENTRE_BAD : MPRG_ST_OK;
  if (bad[0]) return;                                        // (the whole workgroup; no rep written)
  PAR_FOR(x, m) rep[first + x] = (int32_t)x;
  const unsigned long long mask = filter_bits <= 0 ? 0ull : filter_bits >= 64 ? ~0ull : (1ull << filter_bits) - 1ull;
  const int lane = wave_lane();
  for (long long s0 = 0; s0 < m; s0 += ID_TILE) {
    const long long s1 = s0 + ID_TILE < m ? s0 + ID_TILE : m;
    BARRIER();                                               // the tile before is done with; rep as written so far is visible
    for (long long b = s0 + wave_id(); b < s1; b += ID_WAVES) {
      const long long off = seqs[2 * (first + b)], n = seqs[2 * (first + b) + 1];
      const unsigned long long h = id_hash(codes, off, n);
      if (lane == 0) { hash[b - s0] = h; len[b - s0] = n; }
    }
    BARRIER();                                               // hash and len are read-only until the next tile
    // (s0 is a multiple of ID_WAVES: sequence a belongs to the same wavefront in every tile)
    for (long long a = s0 + wave_id(); a < m; a += ID_WAVES) {
      const long long off = seqs[2 * (first + a)], n = seqs[2 * (first + a) + 1];
      if (n == 0 || a == s0 || rep[first + a] != (int32_t)a) continue;       // (wave-uniform) empty, nothing before it, or settled
      const unsigned long long h = a < s1 ? hash[a - s0] : id_hash(codes, off, n);
      const long long bmax = a < s1 ? a : s1;
      long long found = -1;
      for (long long b0 = s0; b0 < bmax && found < 0; b0 += WAVE) {
        const long long b = b0 + lane;
        unsigned long long cand = __ballot(b < bmax && len[b - s0] == n && ((hash[b - s0] ^ h) & mask) == 0ull);
        while (cand && found < 0) {
          const int j = __builtin_ctzll(cand);
          cand &= cand - 1ull;
          const long long boff = seqs[2 * (first + b0 + j)];
          bool differs = false;
          for (long long i0 = 0; i0 < n && !differs; i0 += WAVE) {
            const long long i = i0 + lane;
            differs = __ballot(i < n && codes[off + i] != codes[boff + i]) != 0ull;
          }
          if (!differs) found = b0 + j;
        }
      }
      if (found >= 0 && lane == 0) rep[first + a] = (int32_t)found;
    }
  }
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_columns_weighted(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items,
                                                                      const int32_t *work, int max_kind, const int32_t *weights, long long weights_words,
                                                                      int32_t *cols, long long cols_words, int32_t *status) {
  SHARED(long long, red, PG_WAVES);
  SHARED(int, low, 1);
  long long buf = 0, off = 0, R = 0, W = 0, kind = 0, coff = 0, woff = 0, S = 0;
#define PG_ITEM_STRIDE MPRG_PG_WITEM_FIELDS
#define PG_ITEM_READ_MORE woff = I[6]; S = I[7];
#define PG_ITEM_ALSO_BAD woff < 0 || woff > weights_words || R > weights_words - woff || S < R || S > PG_MAX_ROWS
#include "pg_item.inc"
#undef PG_ITEM_STRIDE
#undef PG_ITEM_READ_MORE
#undef PG_ITEM_ALSO_BAD
  if (st != MPRG_PG_OK) {                                    // (the whole workgroup)
    if (threadIdx.x == 0) status[BLOCK_ID] = st;
    return;
  }
  const int32_t *wt = weights + woff;
  ONE_THREAD low[0] = 0;
  BARRIER();
  long long part = 0;
  int below = 0;
  PAR_FOR(r, R) { const long long w = wt[r]; below |= w < 1; part += w; }
  if (below) ATOMIC_OR(&low[0], 1);
#include "wg_sum.inc"
  WG_TOTAL(sum, PG_WAVES);                                   // (every thread: st stays workgroup-uniform)
  if (low[0] || sum != S) st = MPRG_PG_BAD_ITEM;
  if (threadIdx.x == 0) status[BLOCK_ID] = st;
  if (st != MPRG_PG_OK) return;                              // (the whole workgroup)
  const long long c = tile * 256 + (long long)threadIdx.x;
  if (c >= W) return;
  const uint8_t *text = (const uint8_t *)(uintptr_t)bufs[2 * buf] + off;
#define AL_CELL(r) text[(r) * W + c]
#define AL_WEIGHT(r) wt[r]
#include "al_counts.inc"
#undef AL_CELL
#undef AL_WEIGHT
  const long long pl_rows = S, pl_stride = W;                    // (the rows of the text with row r written w_r times)
  int32_t *o = cols + coff + c;
#include "al_planes.inc"
}
