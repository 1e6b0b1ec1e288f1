// ---------------------------------------------------------------------------------------------------------------
// K-C  `compare_msa`: a test MSA scored against a reference MSA of the same records (make_prg_amd/from_msa/msa_compare.py holds
//      the spec; DESIGN.md §3b, "Truth recovery").  Integers only.
//
// Texts are K-P's: R x W CELL CODES (0..11, '-' = 4), row-major, named by {buffer, offset} against the table `bufs`.  A locus is
// a test text (R x W_T) and a reference text (R x W_R); the host has matched the rows.
//
// k_msa_compare_map: a wavefront per row {locus, reference row, test row, reversed, tpos offset, tpos capacity}.  Three walks in
//   chunks of 64 columns, a ballot and a popcount giving a residue's index in its row: (1) both rows are counted, and a row whose
//   two residue counts differ, or exceed its tpos capacity, is refused with nothing written; (2) the test row: residue p's column
//   goes to tpos[p], and m[column] takes an integer atomic add; (3) the reference row: residue p reads its test column
//   tc = tpos[p] (tpos[n - 1 - p] for a reversed row), compares its code with the test cell's (complemented for a reversed row)
//   and writes tmap(row, c) = tc; a gap writes INT32_MAX.  Between (2) and (3) the wavefront waits for its own stores.
//   tmap is row-major (layout 0: tmap[row W_R + c]) or column-major (layout 1: tmap[c R + row]).
// k_msa_compare_columns: a workgroup per {locus, column block q}.  P the next power of two >= R, G = 8 192 / P: the block's G
//   reference columns go into an LDS tile of 8 192 int32 (32 KB), a segment of P words per column, filled up with INT32_MAX (as
//   is every value outside [0, W_T): what a refused row left unwritten cannot index anything).  One bitonic sort over the tile
//   whose partners i ^ j stay inside a segment (j < P) and whose last merge is ascending in every segment; then every element's
//   lower bound in its segment by bisection: i - lower bound values equal to it stand before it, and these ranks add up to the
//   column's sum over t of C(n_{c,t}, 2).  The segment's first word does the column: n_c is the sentinel's lower bound, kept is
//   first == last valid value, identical is kept and m[value] == n_c.  The block also takes its share of the locus's m table for
//   test_pairs.  Three workgroup sums (wg_sum.inc), then at most six 64-bit integer atomic adds per workgroup.  Barriers only: no
//   loop here waits for another thread's store.
// ---------------------------------------------------------------------------------------------------------------
#define CM_THREADS 256
#define CM_WAVES (CM_THREADS / 64)
#define CC_THREADS 256
#define CC_WAVES (CC_THREADS / 64)
#define CC_TILE 8192
#define CMP_GAP_V 0x7fffffff

// star_align.revcomp's table: A<->T, C<->G, R<->Y, K<->M; '-', S, W, N (and anything above) unchanged
MPRG_DEV int cmp_complement(int c) { return c < 4 ? 3 - c : c == 5 ? 6 : c == 6 ? 5 : c == 7 ? 8 : c == 8 ? 7 : c; }

struct CmpLocus { long long tbuf, toff, WT, rbuf, roff, WR, R, moff_map, layout, moff; };

// the locus's fields against the tables both kernels see: the widths, the row count, tmap and m inside their buffers
MPRG_DEV bool cmp_locus_ok(const int64_t *loci, int n_loci, long long l, long long tmap_words, long long m_words, CmpLocus *L) {
  if (l < 0 || l >= n_loci) return false;
  const int64_t *I = loci + MPRG_CMP_LOCUS_FIELDS * l;
  L->tbuf = I[0]; L->toff = I[1]; L->WT = I[2]; L->rbuf = I[3]; L->roff = I[4]; L->WR = I[5]; L->R = I[6]; L->moff_map = I[7];
  L->layout = I[8]; L->moff = I[9];
  if (L->R < 1 || L->R > 0x7fffffffLL || L->WT < 1 || L->WT > 0x7ffffffeLL || L->WR < 1 || L->WR > 0x7ffffffeLL) return false;
  if (L->layout != 0 && L->layout != 1) return false;
  if (L->moff_map < 0 || L->moff_map > tmap_words || L->R > (tmap_words - L->moff_map) / L->WR) return false;
  return L->moff >= 0 && L->moff <= m_words && L->WT <= m_words - L->moff;
}

MPRG_DEV long long cmp_map_index(const CmpLocus &L, long long row, long long c) {
  return L.moff_map + (L.layout ? c * L.R + row : row * L.WR + c);
}

__global__ void __launch_bounds__(CM_THREADS) k_msa_compare_map(const int64_t *bufs, int n_bufs, const int64_t *loci, int n_loci,
                                                                const int64_t *rows, long long n_rows, int32_t *tpos,
                                                                long long tpos_words, int32_t *tmap, long long tmap_words, int32_t *m,
                                                                long long m_words, int32_t *status) {
  const long long q = (long long)BLOCK_ID * CM_WAVES + wave_id();
  if (q >= n_rows) return;                                   // (a whole wavefront)
  const int lane = wave_lane();
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t *Q = rows + MPRG_CMP_ROW_FIELDS * q;
  const long long l = Q[0], kr = Q[1], kt = Q[2], rev = Q[3], poff = Q[4], cap = Q[5];
  CmpLocus L;
  int st = MPRG_CMP_OK;
  if (!cmp_locus_ok(loci, n_loci, l, tmap_words, m_words, &L) || !pg_text_ok(bufs, n_bufs, L.tbuf, L.toff, L.R, L.WT) ||
      !pg_text_ok(bufs, n_bufs, L.rbuf, L.roff, L.R, L.WR) || kr < 0 || kr >= L.R || kt < 0 || kt >= L.R || (rev != 0 && rev != 1) ||
      cap < 0 || poff < 0 || poff > tpos_words || cap > tpos_words - poff)
    st = MPRG_CMP_BAD_ITEM;
  if (st != MPRG_CMP_OK) {                                   // (the whole wavefront)
    if (lane == 0) status[q] = st;
    return;
  }
  const uint8_t *trow = (const uint8_t *)(uintptr_t)bufs[2 * L.tbuf] + L.toff + kt * L.WT;
  const uint8_t *rrow = (const uint8_t *)(uintptr_t)bufs[2 * L.rbuf] + L.roff + kr * L.WR;
  // (1) the two residue counts; nothing is written before they agree
  long long nt = 0, nr = 0;
  for (long long c0 = 0; c0 < L.WT; c0 += 64) {
    const long long c = c0 + lane;
    nt += __popcll(__ballot(c < L.WT && trow[c] != C_GAP));
  }
  for (long long c0 = 0; c0 < L.WR; c0 += 64) {
    const long long c = c0 + lane;
    nr += __popcll(__ballot(c < L.WR && rrow[c] != C_GAP));
  }
  if (nt != nr || nt > cap) {                                // (the whole wavefront)
    if (lane == 0) status[q] = MPRG_CMP_COUNT;
    return;
  }
  // (2) the test row: residue p's column, and the column's residue count
  int32_t *tp = tpos + poff;
  int32_t *mt = m + L.moff;
  long long base = 0;
  for (long long c0 = 0; c0 < L.WT; c0 += 64) {
    const long long c = c0 + lane;
    const bool res = c < L.WT && trow[c] != C_GAP;
    const unsigned long long b = __ballot(res);
    if (res) {
      tp[base + __popcll(b & below)] = (int32_t)c;
      ATOMIC_ADD(&mt[c], 1);
    }
    base += __popcll(b);
  }
  WAVE_SYNC_GLOBAL();                                        // the wavefront's tpos stores before its other lanes read them
  // (3) the reference row: every cell's v, and the codes
  int differ = 0;
  base = 0;
  for (long long c0 = 0; c0 < L.WR; c0 += 64) {
    const long long c = c0 + lane;
    const int cell = c < L.WR ? rrow[c] : C_GAP;
    const bool res = cell != C_GAP;
    const unsigned long long b = __ballot(res);
    if (c < L.WR) {
      int32_t v = CMP_GAP_V;
      if (res) {
        const long long p = base + __popcll(b & below);
        v = tp[rev ? nt - 1 - p : p];
        const int tc = trow[v];
        differ |= cell != (rev ? cmp_complement(tc) : tc);
      }
      tmap[cmp_map_index(L, kr, c)] = v;
    }
    base += __popcll(b);
  }
  const unsigned long long differing = __ballot(differ);
  if (lane == 0) status[q] = differing ? MPRG_CMP_CODE : MPRG_CMP_OK;
}

__global__ void __launch_bounds__(CC_THREADS) k_msa_compare_columns(const int64_t *loci, int n_loci, const int32_t *work,
                                                                    const int32_t *tmap, long long tmap_words, const int32_t *m,
                                                                    long long m_words, int64_t *counts, int32_t *status) {
  SHARED(int32_t, tile, CC_TILE);
  SHARED(long long, red, CC_WAVES);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long l = wk[0], q = wk[1];
  CmpLocus L;
  int st = MPRG_CMP_OK;
  long long P = 1;
  if (!cmp_locus_ok(loci, n_loci, l, tmap_words, m_words, &L) || L.R > MPRG_CMP_MAX_ROWS) st = MPRG_CMP_BAD_ITEM;
  else {
    while (P < L.R) P <<= 1;
    if (q < 0 || q * (CC_TILE / P) >= L.WR) st = MPRG_CMP_BAD_ITEM;
  }
  if (threadIdx.x == 0) status[BLOCK_ID] = st;
  if (st != MPRG_CMP_OK) return;                             // (the whole workgroup)
  const long long G = CC_TILE / P, c_lo = q * G;
  const long long cols = L.WR - c_lo < G ? L.WR - c_lo : G;  // the block's columns inside the text
  const long long R = L.R;
  int lg = 0;                                                // P = 1 << lg
  while ((1ll << lg) < P) ++lg;
  // the tile: column g's R values in tile[g P ..], every other word the sentinel
  if (L.layout) {
    PAR_FOR(i, CC_TILE) {                                    // (consecutive threads: consecutive rows of a column, contiguous in tmap)
      const long long g = i >> lg, r = i & (P - 1);
      int32_t v = CMP_GAP_V;
      if (g < cols && r < R) v = tmap[L.moff_map + (c_lo + g) * R + r];
      tile[i] = v < 0 || v >= L.WT ? CMP_GAP_V : v;
    }
  } else {
    PAR_FOR(i, CC_TILE) tile[i] = CMP_GAP_V;
    BARRIER();
    PAR_FOR(i, R * cols) {                                   // (consecutive threads: consecutive columns of a row)
      const long long r = i / cols, g = i - r * cols;
      const int32_t v = tmap[L.moff_map + r * L.WR + c_lo + g];
      if (v >= 0 && v < L.WT) tile[g * P + r] = v;
    }
  }
  BARRIER();
  // the segmented bitonic sort: the partner i ^ j differs below bit lg, the direction comes from the index inside the segment
  for (long long k = 2; k <= P; k <<= 1) {
    for (long long j = k >> 1; j > 0; j >>= 1) {
      PAR_FOR(t, CC_TILE / 2) {
        const long long i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), h = i | j;
        const bool up = ((i & (P - 1)) & k) == 0;
        const int32_t a = tile[i], b = tile[h];
        if ((a > b) == up) { tile[i] = b; tile[h] = a; }
      }
      BARRIER();
    }
  }
  // the ranks, and per segment the column
  long long part = 0, cols_part = 0;
  PAR_FOR(i, CC_TILE) {
    const long long s = i & ~(P - 1);
    const int32_t v = tile[i];
    if (v != CMP_GAP_V) {
      long long lo = s, hi = i;                              // the first word of [s, i] that is not below v
      while (lo < hi) { const long long mid = (lo + hi) >> 1; if (tile[mid] < v) lo = mid + 1; else hi = mid; }
      part += i - lo;
    }
    if (i == s && (i >> lg) < cols) {
      long long lo = s, hi = s + P;                          // the first sentinel of the segment, or its end
      while (lo < hi) { const long long mid = (lo + hi) >> 1; if (tile[mid] != CMP_GAP_V) lo = mid + 1; else hi = mid; }
      const long long n = lo - s;
      part += (n * (n - 1) / 2) << 32;
      if (n >= 2) {
        cols_part += 1;
        if (tile[s] == tile[s + n - 1]) cols_part += (1ll << 16) + (m[L.moff + tile[s]] == n ? 1ll << 32 : 0);
      }
    }
  }
#include "wg_sum.inc"
  WG_TOTAL(pairs, CC_WAVES);                                 // shared | ref_pairs << 32: each below 2^26 per tile
  BARRIER();
  part = cols_part;
#include "wg_sum.inc"
  WG_TOTAL(columns, CC_WAVES);                               // ref_columns | kept << 16 | identical << 32: each at most 4 096 per tile
  BARRIER();
  // this block's share of the m table
  const long long n_blocks = (L.WR + G - 1) / G, share = (L.WT + n_blocks - 1) / n_blocks;
  const long long t_lo = q * share < L.WT ? q * share : L.WT, t_hi = t_lo + share < L.WT ? t_lo + share : L.WT;
  part = 0;
  PAR_FOR(t, t_hi - t_lo) { const long long mt = m[L.moff + t_lo + t]; part += mt * (mt - 1) / 2; }
#include "wg_sum.inc"
  if (threadIdx.x == 0) {
    WG_TOTAL(test_pairs, CC_WAVES);
    const long long add[6] = {pairs & 0xffffffffLL, pairs >> 32, test_pairs, columns & 0xffff, (columns >> 16) & 0xffff, columns >> 32};
    for (int f = 0; f < 6; ++f)
      if (add[f]) ATOMIC_ADD((unsigned long long *)(counts + MPRG_CMP_COUNTS * l + f), (unsigned long long)add[f]);
  }
}
