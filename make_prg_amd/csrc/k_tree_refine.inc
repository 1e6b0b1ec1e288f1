// ---------------------------------------------------------------------------------------------------------------
// K-T  tree refinement of `from_msa --unaligned --progressive --refine-tree` (make_prg_amd/from_msa/star_align.py holds the spec,
//      "Tree refinement"; DESIGN.md §3b): an MSA's text split into the two sub-alignments of a guide-tree edge, and the objective S
//      of a text whose rows count w times.  The realignment of the two halves is k_prog_columns(_weighted)', the DP kernels' and
//      k_prog_rows' (K-P), unchanged.  Integers only.
//
// Texts are K-P's: R x W CELL CODES (0..11, '-' = 4), row-major, named by {buffer, offset} against the table `bufs`.  A text may
// have 4 096 rows and 10^6 columns: nothing here keeps a text, a row or a column set in LDS.
//
// mprg_tree_split is three launches over one work table {item, 256-column tile}:
// k_tree_split_flags: one workgroup per (item, tile), thread = column, the rows walked in order (a row of the tile is 256
//   contiguous bytes: coalesced; k_refine_counts' access pattern).  Every cell is read ONCE for both column sets: a row's side
//   byte (workgroup-uniform) says which of the column's two keep flags a cell that is not '-' sets.  Writes the column's flags
//   (bit 0: Y keeps it, bit 1: X does) and the tile's two counts of kept columns (a ballot per wavefront, added up through LDS).
// k_tree_split_scan: one wavefront per item: the side bytes checked and counted, the tiles' counts turned into exclusive prefixes
//   in place (64 tiles per wave scan), W_Y and W_X, the output range checked; writes the item's status and widths.
// k_tree_split_rows: one workgroup per (item, tile) of an item whose status is OK: a kept column's place is its tile's prefix
//   plus its rank among the tile's kept columns (a workgroup scan per side); the rows walked in order again, row r of side s
//   writes its cell to the s text's next row: the lanes of kept columns write consecutive bytes.  A cell is read a second time
//   only where its side keeps the column; every output byte is written once.
// So a cell costs at most two byte reads and one byte written, a row one side byte per tile and launch, a column one flag byte.
//
// k_tree_objective: k_refine_counts' tile walk on cell codes with row r counted weights[r] times and E all-gap rows more: the
//   five counts in registers, a row's run starts from the lane below by a shuffle, one 64-bit integer atomic per tile.  The
//   workgroup first adds up the weights (wg_sum.inc), as k_prog_columns_weighted does.
// ---------------------------------------------------------------------------------------------------------------
#define TS_THREADS 256
#define TS_WAVES (TS_THREADS / 64)

// a split item's fields against the buffers: the text, its R side bytes, its W flags and its tiles + 1 table entries
struct TsItem { long long buf, off, R, W, soff, ooff, coff, toff, nt; };
MPRG_DEV bool ts_item_ok(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items, long long it, long long sides_bytes,
                         long long n_cols, long long n_tiles, TsItem &t) {
  if (it < 0 || it >= n_items) return false;
  const int64_t *I = items + MPRG_TS_ITEM_FIELDS * it;
  t.buf = I[0]; t.off = I[1]; t.R = I[2]; t.W = I[3]; t.soff = I[4]; t.ooff = I[5]; t.coff = I[6]; t.toff = I[7];
  if (!pg_text_ok(bufs, n_bufs, t.buf, t.off, t.R, t.W) || t.R < 2) return false;
  t.nt = (t.W + 255) / 256;
  return t.soff >= 0 && t.soff <= sides_bytes && t.R <= sides_bytes - t.soff && t.coff >= 0 && t.coff <= n_cols && t.W <= n_cols - t.coff &&
         t.toff >= 0 && t.toff <= n_tiles && t.nt + 1 <= n_tiles - t.toff;
}

__global__ void __launch_bounds__(TS_THREADS) k_tree_split_flags(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items,
                                                                 const int32_t *work, const uint8_t *sides, long long sides_bytes,
                                                                 uint8_t *flags, long long n_cols, int32_t *tiles, long long n_tiles) {
  SHARED(int, cnt, 2 * TS_WAVES);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long tile = wk[1];
  TsItem t;
  if (!ts_item_ok(bufs, n_bufs, items, n_items, wk[0], sides_bytes, n_cols, n_tiles, t) || tile < 0 || tile >= t.nt) return;   // (the whole workgroup)
  const long long c = tile * 256 + (long long)threadIdx.x;
  const bool in = c < t.W;
  const uint8_t *text = (const uint8_t *)(uintptr_t)bufs[2 * t.buf] + t.off + (in ? c : 0);
  const uint8_t *side = sides + t.soff;
  unsigned keep = 0;
#pragma unroll 4
  for (long long r = 0; r < t.R; ++r) {
    const unsigned sd = side[r];                             // (0: Y, 1: X; anything else sets no flag, k_tree_split_scan refuses it)
    const unsigned ch = text[r * t.W];
    if (ch != (unsigned)C_GAP && sd < 2u) keep |= 1u << sd;
  }
  if (!in) keep = 0;
  if (in) flags[t.coff + c] = (uint8_t)keep;
  const int ny = __popcll(__ballot(keep & 1u)), nx = __popcll(__ballot(keep & 2u));
  if (wave_lane() == 0) { cnt[2 * wave_id()] = ny; cnt[2 * wave_id() + 1] = nx; }
  BARRIER();
  if (threadIdx.x == 0) {
    int sy = 0, sx = 0;
    for (int w = 0; w < TS_WAVES; ++w) { sy += cnt[2 * w]; sx += cnt[2 * w + 1]; }
    tiles[2 * (t.toff + tile)] = sy;
    tiles[2 * (t.toff + tile) + 1] = sx;
  }
}

__global__ void __launch_bounds__(TS_THREADS) k_tree_split_scan(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items,
                                                                const uint8_t *sides, long long sides_bytes, long long n_cols,
                                                                int32_t *tiles, long long n_tiles, long long out_bytes, int64_t *widths,
                                                                int32_t *status, int have_counts) {
  const long long it = (long long)BLOCK_ID * TS_WAVES + wave_id();
  if (it >= n_items) return;                                 // (a whole wavefront)
  const int lane = wave_lane();
  TsItem t;
  // (have_counts 0: an empty work table, so no flags launch wrote the tiles' counts: every item is refused)
  if (!have_counts || !ts_item_ok(bufs, n_bufs, items, n_items, it, sides_bytes, n_cols, n_tiles, t)) {
    if (lane == 0) status[it] = MPRG_PG_BAD_ITEM;
    return;
  }
  long long ry = 0;
  bool bad = false;
  for (long long r0 = 0; r0 < t.R; r0 += WAVE) {
    const long long r = r0 + lane;
    const unsigned sd = r < t.R ? (unsigned)sides[t.soff + r] : 1u;
    bad |= sd > 1u;
    ry += __popcll(__ballot(r < t.R && sd == 0u));
  }
  bad = __ballot(bad) != 0ull;
  if (bad || ry < 1 || ry >= t.R) { if (lane == 0) status[it] = MPRG_PG_BAD_ITEM; return; }   // a side byte above 1, a side without rows
  int32_t *T = tiles + 2 * t.toff;
  int cy = 0, cx = 0;
  for (long long k0 = 0; k0 < t.nt; k0 += WAVE) {
    const long long k = k0 + lane;
    const int vy = k < t.nt ? T[2 * k] : 0, vx = k < t.nt ? T[2 * k + 1] : 0;
    const int iy = wave_scan_incl(vy), ix = wave_scan_incl(vx);
    if (k < t.nt) { T[2 * k] = cy + iy - vy; T[2 * k + 1] = cx + ix - vx; }
    cy += __shfl(iy, 63);
    cx += __shfl(ix, 63);
  }
  const long long wy = cy, wx = cx, rx = t.R - ry;
  int st = MPRG_PG_OK;
  if (wy < 1 || wx < 1 || wy > t.W || wx > t.W) st = MPRG_PG_BAD_ITEM;            // a side without a kept column (or counts no flags launch wrote)
  else if (t.ooff < 0 || t.ooff > out_bytes || ry * wy + rx * wx > out_bytes - t.ooff) st = MPRG_PG_NO_SPACE;   // (at most R W: no overflow)
  if (lane == 0) {
    status[it] = st;
    if (st == MPRG_PG_OK) { T[2 * t.nt] = (int32_t)ry; T[2 * t.nt + 1] = (int32_t)rx; widths[2 * it] = wy; widths[2 * it + 1] = wx; }
  }
}

__global__ void __launch_bounds__(TS_THREADS) k_tree_split_rows(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items,
                                                                const int32_t *work, const uint8_t *sides, long long sides_bytes,
                                                                const uint8_t *flags, long long n_cols, const int32_t *tiles,
                                                                long long n_tiles, const int64_t *widths, const int32_t *status,
                                                                uint8_t *out) {
  SHARED(int, scratch, 17);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long it = wk[0], tile = wk[1];
  TsItem t;
  if (!ts_item_ok(bufs, n_bufs, items, n_items, it, sides_bytes, n_cols, n_tiles, t) || tile < 0 || tile >= t.nt ||
      status[it] != MPRG_PG_OK) return;                      // (the whole workgroup)
  const long long c = tile * 256 + (long long)threadIdx.x;
  const bool in = c < t.W;
  const unsigned keep = in ? (unsigned)flags[t.coff + c] : 0u;
  const int32_t *T = tiles + 2 * t.toff;
  const long long wy = widths[2 * it], wx = widths[2 * it + 1], ry = T[2 * t.nt], rx = T[2 * t.nt + 1];
  int total = 0;
  const long long dy = (long long)T[2 * tile] + block_scan_excl((int)(keep & 1u), scratch, &total);
  const long long dx = (long long)T[2 * tile + 1] + block_scan_excl((int)((keep >> 1) & 1u), scratch, &total);
  // (the scan's prefixes are always in range; tables of another origin cannot make a lane write outside the two texts)
  const bool ky = (keep & 1u) && dy >= 0 && dy < wy, kx = (keep & 2u) && dx >= 0 && dx < wx;
  const uint8_t *text = (const uint8_t *)(uintptr_t)bufs[2 * t.buf] + t.off + (in ? c : 0);
  const uint8_t *side = sides + t.soff;
  uint8_t *oy = out + t.ooff + dy, *ox = out + t.ooff + ry * wy + dx;
  long long ny = 0, nx = 0;                                  // rows of either side above row r
  for (long long r = 0; r < t.R; ++r) {
    if (side[r] == 0) {                                      // (workgroup-uniform)
      if (ky && ny < ry) oy[ny * wy] = text[r * t.W];
      ++ny;
    } else {
      if (kx && nx < rx) ox[nx * wx] = text[r * t.W];
      ++nx;
    }
  }
}

__global__ void __launch_bounds__(TS_THREADS) k_tree_objective(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items,
                                                               const int32_t *work, const int32_t *weights, long long weights_words,
                                                               int64_t *sums, int32_t *status) {
  SHARED(long long, red, TS_WAVES);
  SHARED(int, low, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long it = wk[0], tile = wk[1];
  long long buf = 0, off = 0, R = 0, W = 0, woff = 0, S = 0, E = 0;
  int st = MPRG_PG_OK;
  if (it < 0 || it >= n_items) st = MPRG_PG_BAD_ITEM;
  else {
    const int64_t *I = items + MPRG_TS_OBJ_FIELDS * it;
    buf = I[0]; off = I[1]; R = I[2]; W = I[3]; woff = I[4]; S = I[5]; E = I[6];
    // rows in all: S + E <= 2^20, and 32 (S + E)^2 W < 2^63: |S(A)| <= (20 + 11) rows^2 W
    if (!pg_text_ok(bufs, n_bufs, buf, off, R, W) || tile < 0 || tile * 256 >= W || woff < 0 || woff > weights_words ||
        R > weights_words - woff || S < R || E < 0 || E > PG_MAX_ROWS || S > PG_MAX_ROWS - E || (S + E) * (S + E) > (1LL << 58) / W)
      st = MPRG_PG_BAD_ITEM;
  }
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
  WG_TOTAL(sum, TS_WAVES);                                   // (every thread: st stays workgroup-uniform)
  if (low[0] || sum != S) st = MPRG_PG_BAD_ITEM;
  if (threadIdx.x == 0) status[BLOCK_ID] = st;
  if (st != MPRG_PG_OK) return;                              // (the whole workgroup)
  BARRIER();                                                 // red is written again below
  const long long c = tile * 256 + (long long)threadIdx.x;
  const bool in = c < W;
  const int lane = wave_lane();
  const uint8_t *text = (const uint8_t *)(uintptr_t)bufs[2 * buf] + off;
  const long long rows = S + E;
  long long cnt[5] = {0, 0, 0, 0, E};
  long long starts = 0;
  for (long long r = 0; r < R; ++r) {
    const uint8_t *row = text + r * W;
    const long long w = wt[r];
    const unsigned ch = in ? (unsigned)row[c] : 0u;
    unsigned left = __shfl_up(ch, 1);
    if (lane == 0) left = in && c > 0 ? (unsigned)row[c - 1] : 0u;
#pragma unroll
    for (unsigned x = 0; x < 5; ++x) cnt[x] += ch == x ? w : 0;
    starts += in && ch == (unsigned)C_GAP && left != (unsigned)C_GAP ? w : 0;
  }
  if (c == 0) starts += E;                                   // an all-gap row is one run
  part = 0;
  if (in) {
    const long long a = cnt[0], b = cnt[1], g = cnt[2], t = cnt[3], gap = cnt[4];
    const long long same = (a * (a - 1) + b * (b - 1) + g * (g - 1) + t * (t - 1)) / 2;
    const long long diff = a * b + a * g + a * t + b * g + b * t + g * t;
    part = 2 * (20 * same - 9 * diff - 10 * gap * (rows - gap));
  }
  part -= 11 * (rows - 1) * starts;
#include "wg_sum.inc"
  if (threadIdx.x == 0) {
    WG_TOTAL(s, TS_WAVES);
    ATOMIC_ADD((unsigned long long *)(sums + it), (unsigned long long)s);
  }
}
