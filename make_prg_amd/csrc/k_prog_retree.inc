// ---------------------------------------------------------------------------------------------------------------
// K-R  the identities of `from_msa --unaligned --progressive --retree` (make_prg_amd/from_msa/star_align.py holds the spec,
//      "Retree"; DESIGN.md §3b): all pairs of rows of an MSA's text compared column by column, into the tables mprg_prog_tree
//      reads.  Integers only.
//
// Texts are K-P's: R x W CELL CODES (0..11, '-' = 4), row-major, named by {buffer, offset} against the table `bufs`.
//
// k_prog_identities: one workgroup of 256 threads per work item {item, row block q}: the block's PI_BLOCK = 16 rows over a tile of
//   PI_TILE = 2 048 columns staged in LDS (32 KB), cells past the text's last column as '-'.  Every later row r' of the text (and
//   the block's own rows) is streamed through that tile by one wavefront, r' = first row + wavefront, + 4, ...: a lane takes 16
//   consecutive COLUMNS per step, so its four words of the staged rows are aligned in LDS whatever the text's offset and W are,
//   and the streamed row's 16 bytes are one load at whatever address they have (the last, partial chunk of a row byte by byte,
//   filled up with '-').  So nothing is masked: a '-' matches nothing.  Four cells per 32-bit operation: with
//   t = (x ^ y) | (x & 0x0C0C0C0C) a byte of t is 0 iff the two cells are equal and below 4, and (t + 0x7F7F7F7F) & 0x80808080 has
//   a bit per byte that is not.  A lane keeps the 16 counts of its columns against the 16 staged rows in registers; per streamed
//   row and tile they are added up over the wavefront by a halving exchange (lane ^ 32 keeps 8 of 16, lane ^ 16 4 of 8, ...: 17
//   shuffles for 16 sums) and lane 4 k holds row k's.  r' = r gives nw', r' > r the pair's s'; the first tile stores, a later
//   tile adds to what the same lane stored.  Every pair belongs to one lane of one workgroup: no atomics.
//   Global bytes: every streamed byte is compared against 16 rows, so R^2 W / 32 bytes are read for R^2 W / 2 cell compares.
// ---------------------------------------------------------------------------------------------------------------
#define PI_THREADS 256
#define PI_WAVES (PI_THREADS / 64)
#define PI_BLOCK MPRG_PI_BLOCK_ROWS
#define PI_TILE 2048                           // columns of the LDS tile
#define PI_TILE_WORDS (PI_TILE / 4)
#define PI_CHUNK 16                            // columns a lane takes per step

// the cells of four columns in which x and y hold the same code and that code is below 4
MPRG_DEV int pi_matches(uint32_t x, uint32_t y) {
  const uint32_t t = (x ^ y) | (x & 0x0C0C0C0Cu);
  return 4 - __popc((t + 0x7F7F7F7Fu) & 0x80808080u);
}

// n (0 .. 3) bytes at p, then '-' up to four
MPRG_DEV uint32_t pi_tail_word(const uint8_t *p, long long n) {
  uint32_t v = 0x04040404u;
  for (long long k = 0; k < n; ++k) v = (v & ~(0xFFu << (8 * k))) | ((uint32_t)p[k] << (8 * k));
  return v;
}

__global__ void __launch_bounds__(PI_THREADS) k_prog_identities(const int64_t *bufs, int n_bufs, const int64_t *items, int n_items,
                                                                const int32_t *work, const int32_t *leaf, long long leaf_words,
                                                                uint32_t *shared, long long shared_words, int64_t *nw, long long n_seqs,
                                                                int32_t *status) {
  SHARED(uint32_t, tile, PI_BLOCK * PI_TILE_WORDS);
  SHARED(int, bad, 1);
  static_assert(PI_BLOCK == 16, "the wavefront's halving exchange adds up 16 sums");
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const long long it = wk[0], q = wk[1];
  long long buf = 0, off = 0, R = 0, W = 0, loff = 0, first = 0, m = 0, toff = 0;
  int st = MPRG_PG_OK;
  if (it < 0 || it >= n_items) st = MPRG_PG_BAD_ITEM;
  else {
    const int64_t *I = items + MPRG_PI_ITEM_FIELDS * it;
    buf = I[0]; off = I[1]; R = I[2]; W = I[3]; loff = I[4]; first = I[5]; m = I[6]; toff = I[7];
    if (!pg_text_ok(bufs, n_bufs, buf, off, R, W) || q < 0 || q * PI_BLOCK >= R || loff < 0 || loff > leaf_words || R > leaf_words - loff ||
        m < 1 || m > 0x7fffffffLL || first < 0 || first > n_seqs || m > n_seqs - first || toff < 0 || toff > shared_words ||
        m * m > shared_words - toff)
      st = MPRG_PG_BAD_ITEM;
  }
  if (st != MPRG_PG_OK) {                                    // (the whole workgroup)
    if (threadIdx.x == 0) status[BLOCK_ID] = st;
    return;
  }
  const int32_t *lf = leaf + loff;
  ONE_THREAD bad[0] = 0;
  BARRIER();
  int out = 0;
  PAR_FOR(r, R) out |= lf[r] < 0 || lf[r] >= m;
  if (out) ATOMIC_OR(&bad[0], 1);
  BARRIER();
  if (bad[0]) st = MPRG_PG_BAD_ITEM;                         // (every thread: st stays workgroup-uniform)
  if (threadIdx.x == 0) status[BLOCK_ID] = st;
  if (st != MPRG_PG_OK) return;                              // (the whole workgroup)
  const uint8_t *text = (const uint8_t *)(uintptr_t)bufs[2 * buf] + off;
  const long long r0 = q * PI_BLOCK;
  const int rows = (int)(R - r0 < PI_BLOCK ? R - r0 : PI_BLOCK);
  const int lane = wave_lane(), wave = wave_id();
  for (long long c0 = 0; c0 < W; c0 += PI_TILE) {
    BARRIER();                                               // the tile before this one has been read
    PAR_FOR(i, PI_BLOCK * PI_TILE_WORDS) {
      const int r = (int)(i / PI_TILE_WORDS);
      const long long c = c0 + 4 * (i % PI_TILE_WORDS);
      uint32_t v = 0x04040404u;
      if (r < rows && c < W) {
        const uint8_t *p = text + (r0 + r) * W + c;
        if (c + 4 <= W) __builtin_memcpy(&v, p, 4);
        else v = pi_tail_word(p, W - c);
      }
      tile[i] = v;
    }
    BARRIER();
    const long long cols = W - c0 < PI_TILE ? W - c0 : PI_TILE;          // the tile's columns inside the text
    for (long long rs = r0 + wave; rs < R; rs += PI_WAVES) {             // (a whole wavefront)
      const uint8_t *row = text + rs * W + c0;
      int cnt[PI_BLOCK];
#pragma unroll
      for (int k = 0; k < PI_BLOCK; ++k) cnt[k] = 0;
      for (long long j = (long long)lane * PI_CHUNK; j < cols; j += 64 * PI_CHUNK) {
        uint32_t y[4];
        if (j + PI_CHUNK <= cols) __builtin_memcpy(y, row + j, PI_CHUNK);
        else {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const long long left = cols - j - 4 * u;
            y[u] = 0x04040404u;
            if (left >= 4) __builtin_memcpy(&y[u], row + j + 4 * u, 4);
            else if (left > 0) y[u] = pi_tail_word(row + j + 4 * u, left);
          }
        }
        const uint32_t *x = tile + j / 4;
#pragma unroll
        for (int k = 0; k < PI_BLOCK; ++k) {
#pragma unroll
          for (int u = 0; u < 4; ++u) cnt[k] += pi_matches(x[k * PI_TILE_WORDS + u], y[u]);
        }
      }
      // the wavefront's sums: a lane whose bit h of the lane index is set keeps the upper half of what it holds, the other lane
      // the lower half; after lane ^ 32, 16, 8, 4 a lane holds the sum of staged row (lane >> 2) & 15 over its quad's residue
#pragma unroll
      for (int h = 8, d = 32; h >= 1; h >>= 1, d >>= 1) {
        const bool up = (lane & d) != 0;
#pragma unroll
        for (int k = 0; k < h; ++k) {
          const int keep = up ? cnt[k + h] : cnt[k], send = up ? cnt[k] : cnt[k + h];
          cnt[k] = keep + __shfl_xor(send, d);
        }
      }
      int sum = cnt[0];
      sum += __shfl_xor(sum, 2);
      sum += __shfl_xor(sum, 1);
      const int k = lane >> 2;
      const long long r = r0 + k;
      if ((lane & 3) == 0 && k < rows && r <= rs) {
        if (r == rs) {
          int64_t *dst = nw + first + lf[r];
          *dst = (c0 ? *dst : 0) + sum;
        } else {
          const long long a = lf[r], b = lf[rs];
          uint32_t *dst = shared + toff + (a < b ? a * m + b : b * m + a);
          *dst = (c0 ? *dst : 0u) + (uint32_t)sum;
        }
      }
    }
  }
}
