// ---------------------------------------------------------------------------------------------------------------
// K3  ungap rows + group identical rows
//     reference from_msa/cluster_sequences.py:220-233 (ungapped / gapped row dictionaries, first-appearance order),
//     utils/seq_utils.py:45-46 (ungap), :58-70 (unique gapped / ungapped counts), leaf emission
//     recursion_tree.py:272-274 -> utils/seq_utils.py:155-158 (order-preserving dedupe of ungapped rows)
//
// K3a (k_ungap_hash): a group of 8-64 LANES per row (a wavefront takes 8 rows of a narrow view at once, one row of a wide
// one), a lane takes four consecutive cells of the row-major copy per step (see the kernel): the ungapped row comes out
// ROW-MAJOR (row i at U + i * upitch, upitch = columns rounded up to 16), so that the
// comparison below and the k-mer kernels read it with wide, coalesced loads.  Two 64-bit hashes per row (ungapped content,
// gapped content) are sums over the row's WORDS of a mixed (word, position) value — commutative, so a wave reduction gives
// them.  A hash is only a FILTER: rows are declared identical after an exact comparison, so the grouping is exact.
// K3b (k_ungap_dedupe): one workgroup per view.  An open-addressing table in LDS keyed by (hash, length) keeps the
// SMALLEST row index per key (atomicMin: order independent); a row's nominee is that row.  Every nominated pair is
// compared 16 bytes per lane; a refuted nominee (a 64-bit collision: practically never) sends the view to the exact
// all-pairs search.  First-appearance lists come from workgroup prefix sums over "is the first of its group" flags.
// K3n (k_rows_narrow, k_rows_narrow_s), K3w (k_rows_wave, k_dedupe_wave): NARROW views (at most RV_COLS columns and DD_ROWS rows: the rule
// below the root) take all of the above in ONE launch — a workgroup per view, or a wavefront for a view of at most 64 rows —, with a
// LANE per row for the row phase: a lane that walks its row alone keeps the kept-byte count, both hashes and the compaction state in
// registers (no prefix sum over a group of lanes, no second pass over the compacted rows), and the hashes are in LDS when the dedupe
// table is built.  Same hashes, lengths, rows and lists as K3a + K3a' + K3b write.  MPRG_ROW_VIEWS=0 leaves every view to those.
// K3m (k_rows_mid): MID-WIDTH views (RV_COLS < columns <= RM_COLS, at most RV_ROWS_S rows: most of the root's non-match intervals that are
// not narrow) in one launch too — a group of lanes per row as in K3a, but 16 cells per lane, two rows' loads in flight per lane, the
// compaction through a staging row in LDS, from which the ungapped hash is taken.  MPRG_ROW_MID=0 leaves them to K3a + K3a' + K3b.
// ---------------------------------------------------------------------------------------------------------------
MPRG_DEV uint64_t hash_mix(uint64_t x) {          // splitmix64 finaliser
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL; x ^= x >> 27; x *= 0x94d049bb133111ebULL; x ^= x >> 31;
  return x;
}
#ifdef MPRG_TEST_WEAK_HASH      // test-only build: all rows collide, so the exact-comparison paths decide alone
#define MPRG_HASH_MIX(x) 1ULL
#else
#define MPRG_HASH_MIX(x) hash_mix(x)
#endif
MPRG_DEV int u_pitch(int n_cols) { return (n_cols + 15) & ~15; }
MPRG_DEV uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}

// K3a  ungap + gapped-row hash: one workgroup per (view, 256-row chunk), a group of lanes per row.
//      A lane takes FOUR consecutive cells per step (one unaligned 4-byte load: 64 lanes read 256 contiguous bytes of
//      a row): the gap bytes of the word are found with a few SWAR operations, the lanes' kept-counts are prefix-summed
//      over the row's group, and the kept bytes go out as one word (no gap in it: the common case) or byte by byte.  The gapped
//      hash mixes one WORD (4 cells + its column) per lane and step, not one cell.  The ungapped hash is taken from the
//      compacted rows by k_ungap_dedupe, 8 bytes per lane (it must not depend on how a row's characters fell into words).
#define UG_ROWS 256
// rows per work item {view, row chunk} of the row kernels below: 256; 8 for a WIDE view (a wavefront takes a row of thousands of
// columns alone — two rows per wavefront of a chunk —, and a view of thousands of such rows would otherwise be a few dozen workgroups:
// 32-row chunks left the 10 000 x 20 000 alignment's k_ungap_hash at 0.5 ms, five wavefronts per CU each waiting for its own loads)
#define UG_WIDE 4096
#define UG_ROWS_WIDE 8
#define UG_BATCH 4                     // steps of a row whose words a lane of k_ungap_hash keeps in flight
MPRG_DEV int ug_chunk_rows(long long n_cols) { return n_cols > UG_WIDE ? UG_ROWS_WIDE : UG_ROWS; }
MPRG_DEV long long ug_chunks(long long S, long long n_cols) { const int ch = ug_chunk_rows(n_cols); return (S + ch - 1) / ch; }
MPRG_DEV uint64_t hash_word(uint64_t w, unsigned pos) { return MPRG_HASH_MIX(w ^ ((uint64_t)(pos + 1) << 40)); }
// gcodes_all (optional): a DENSE copy of the view's gapped rows in the layout of the ungapped ones (row i at aux0 + i * upitch):
// the kernels that visit the view afterwards (gapped comparison here, cluster_further) then read one contiguous block of a
// few KB instead of a narrow slice of every arena row (64-byte sectors for 30 useful bytes).
// small views (the rule below the first levels): all three stages by ONE wavefront, DW_WAVES views per workgroup (k_dedupe_wave
// below); the workgroup-per-chunk / workgroup-per-view kernels leave them alone when bit 0 of `form` is set
// (measured on MI355X, 7 500 config-C alignments per pass: the level of ~100-row x ~40-column views 5.1 ms by workgroups, 7.7 ms by
//  wavefronts — a wavefront alone walks such a view's three stages too long; the level of ~25 x 5 views 2.2 -> 1.6 ms)
#define DW_WAVES 4
#define DW_ROWS 64
#define DW_SLOTS 128
#define DW_COLS 64
MPRG_DEV bool dw_is_small(long long S, long long n) { return S >= 1 && S <= DW_ROWS && n >= 1 && n <= DW_COLS; }
// narrow views (the rule of the first levels below the root: ~100 rows x ~40 columns): all three stages by ONE workgroup, a LANE per
// row (k_rows_narrow below).  A lane that walks its row alone needs no scan over a group of lanes: the kept-byte count, both hashes and
// the compaction state stay in its registers, and the hashes are in the workgroup's LDS when the dedupe table is built.
#define DD_ROWS 512
#define DD_SLOTS 1024                  // LDS table: twice the rows
#define RV_COLS 64
#define RV_ROWS_S 128                  // ... of at most so many rows by k_rows_narrow_s: a quarter of the LDS, four times the workgroups per CU
#define RV_SLOTS_S 256
// `form` of the row kernels' launches: bit 0 = the small views are k_dedupe_wave's / k_rows_wave's, bit 1 = the narrow ones
// k_rows_narrow's / k_rows_narrow_s's (small views stay with the wavefront kernels where both are on), bit 2 = the mid-width ones k_rows_mid's
#define RF_WAVE 1
#define RF_ROWS 2
MPRG_DEV bool rv_is_narrow(long long S, long long n) { return n >= 1 && n <= RV_COLS && S >= 1 && S <= DD_ROWS; }
MPRG_DEV bool rv_takes(int form, long long S, long long n) { return (form & RF_ROWS) && rv_is_narrow(S, n) && !((form & RF_WAVE) && dw_is_small(S, n)); }
// mid-width views (the children of the root's non-match intervals that are wider than RV_COLS: ~100 rows x 65 .. a few hundred columns):
// all three stages by ONE workgroup, a group of lanes per row and 16 cells per lane, so that a row is one step (k_rows_mid below);
// bit 2 of `form`.  Wider than RM_COLS or more than RV_ROWS_S rows: the general launches.
#define RM_COLS 1024                   // 64 lanes x 16 cells: the widest row that is one step of a wavefront
#define RF_MID 4
MPRG_DEV bool rm_is_mid(long long S, long long n) { return n > RV_COLS && n <= RM_COLS && S >= 1 && S <= RV_ROWS_S; }
MPRG_DEV bool rm_takes(int form, long long S, long long n) { return (form & RF_MID) && rm_is_mid(S, n); }
MPRG_DEV bool rows_elsewhere(int form, long long S, long long n) {
  return ((form & RF_WAVE) && dw_is_small(S, n)) || rv_takes(form, S, n) || rm_takes(form, S, n);
}
// rows [r0, r0 + chunk) of the view, wavefront `wv` of `n_waves`
MPRG_DEV void ug_hash_rows(const uint8_t *arena, const ViewD &d, const int32_t *rowidx, int r0, int chunk, int wv, int n_waves,
                           uint8_t *ucodes_all, uint64_t *hashes, int32_t *ulen_all, uint8_t *gcodes_all) {
  const int n = d.n_cols, S = d.n_rows;
  const int upitch = u_pitch(n);
  uint8_t *U = ucodes_all + d.aux0;
  uint64_t *hg = hashes + 2 * d.row_off + S;
  int32_t *ulen = ulen_all + d.row_off;
  const int lane = wave_lane();
  // lanes per row: a step covers 4 cells per lane, so a row of a narrow view (the rule below the root: a few dozen columns)
  // needs 8 or 16 lanes, and a wavefront takes 8 or 4 such rows at once; prefix sums and reductions run per group of G lanes
  int G = WAVE;
  while (G > 8 && 4 * (G >> 1) >= n) G >>= 1;
  const int rows_per_wave = WAVE / G, gl = lane & (G - 1), sub = lane / G;
  for (int ib = r0 + wv * rows_per_wave; ib < r0 + chunk && ib < S; ib += n_waves * rows_per_wave) {   // uniform per wave
    const int i = ib + sub;
    const bool live = i < S && i < r0 + chunk;
    const uint8_t *src = arena + d.rm + (long long)(live ? view_row(d, rowidx, i) : 0) * d.pitchC + d.col0;
    uint8_t *dst = U + (long long)i * upitch;
    uint8_t *gdst = gcodes_all ? gcodes_all + d.aux0 + (long long)i * upitch : nullptr;
    uint64_t g = 0;
    int len = 0;
    // one step of the row: the word w of columns c0 + 4 gl .. + 3 (loaded by the caller), its gapped hash, the kept bytes to their place
#define UG_STEP(w_, c0_) do {                                                                                                          \
      const int c = (c0_) + 4 * gl;                                                                                                    \
      uint32_t w = (w_);                                                                                                               \
      if (live && c < n) {                                                                                                             \
        if (c + 4 > n) {                             /* the row's last word: cells past n count as gaps */                             \
          const uint32_t keep = 0xffffffffu >> (8 * (c + 4 - n));                                                                      \
          w = (w & keep) | (0x04040404u & ~keep);                                                                                      \
        }                                                                                                                              \
        g += hash_word(w, (unsigned)c);                                                                                                \
        if (gdst) __builtin_memcpy(gdst + c, &w, 4);   /* (cells past n are gaps; upitch >= n rounded up to 16) */                     \
      }                                                                                                                                \
      const uint32_t v = w ^ 0x04040404u;            /* zero bytes = gaps */                                                           \
      const uint32_t gap = ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;   /* 0x80 in every gap byte, exactly */             \
      const int kept = 4 - __popc(gap);                                                                                                \
      int incl = kept;                               /* inclusive prefix sum over the row's G lanes */                                 \
      for (int dd = 1; dd < G; dd <<= 1) { const int y = __shfl_up(incl, dd, G); if (gl >= dd) incl += y; }                            \
      const int at = len + incl - kept;                                                                                                \
      if (live) {                                                                                                                      \
        if (kept == 4) __builtin_memcpy(dst + at, &w, 4);                                                                              \
        else if (kept) {                                                                                                               \
          int o = at;                                                                                                                  \
          _Pragma("unroll") for (int u = 0; u < 4; ++u) if (!((gap >> (8 * u + 7)) & 1u)) dst[o++] = (uint8_t)(w >> (8 * u));        \
        }                                                                                                                              \
      }                                                                                                                                \
      len += __shfl(incl, G - 1, G);                                                                                                   \
    } while (0)
    if (n <= 4 * G) {                                  // the rule below the root: the row is ONE step
      uint32_t w0 = 0x04040404u;                       // four gaps: what a lane past the end contributes
      if (live && 4 * gl < n) __builtin_memcpy(&w0, src + 4 * gl, 4);      // the arena is padded: the bytes past n exist
      UG_STEP(w0, 0);
    } else {
      // UG_BATCH steps of a wide row per round trip: their words first (a row of 20 000 columns is 79 steps of 256 bytes; one step per
      // trip left a wavefront waiting a memory latency per 256 bytes: 0.9 TB/s on the 10 000 x 20 000 alignment), then each step's scan
      for (int cb = 0; cb < n; cb += UG_BATCH * 4 * G) {
        uint32_t wq[UG_BATCH];
#pragma unroll
        for (int q = 0; q < UG_BATCH; ++q) {
          const int c = cb + q * 4 * G + 4 * gl;
          wq[q] = 0x04040404u;
          if (live && c < n) __builtin_memcpy(&wq[q], src + c, 4);
        }
#pragma unroll
        for (int q = 0; q < UG_BATCH; ++q) {
          if (cb + q * 4 * G >= n) break;              // (uniform per wavefront)
          UG_STEP(wq[q], cb + q * 4 * G);
        }
      }
    }
#undef UG_STEP
    for (int dd = G >> 1; dd >= 1; dd >>= 1) g += (uint64_t)__shfl_xor((unsigned long long)g, dd, G);
    if (live && gl == 0) { hg[i] = g; ulen[i] = len; }
  }
}
KERNEL(k_ungap_hash, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, const int32_t *work,
       uint8_t *ucodes_all, uint64_t *hashes, int32_t *ulen_all, uint8_t *gcodes_all, int form, DsCount dc) {
  DS_GUARD(dc, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const ViewD d = load_view(views, wk[0]);
  if (rows_elsewhere(form, d.n_rows, d.n_cols)) return;
  const int chunk = ug_chunk_rows(d.n_cols);
  ug_hash_rows(arena, d, rowidx, wk[1] * chunk, chunk, wave_id(), N_THREADS / WAVE, ucodes_all, hashes, ulen_all, gcodes_all);
}

// K3a'  ungapped hashes from the compacted rows: the same (view, 256-row chunk) work items as k_ungap_hash, a group of lanes per
//       row, 8 bytes per lane (rows are 16-byte aligned; the bytes past a row's length are masked off).  Until round 4 the
//       view's ONE k_ungap_dedupe workgroup did this for all its rows: 200 MB through one workgroup for the 10 000 x 20 000
//       alignment of BASELINE config D (100 ms of its 150 ms).
MPRG_DEV void ug_hash_u_rows(const ViewD &d, int r0, int chunk, int wv, int n_waves, const uint8_t *ucodes_all, uint64_t *hashes,
                             const int32_t *ulen_all) {
  const int n = d.n_cols, S = d.n_rows, upitch = u_pitch(n);
  const uint8_t *U = ucodes_all + d.aux0;
  uint64_t *hu_w = hashes + 2 * d.row_off;
  const int32_t *ulen = ulen_all + d.row_off;
  const int lane = wave_lane();
  int G = WAVE;                                        // lanes per row: 8 bytes per lane and step (see k_ungap_hash)
  while (G > 4 && 8 * (G >> 1) >= n) G >>= 1;
  const int rows_per_wave = WAVE / G, gl = lane & (G - 1), sub = lane / G;
  for (int ib = r0 + wv * rows_per_wave; ib < r0 + chunk && ib < S; ib += n_waves * rows_per_wave) {
    const int i = ib + sub;
    const bool live = i < S && i < r0 + chunk;
    const int len = live ? ulen[i] : 0;
    const uint8_t *row = U + (long long)(live ? i : 0) * upitch;
    uint64_t a = 0;
    for (int p = 8 * gl; p < len; p += 8 * G) {
      uint64_t w = *(const uint64_t *)(row + p);
      if (p + 8 > len) w &= 0xffffffffffffffffULL >> (8 * (p + 8 - len));
      a += hash_word(w, (unsigned)p);
    }
    for (int dd = G >> 1; dd >= 1; dd >>= 1) a += (uint64_t)__shfl_xor((unsigned long long)a, dd, G);
    if (live && gl == 0) hu_w[i] = a;
  }
}
KERNEL(k_ungap_hash_u, const int64_t *views, const int32_t *work, const uint8_t *ucodes_all, uint64_t *hashes, const int32_t *ulen_all,
       int form, DsCount dc) {
  DS_GUARD(dc, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const ViewD d = load_view(views, wk[0]);
  if (rows_elsewhere(form, d.n_rows, d.n_cols)) return;
  const int chunk = ug_chunk_rows(d.n_cols);
  ug_hash_u_rows(d, wk[1] * chunk, chunk, wave_id(), N_THREADS / WAVE, ucodes_all, hashes, ulen_all);
}

// K3b  groups of identical rows + first-appearance lists, one view per workgroup
#define DD_EMPTY 0xffffffffffffffffULL
// 16 ungapped characters of rows i and j differ?  (U is row-major, rows 16-byte aligned)
MPRG_DEV bool dd_diff_u16(const uint8_t *U, int upitch, int i, int j, int p0, int len) {
  const uint4 x = *(const uint4 *)(U + (long long)i * upitch + p0), y = *(const uint4 *)(U + (long long)j * upitch + p0);
  unsigned m[4] = {x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w};
  const int valid = len - p0;          // bytes of this block inside the row (the rest is stale scratch)
  if (valid >= 16) return (m[0] | m[1] | m[2] | m[3]) != 0;
  unsigned bad = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int vb = valid - 4 * w;
    const unsigned keep = vb >= 4 ? 0xffffffffu : (vb <= 0 ? 0u : ((1u << (8 * vb)) - 1u));
    bad |= m[w] & keep;
  }
  return bad != 0;
}
// K3a''  groups of identical rows in a BIG view (more rows than k_ungap_dedupe's LDS table holds: a root-level view of thousands
//        of rows): the smallest earlier row with identical content, ungapped (rep_u) and gaps included (rep_g), by an exact scan —
//        one {view, row chunk} work item per workgroup, thread = row; the candidates' hashes and lengths pass through LDS a chunk at a
//        time (every thread reads the same entry: a broadcast), symbols are compared only when hash and length agree.  Chunks in
//        ascending order: the first hit is the smallest j.  Until round 4 the view's ONE k_ungap_dedupe workgroup did this for
//        all its rows (23 ms for the 10 000 rows of BASELINE config D).  Small views return at once.
KERNEL(k_dedupe_scan_big, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, const int32_t *work,
       const uint8_t *ucodes_all, const uint64_t *hashes, const int32_t *ulen_all, int32_t *rep_u_all, int32_t *rep_g_all, DsCount dc) {
  DS_GUARD(dc, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const ViewD d = load_view(views, wk[0]);
  const int n = d.n_cols, S = d.n_rows, chunk = ug_chunk_rows(n), r0 = wk[1] * chunk, upitch = u_pitch(n);
  if (S <= DD_ROWS) return;
  const uint8_t *U = ucodes_all + d.aux0;
  const uint64_t *hu = hashes + 2 * d.row_off, *hg = hu + S;
  const int32_t *ulen = ulen_all + d.row_off;
  __shared__ uint64_t s_hu[DD_ROWS], s_hg[DD_ROWS];
  __shared__ int32_t s_len[DD_ROWS];
  __shared__ int32_t s_ru[UG_ROWS], s_rg[UG_ROWS];             // smallest identical earlier row found so far, per row of the chunk
  const int i_end = r0 + chunk < S ? r0 + chunk : S;          // this workgroup's rows: [r0, i_end); their candidates: j < i_end - 1
  // thread = (row of the chunk, class of candidates): a chunk of a WIDE view is 8 rows, so 32 threads share a row's candidates
  // (candidate t of a block goes to the thread with t % G == its class) — thread = row left most of the 256 threads idle while a few
  // walked all earlier rows alone (1.2 ms for the 10 000 rows of BASELINE config D).  Each class keeps the smallest identical row it
  // meets; the classes' minimum (atomicMin in LDS) is the smallest of all.
  const int G = N_THREADS / chunk > 0 ? N_THREADS / chunk : 1, ri_ = (int)threadIdx.x % chunk, cls = (int)threadIdx.x / chunk;
  const int i = r0 + ri_;
  const bool live = cls < G && i < i_end;
  if (threadIdx.x < UG_ROWS) { s_ru[threadIdx.x] = 0x7fffffff; s_rg[threadIdx.x] = 0x7fffffff; }
  const uint64_t a = live ? hu[i] : 0, g = live ? hg[i] : 0;
  const int len = live ? ulen[i] : 0;
  const uint8_t *ri = arena + d.rm + (long long)(live ? view_row(d, rowidx, i) : 0) * d.pitchC + d.col0;
  for (int c0 = 0; c0 < i_end - 1; c0 += DD_ROWS) {           // uniform trip count
    BARRIER();
    // (settled in an EARLIER block — read between the barriers: the classes of a row must all scan the block in which one of them finds
    //  the first identical row, or a smaller one of another class would be skipped)
    const bool done_u = s_ru[ri_] != 0x7fffffff, done_g = s_rg[ri_] != 0x7fffffff;
    PAR_FOR(t, DD_ROWS) { if (c0 + t < S) { s_hu[t] = hu[c0 + t]; s_hg[t] = hg[c0 + t]; s_len[t] = ulen[c0 + t]; } }
    BARRIER();
    if (!live || i <= c0) continue;
    const int j1 = (i < c0 + DD_ROWS ? i : c0 + DD_ROWS) - c0;
    // (the filter pass is branch-free, eight candidates of the class per step: the first candidate whose hash and length agree;
    //  symbols are compared only then — and the scan goes on behind a candidate that turns out to differ, a 64-bit collision.
    //  Blocks in ascending order: a row settled in an earlier block is done.)
    if (!done_u) {
      for (int t0 = cls; t0 < j1;) {
        int hit = 0x7fffffff;
        for (int t = t0; t < j1 && hit == 0x7fffffff; t += 8 * G) {
#pragma unroll
          for (int q = 7; q >= 0; --q) { const int tq = t + q * G; if (tq < j1 && s_hu[tq] == a && s_len[tq] == len) hit = tq; }
        }
        if (hit == 0x7fffffff) break;
        bool bad = false;
        for (int p = 0; p < len && !bad; p += 16) bad = dd_diff_u16(U, upitch, i, c0 + hit, p, len);
        if (!bad) { atomicMin(&s_ru[ri_], c0 + hit); break; }
        t0 = hit + G;
      }
    }
    if (!done_g) {
      for (int t0 = cls; t0 < j1;) {
        int hit = 0x7fffffff;
        for (int t = t0; t < j1 && hit == 0x7fffffff; t += 8 * G) {
#pragma unroll
          for (int q = 7; q >= 0; --q) { const int tq = t + q * G; if (tq < j1 && s_hg[tq] == g) hit = tq; }
        }
        if (hit == 0x7fffffff) break;
        const uint8_t *rj = arena + d.rm + (long long)view_row(d, rowidx, c0 + hit) * d.pitchC + d.col0;
        bool bad = false;
        for (int c = 0; c < n && !bad; ++c) bad = ri[c] != rj[c];
        if (!bad) { atomicMin(&s_rg[ri_], c0 + hit); break; }
        t0 = hit + G;
      }
    }
  }
  BARRIER();
  if (live && cls == 0) {
    rep_u_all[d.row_off + i] = s_ru[ri_] == 0x7fffffff ? i : s_ru[ri_];
    rep_g_all[d.row_off + i] = s_rg[ri_] == 0x7fffffff ? i : s_rg[ri_];
  }
}

// exact search from scratch (after a refuted nominee, or for views with more rows than the LDS table holds): smallest
// j <= i with identical content, hashes and lengths as filters, symbols decide
#define DD_EXACT(HU, HG, LEN, RU, RG)                                                                                   \
  P_FOR(i, S) {                                                                                                       \
    int ru = (int)i;                                                                                                    \
    const int len = LEN[i];                                                                                             \
    const uint64_t a = HU[i];                                                                                           \
    for (int j = 0; j < (int)i; ++j) {                                                                                  \
      if (HU[j] != a || LEN[j] != len) continue;                                                                        \
      bool bad = false;                                                                                                 \
      for (int p = 0; p < len && !bad; p += 16) bad = dd_diff_u16(U, upitch, (int)i, j, p, len);                        \
      if (!bad) { ru = j; break; }                                                                                      \
    }                                                                                                                   \
    int rg = (int)i;                                                                                                    \
    const uint64_t g = HG[i];                                                                                           \
    const uint8_t *ri = arena + d.rm + (long long)view_row(d, rowidx, i) * d.pitchC + d.col0;                           \
    for (int j = 0; j < (int)i; ++j) {                                                                                  \
      if (HG[j] != g) continue;                                                                                         \
      const uint8_t *rj = arena + d.rm + (long long)view_row(d, rowidx, j) * d.pitchC + d.col0;                         \
      bool bad = false;                                                                                                 \
      for (int c = 0; c < n && !bad; ++c) bad = ri[c] != rj[c];                                                         \
      if (!bad) { rg = j; break; }                                                                                      \
    }                                                                                                                   \
    RU[i] = ru; RG[i] = rg;                                                                                             \
  }

// LDS of one view's dedupe: ROWS rows, SLOTS = 2 x ROWS table slots
template <int ROWS, int SLOTS> struct DdLds {
  unsigned long long t_key[SLOTS];
  uint64_t s_hu[ROWS], s_hg[ROWS];
  int t_min[SLOTS];
  int32_t s_len[ROWS], s_ru[ROWS], s_rg[ROWS];
  long long wsum[16];
  int scan_tmp[17];
  int refuted[1];
};
// exclusive prefix sum over the threads that run the view: the workgroup, or (WV) one wavefront
template <bool WV> MPRG_DEV int dd_scan_excl(int v, int *scratch, int *total) {
  if (!WV) return block_scan_excl(v, scratch, total);
  const int incl = wave_scan_incl(v);
  *total = __shfl(incl, WAVE - 1);
  return incl - v;
}
// view q of the launch's table (q also places its k-mer occurrence offsets and its summary).  WV: run by ONE wavefront (DW_ROWS rows
// at most): loops stride the 64 lanes, WAVE_SYNC where the workgroup form has a barrier
// LOADED: the caller has put the rows' hashes and lengths into L.s_hu / s_hg / s_len (and passed a barrier)
template <bool WV, int ROWS, int SLOTS, bool LOADED = false>
MPRG_DEV void dd_view(const int q, const ViewD &d, const uint8_t *arena, const int32_t *rowidx, int kmer_size,
                      uint8_t *ucodes_all, const uint8_t *gcodes_all, uint64_t *hashes, int32_t *ulen_all, int32_t *rep_u_all, int32_t *rep_g_all,
                      int32_t *d_of_row_all, int32_t *s_of_row_all, int32_t *reps_pos_all, int32_t *reps_len_all,
                      int32_t *seqrow_all, int64_t *occ_off_all, int64_t *summary, DdLds<ROWS, SLOTS> &L) {
#define P_FOR(i_, n_) for (long long i_ = WV ? wave_lane() : MPRG_TID; i_ < (long long)(n_); i_ += WV ? WAVE : (int)blockDim.x)
#define P_BAR() do { if (WV) WAVE_SYNC(); else BARRIER(); } while (0)
#define P_ONE if ((WV ? wave_lane() : MPRG_TID) == 0)
  const int n = d.n_cols, S = d.n_rows;
  const int upitch = u_pitch(n);
  const uint8_t *U = ucodes_all + d.aux0;
  const uint64_t *hu = hashes + 2 * d.row_off, *hg = hu + S;
  int32_t *ulen = ulen_all + d.row_off, *rep_u = rep_u_all + d.row_off, *rep_g = rep_g_all + d.row_off;
  int32_t *dor = d_of_row_all + d.row_off, *sor = s_of_row_all + d.row_off;
  int32_t *rpos = reps_pos_all + d.row_off, *rlen = reps_len_all + d.row_off, *seqrow = seqrow_all + d.row_off;
  int64_t *occ = occ_off_all + d.row_off + q;
  unsigned long long *t_key = L.t_key;
  int *t_min = L.t_min;
  uint64_t *s_hu = L.s_hu, *s_hg = L.s_hg;
  int32_t *s_len = L.s_len, *s_ru = L.s_ru, *s_rg = L.s_rg;
  int *scan_tmp = L.scan_tmp, *refuted = L.refuted;
  const bool in_lds = S <= ROWS;
  int32_t *RU = in_lds ? s_ru : rep_u, *RG = in_lds ? s_rg : rep_g;
  // (the rows' ungapped hashes come from k_ungap_hash_u)
  if (in_lds) {
    if (!LOADED) P_FOR(i, S) { s_hu[i] = hu[i]; s_hg[i] = hg[i]; s_len[i] = ulen[i]; }
    P_ONE { refuted[0] = 0; }
    // ---- nominees: smallest row with the same (hash, length), ungapped then gapped content, through the LDS table
    unsigned slots = 64;                  // power of two >= 2 S: a small view does not pay for clearing the whole table
    while ((int)slots < 2 * S) slots <<= 1;
    for (int pass = 0; pass < 2; ++pass) {
      P_FOR(s, slots) { t_key[s] = DD_EMPTY; t_min[s] = 0x7fffffff; }
      P_BAR();
      P_FOR(i, S) {
        unsigned long long key = pass == 0 ? hash_mix(s_hu[i] + (uint64_t)s_len[i]) : s_hg[i];
        if (key == DD_EMPTY) key = 0;
        unsigned s = (unsigned)(key >> 7) & (slots - 1);
        for (;;) {
          const unsigned long long old = atomicCAS(&t_key[s], (unsigned long long)DD_EMPTY, key);
          if (old == DD_EMPTY || old == key) { atomicMin(&t_min[s], (int)i); break; }
          s = (s + 1) & (slots - 1);
        }
      }
      P_BAR();
      P_FOR(i, S) {
        unsigned long long key = pass == 0 ? hash_mix(s_hu[i] + (uint64_t)s_len[i]) : s_hg[i];
        if (key == DD_EMPTY) key = 0;
        unsigned s = (unsigned)(key >> 7) & (slots - 1);
        while (t_key[s] != key) s = (s + 1) & (slots - 1);
        (pass == 0 ? s_ru : s_rg)[i] = t_min[s];
      }
      P_BAR();
    }
    // ---- every nominated pair, symbol by symbol: ungapped rows 16 bytes per lane (items = row x block, blocks fastest:
    //      a wave reads consecutive 16-byte pieces of a row), gapped rows 4 bytes per lane over the row-major copy
    {
      const int nblk = upitch / 16;
      P_FOR(e, (long long)S * nblk) {
        const int i = (int)((unsigned)e / (unsigned)nblk), p0 = (int)((unsigned)e % (unsigned)nblk) * 16;
        const int j = s_ru[i], len = s_len[i];
        // a nominee that is also the row's GAPPED nominee is settled by the gapped comparison below (equal with gaps => equal
        // without): most repeated rows of a pan-genome alignment are repeats gaps included
        if (j != i && j != s_rg[i] && p0 < len && (s_len[j] != len || dd_diff_u16(U, upitch, i, j, p0, len))) refuted[0] = 1;
      }
      if (gcodes_all) {                                // gapped rows from their dense copy, 16 bytes per lane like the ungapped ones
        const uint8_t *Gc = gcodes_all + d.aux0;
        P_FOR(e, (long long)S * nblk) {
          const int i = (int)((unsigned)e / (unsigned)nblk), p0 = (int)((unsigned)e % (unsigned)nblk) * 16;
          const int j = s_rg[i];
          if (j != i && p0 < n && dd_diff_u16(Gc, upitch, i, j, p0, n)) refuted[0] = 1;
        }
      }
      const int nw = (n + 3) >> 2;                     // gapped rows: 4 cells per lane (unaligned word loads; the arena is padded)
      P_FOR(e, gcodes_all ? 0 : (long long)S * nw) {
        const int i = (int)((unsigned)e / (unsigned)nw), c = ((int)((unsigned)e % (unsigned)nw)) << 2;
        const int j = s_rg[i];
        if (j == i) continue;
        uint32_t x, y;
        __builtin_memcpy(&x, arena + d.rm + (long long)view_row(d, rowidx, i) * d.pitchC + d.col0 + c, 4);
        __builtin_memcpy(&y, arena + d.rm + (long long)view_row(d, rowidx, j) * d.pitchC + d.col0 + c, 4);
        const uint32_t keep = c + 4 > n ? 0xffffffffu >> (8 * (c + 4 - n)) : 0xffffffffu;
        if ((x ^ y) & keep) refuted[0] = 1;
      }
    }
    P_BAR();
    if (refuted[0]) {                    // a 64-bit hash collision: exact search for every row of this view
      DD_EXACT(s_hu, s_hg, s_len, s_ru, s_rg)
      P_BAR();
    }
  }
  // (more rows than the LDS table holds: rep_u / rep_g come from k_dedupe_scan_big, the launch before this one)
  // ---- first-appearance lists (cluster_sequences.py:220-233: the insertion-ordered dictionaries) by prefix sums: all
  //      distinct rows (leaf alleles), the long ones (>= k-mer size; they are clustered) with the offsets of their k-mer
  //      occurrences, the short ones (each becomes a cluster of its own)
  int base_u = 0, base_d = 0, base_s = 0, base_g = 0, base_t = 0;
  long long sumlen = 0;                  // (per-thread partial; reduced below)
  for (int c0 = 0; c0 < S; c0 += WV ? WAVE : N_THREADS) {           // uniform trip count
    const int i = c0 + (WV ? wave_lane() : (int)threadIdx.x);
    const bool live = i < S;
    const int len = live ? (in_lds ? s_len[i] : ulen[i]) : 0;
    const bool is_u = live && RU[i] == i, is_g = live && RG[i] == i;
    const bool is_long = is_u && len >= kmer_size, is_short = is_u && !is_long;
    // three of the counters share one scan (10 bits each: a chunk is at most 1024 rows); short = distinct - long
    int tot_p, tot_t;
    const int ip = dd_scan_excl<WV>((is_u ? 1 : 0) | (is_long ? 1 << 10 : 0) | (is_g ? 1 << 20 : 0), scan_tmp, &tot_p);
    const int iu = ip & 1023, id = (ip >> 10) & 1023, is = iu - id;
    const int tot_u = tot_p & 1023, tot_d = (tot_p >> 10) & 1023, tot_s = tot_u - tot_d, tot_g = (tot_p >> 20) & 1023;
    const int it = dd_scan_excl<WV>(is_long ? len - kmer_size + 1 : 0, scan_tmp, &tot_t);
    if (is_u) { rpos[base_u + iu] = i; rlen[base_u + iu] = len; sumlen += len; }
    if (is_long) { dor[i] = base_d + id; sor[i] = -1; seqrow[base_d + id] = i; occ[base_d + id + 1] = (long long)base_t + it + (len - kmer_size + 1); }
    if (is_short) { dor[i] = -1; sor[i] = base_s + is; }
    if (live && in_lds) { rep_u[i] = s_ru[i]; rep_g[i] = s_rg[i]; }
    base_u += tot_u; base_d += tot_d; base_s += tot_s; base_g += tot_g; base_t += tot_t;
  }
  // total ungapped length of the distinct rows: per-thread partials -> one value
  {
    long long v = wave_scan_incl_ll(sumlen);
    long long *wsum = L.wsum;
    if (wave_lane() == WAVE - 1) wsum[WV ? 0 : wave_id()] = v;
    P_BAR();
    P_ONE {
      long long tot = 0;
      for (int w = 0; w < (WV ? 1 : N_THREADS / WAVE); ++w) tot += wsum[w];
      occ[0] = 0;
      int64_t *sm = summary + 8 * (long long)q;
      sm[0] = base_u; sm[1] = base_g; sm[2] = base_d; sm[3] = base_t; sm[4] = tot; sm[5] = base_s; sm[6] = 0; sm[7] = 0;
    }
  }
  P_BAR();
  __threadfence_block();
  if (WV) WAVE_SYNC_GLOBAL();
  P_FOR(i, S) {                         // rows that repeat an earlier row take its indices
    const int r = RU[i];
    if (r != (int)i) { dor[i] = dor[r]; sor[i] = sor[r]; }
  }
#undef P_FOR
#undef P_BAR
#undef P_ONE
}
KERNEL(k_ungap_dedupe, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, int kmer_size,
       uint8_t *ucodes_all, const uint8_t *gcodes_all, uint64_t *hashes, int32_t *ulen_all, int32_t *rep_u_all, int32_t *rep_g_all,
       int32_t *d_of_row_all, int32_t *s_of_row_all, int32_t *reps_pos_all, int32_t *reps_len_all,
       int32_t *seqrow_all, int64_t *occ_off_all, int64_t *summary, int form, DsCount dc) {
  DS_GUARD(dc, 1);
  const ViewD d = load_view(views, BLOCK_ID);
  if (rows_elsewhere(form, d.n_rows, d.n_cols)) return;          // k_dedupe_wave's, k_rows_narrow's, k_rows_mid's
  __shared__ DdLds<DD_ROWS, DD_SLOTS> L;
  dd_view<false, DD_ROWS, DD_SLOTS>(BLOCK_ID, d, arena, rowidx, kmer_size, ucodes_all, gcodes_all, hashes, ulen_all, rep_u_all, rep_g_all, d_of_row_all,
                                    s_of_row_all, reps_pos_all, reps_len_all, seqrow_all, occ_off_all, summary, L);
}
// K3n  a NARROW selected view (rv_is_narrow) — ungap + dense gapped copy + both hashes + row groups + first-appearance lists — by ONE
//      workgroup.  Row phase: a LANE per row walks the row's words in column order (word c = columns c .. c + 3 of the view, cells past
//      n count as gaps: the words k_ungap_hash forms), RV_BATCH words per trip: the gapped hash is the sum of hash_word(w, c); the kept
//      bytes of a word (all four: the common case; else squeezed together with selects) are appended to a 64-bit accumulator, and
//      whenever 8 bytes are complete — and once at the end, for the tail, whose upper bytes are zero — they go to the ungapped row as ONE
//      store and hash_word(8 bytes, their position) is added to the ungapped hash: the sum k_ungap_hash_u forms over the compacted
//      row (both hashes are commutative sums, so hashes / ulen / the ungapped rows / the gapped copy are what the three launches write).
//      The row is streamed, not held: nothing here depends on n <= RV_COLS.  Hashes and lengths go straight into the LDS arrays of the
//      dedupe (and to `hashes` / `ulen`, which the ABI documents); dd_view runs from the nominee table on.
//      Cells: unaligned 4-byte loads from the row-major copy (a wavefront's load touches 64 rows; the words k_ungap_hash loads).
//      The views of at most RV_ROWS_S rows go to k_rows_narrow_s, the same body over a quarter of the LDS: these workgroups wait for
//      memory between their barriers, and the LDS of the 512-row form holds six of them on a CU.
#define RV_BATCH 8
template <bool WV>                     // WV: the view is ONE wavefront's (k_dedupe_wave), else the workgroup's
MPRG_DEV void rv_rows(const uint8_t *arena, const ViewD &d, const int32_t *rowidx, uint8_t *ucodes_all, uint64_t *hashes,
                      int32_t *ulen_all, uint8_t *gcodes_all, uint64_t *s_hu, uint64_t *s_hg, int32_t *s_len) {
  const int n = d.n_cols, S = d.n_rows, upitch = u_pitch(n);
  uint64_t *hu = hashes + 2 * d.row_off, *hg = hu + S;
  int32_t *ulen = ulen_all + d.row_off;
  for (long long i = WV ? wave_lane() : MPRG_TID; i < S; i += WV ? WAVE : (int)blockDim.x) {
    const uint8_t *src = arena + d.rm + (long long)view_row(d, rowidx, i) * d.pitchC + d.col0;
    uint8_t *dst = ucodes_all + d.aux0 + i * upitch;
    uint8_t *gdst = gcodes_all ? gcodes_all + d.aux0 + i * upitch : nullptr;
    uint64_t g = 0, a = 0, acc = 0;      // gapped hash, ungapped hash, kept bytes not yet stored (`fill` of them, the rest zero)
    int fill = 0, p = 0;                 // p: ungapped bytes stored so far (a multiple of 8)
    for (int cb = 0; cb < n; cb += 4 * RV_BATCH) {     // (n is the view's: uniform over the workgroup)
      uint32_t wq[RV_BATCH];
#pragma unroll
      for (int q = 0; q < RV_BATCH; ++q) {
        const int c = cb + 4 * q;
        wq[q] = 0x04040404u;
        if (c < n) __builtin_memcpy(&wq[q], src + c, 4);                // the arena is padded: the bytes past n exist
      }
#pragma unroll
      for (int q = 0; q < RV_BATCH; ++q) {
        const int c = cb + 4 * q;
        if (c >= n) break;
        uint32_t w = wq[q];
        if (c + 4 > n) {                               // the row's last word: cells past n count as gaps
          const uint32_t keep = 0xffffffffu >> (8 * (c + 4 - n));
          w = (w & keep) | (0x04040404u & ~keep);
        }
        g += hash_word(w, (unsigned)c);
        if (gdst) __builtin_memcpy(gdst + c, &w, 4);   // (upitch >= n rounded up to 16)
        const uint32_t v = w ^ 0x04040404u;            // zero bytes = gaps
        const uint32_t gap = ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;   // 0x80 in every gap byte, exactly
        uint32_t kw = w;                               // the word's kept bytes, squeezed to its low end; the rest zero
        int k = 4;
        if (gap) {
          kw = 0; k = 0;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const bool keep = !((gap >> (8 * u + 7)) & 1u);
            kw |= keep ? ((w >> (8 * u)) & 0xffu) << (8 * k) : 0u;
            k += keep ? 1 : 0;
          }
        }
        acc |= (uint64_t)kw << (8 * fill);             // (fill <= 7; what does not fit is taken up again below)
        fill += k;
        if (fill >= 8) {
          __builtin_memcpy(dst + p, &acc, 8);
          a += hash_word(acc, (unsigned)p);
          p += 8; fill -= 8;
          acc = (uint64_t)kw >> (8 * (k - fill));      // the last `fill` kept bytes of the word
        }
      }
    }
    if (fill > 0) {                                    // the tail, upper bytes zero (p + 8 <= upitch: a multiple of 16 >= n)
      __builtin_memcpy(dst + p, &acc, 8);
      a += hash_word(acc, (unsigned)p);
    }
    const int len = p + fill;
    hu[i] = a; hg[i] = g; ulen[i] = len;
    s_hu[i] = a; s_hg[i] = g; s_len[i] = len;
  }
}
#define RV_PARAMS const uint8_t *arena, const int64_t *views, const int32_t *rowidx, int kmer_size,                              \
       uint8_t *ucodes_all, uint8_t *gcodes_all, uint64_t *hashes, int32_t *ulen_all, int32_t *rep_u_all, int32_t *rep_g_all, \
       int32_t *d_of_row_all, int32_t *s_of_row_all, int32_t *reps_pos_all, int32_t *reps_len_all,                            \
       int32_t *seqrow_all, int64_t *occ_off_all, int64_t *summary, int form, DsCount dc
#define RV_BODY(ROWS_, SLOTS_, mine_) do {                                                                                            \
    DS_GUARD(dc, 1);                                                                                                                  \
    const ViewD d = load_view(views, BLOCK_ID);                                                                                       \
    if (!rv_takes(form, d.n_rows, d.n_cols) || !(mine_)) return;                                                                      \
    __shared__ DdLds<ROWS_, SLOTS_> L;                                                                                                \
    rv_rows<false>(arena, d, rowidx, ucodes_all, hashes, ulen_all, gcodes_all, L.s_hu, L.s_hg, L.s_len);                              \
    __threadfence_block();             /* the rows' stores before the other threads' loads of them (the comparisons of dd_view) */    \
    BARRIER();                                                                                                                        \
    dd_view<false, ROWS_, SLOTS_, true>(BLOCK_ID, d, arena, rowidx, kmer_size, ucodes_all, gcodes_all, hashes, ulen_all, rep_u_all,   \
                                        rep_g_all, d_of_row_all, s_of_row_all, reps_pos_all, reps_len_all, seqrow_all, occ_off_all,   \
                                        summary, L);                                                                                  \
  } while (0)
KERNEL(k_rows_narrow, RV_PARAMS) { RV_BODY(DD_ROWS, DD_SLOTS, d.n_rows > RV_ROWS_S); }
KERNEL(k_rows_narrow_s, RV_PARAMS) { RV_BODY(RV_ROWS_S, RV_SLOTS_S, d.n_rows <= RV_ROWS_S); }
#undef RV_BODY
// K3m  a MID-WIDTH selected view (rm_is_mid: RV_COLS < n <= RM_COLS columns, at most RV_ROWS_S rows) — the same outputs as K3n — by ONE
//      workgroup of RM_WAVES wavefronts.  Row phase: a group of G = 8 .. 64 lanes per row, a lane takes SIXTEEN consecutive cells (one
//      unaligned 16-byte load), so a row is ONE step of its group and a wavefront holds 64 / G rows (a "batch": 1 KB) at once; the
//      loads of RM_BATCH batches are issued before the first is consumed (32 bytes per lane in flight: k_ungap_hash's wavefront waits
//      for 256 bytes per trip, and its stores keep the compiler from starting the next row's load).
//      Per lane and batch: the four words k_ungap_hash forms (columns c, c + 4, c + 8, c + 12; cells past n count as gaps) give the
//      gapped hash (sum of hash_word(w, c)) and the dense gapped copy (one aligned 16-byte store: the cells past n up to the pitch are
//      gaps); ONE prefix sum over the group, on the lane's kept count, places the lane's kept bytes in the row's staging row in LDS
//      (a word without a gap as one store, else byte by byte).  After a wavefront-scope sync a lane takes 16 bytes of the staging row:
//      bytes past the row's length zeroed, its two 8-byte words give the ungapped hash as k_ungap_hash_u forms it (sum of
//      hash_word(w8, p), p = 0, 8, ... below the length), and they go to the ungapped row as one aligned 16-byte store (only blocks
//      that begin below the length are written; nothing reads a row past its length).  Hashes and lengths go to `hashes` / `ulen` and
//      into the LDS arrays of the dedupe; dd_view runs from the nominee table on, over the quarter-size block as in k_rows_narrow_s.
//      The 16-byte loads are NOT guarded: a load begins at a column below n, so it ends at most 15 bytes behind the view's last column,
//      which is at most 15 bytes behind the alignment's row-major copy (row pitch = columns rounded up to 16) for the last row; behind
//      every row-major copy the arena holds that alignment's transposed copy (at least 16 bytes: the hosts round both to 256), and
//      include/mprg.h asks for 16 readable bytes behind a row-major copy that stands last.
#define RM_WAVES 4
#define RM_BATCH 2
#define RM_STAGE (16 * WAVE)           // bytes of a wavefront's batch: 64 / G rows of 16 G bytes
MPRG_DEV void rm_rows(const uint8_t *arena, const ViewD &d, const int32_t *rowidx, uint8_t *ucodes_all, uint64_t *hashes, int32_t *ulen_all,
                      uint8_t *gcodes_all, uint64_t *s_hu, uint64_t *s_hg, int32_t *s_len, uint8_t *stage /* this wavefront's RM_BATCH x RM_STAGE */) {
  const int n = d.n_cols, S = d.n_rows, upitch = u_pitch(n);
  uint64_t *hu = hashes + 2 * d.row_off, *hg = hu + S;
  int32_t *ulen = ulen_all + d.row_off;
  int G = WAVE;                                        // lanes per row: 16 cells per lane (n > RV_COLS: at least 8)
  while (G > 8 && 16 * (G >> 1) >= n) G >>= 1;
  const int rows_per_wave = WAVE / G, gl = wave_lane() & (G - 1), sub = wave_lane() / G, c = 16 * gl;
  const int n_waves = N_THREADS / WAVE;
  for (int ib = wave_id() * RM_BATCH * rows_per_wave; ib < S; ib += n_waves * RM_BATCH * rows_per_wave) {   // uniform per wavefront
    uint32_t w[RM_BATCH][4];
    int row[RM_BATCH];
    // every batch's row numbers (loads where the view has a row list), then every batch's cells, before the first is looked at.  The
    // loads are not predicated (a lane past the row's end reads the row's first cells, a row past the view's end the last row): behind a
    // branch the compiler waits for ALL loads in flight before it issues the next one
#pragma unroll
    for (int h = 0; h < RM_BATCH; ++h) {
      const int i = ib + h * rows_per_wave + sub;
      row[h] = i < S ? i : S - 1;
    }
    if (d.rows_off >= 0) {
#pragma unroll
      for (int h = 0; h < RM_BATCH; ++h) row[h] = rowidx[d.rows_off + row[h]];
    }
#pragma unroll
    for (int h = 0; h < RM_BATCH; ++h) __builtin_memcpy(w[h], arena + d.rm + (long long)row[h] * d.pitchC + d.col0 + (c < n ? c : 0), 16);
#pragma unroll
    for (int h = 0; h < RM_BATCH; ++h) {               // gaps: a lane past the row's end, a row past the view's
      const bool dead = ib + h * rows_per_wave + sub >= S || c >= n;
#pragma unroll
      for (int q = 0; q < 4; ++q) w[h][q] = dead ? 0x04040404u : w[h][q];
    }
    int len[RM_BATCH];
    uint64_t g[RM_BATCH];
#pragma unroll
    for (int h = 0; h < RM_BATCH; ++h) {
      const int i = ib + h * rows_per_wave + sub;
      const bool live = i < S;
      uint8_t *srow = stage + h * RM_STAGE + sub * 16 * G;
      uint32_t gap[4];
      int kept = 0;
      g[h] = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cq = c + 4 * q;
        if (cq + 4 > n) {                              // the row's last word: cells past n count as gaps
          const uint32_t keep = cq >= n ? 0u : 0xffffffffu >> (8 * (cq + 4 - n));
          w[h][q] = (w[h][q] & keep) | (0x04040404u & ~keep);
        }
        if (cq < n) g[h] += hash_word(w[h][q], (unsigned)cq);
        const uint32_t v = w[h][q] ^ 0x04040404u;      // zero bytes = gaps
        gap[q] = ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;   // 0x80 in every gap byte, exactly
        kept += 4 - __popc(gap[q]);
      }
      if (live && gcodes_all && c < n) {               // (upitch >= c + 16: rows are 16-byte aligned)
        uint4 x;
        x.x = w[h][0]; x.y = w[h][1]; x.z = w[h][2]; x.w = w[h][3];
        *(uint4 *)(gcodes_all + d.aux0 + (long long)i * upitch + c) = x;
      }
      int incl = kept;                                 // inclusive prefix sum over the row's G lanes
      for (int dd = 1; dd < G; dd <<= 1) { const int y = __shfl_up(incl, dd, G); if (gl >= dd) incl += y; }
      len[h] = __shfl(incl, G - 1, G);
      int o = incl - kept;                             // (a lane of a row past the view's keeps nothing)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 4 - __popc(gap[q]);
        if (k == 4) __builtin_memcpy(srow + o, &w[h][q], 4);
        else if (k) {
          int oo = o;
#pragma unroll
          for (int u = 0; u < 4; ++u) if (!((gap[q] >> (8 * u + 7)) & 1u)) srow[oo++] = (uint8_t)(w[h][q] >> (8 * u));
        }
        o += k;
      }
    }
    WAVE_SYNC();                                       // the staging rows are complete
#pragma unroll
    for (int h = 0; h < RM_BATCH; ++h) {
      const int i = ib + h * rows_per_wave + sub;
      const bool live = i < S;
      const uint4 x = *(const uint4 *)(stage + h * RM_STAGE + sub * 16 * G + c);
      uint64_t lo = 0, hi = 0, a = 0;
      if (c < len[h]) {
        lo = (uint64_t)x.x | (uint64_t)x.y << 32;
        if (c + 8 > len[h]) lo &= 0xffffffffffffffffULL >> (8 * (c + 8 - len[h]));
        a = hash_word(lo, (unsigned)c);
      }
      if (c + 8 < len[h]) {
        hi = (uint64_t)x.z | (uint64_t)x.w << 32;
        if (c + 16 > len[h]) hi &= 0xffffffffffffffffULL >> (8 * (c + 16 - len[h]));
        a += hash_word(hi, (unsigned)(c + 8));
      }
      if (live && c < len[h]) {                        // (c + 16 <= upitch)
        uint4 y;
        y.x = (uint32_t)lo; y.y = (uint32_t)(lo >> 32); y.z = (uint32_t)hi; y.w = (uint32_t)(hi >> 32);
        *(uint4 *)(ucodes_all + d.aux0 + (long long)i * upitch + c) = y;
      }
      uint64_t gg = g[h];
      for (int dd = G >> 1; dd >= 1; dd >>= 1) {
        a += (uint64_t)__shfl_xor((unsigned long long)a, dd, G);
        gg += (uint64_t)__shfl_xor((unsigned long long)gg, dd, G);
      }
      if (live && gl == 0) { hu[i] = a; hg[i] = gg; ulen[i] = len[h]; s_hu[i] = a; s_hg[i] = gg; s_len[i] = len[h]; }
    }
    WAVE_SYNC();                                       // ... and read, before the next batches overwrite them
  }
}
KERNEL(k_rows_mid, RV_PARAMS) {
  DS_GUARD(dc, 1);
  const ViewD d = load_view(views, BLOCK_ID);
  if (!rm_takes(form, d.n_rows, d.n_cols)) return;
  __shared__ DdLds<RV_ROWS_S, RV_SLOTS_S> L;
  __shared__ __attribute__((aligned(16))) uint8_t stage[RM_WAVES * RM_BATCH * RM_STAGE];
  rm_rows(arena, d, rowidx, ucodes_all, hashes, ulen_all, gcodes_all, L.s_hu, L.s_hg, L.s_len, stage + wave_id() * RM_BATCH * RM_STAGE);
  __threadfence_block();               // the rows' stores before the other threads' loads of them (the comparisons of dd_view)
  BARRIER();
  dd_view<false, RV_ROWS_S, RV_SLOTS_S, true>(BLOCK_ID, d, arena, rowidx, kmer_size, ucodes_all, gcodes_all, hashes, ulen_all, rep_u_all,
                                              rep_g_all, d_of_row_all, s_of_row_all, reps_pos_all, reps_len_all, seqrow_all, occ_off_all,
                                              summary, L);
}
#undef RV_PARAMS
// K3w  a SMALL selected view — ungap + hashes + row groups + first-appearance lists — by ONE wavefront, DW_WAVES views per workgroup:
//      the three stages above in a row (their results pass through global memory as they do between the launches: a
//      workgroup-scope fence orders a wavefront's stores before its lanes' loads), no workgroup barrier.
KERNEL(k_dedupe_wave, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, int n_views, int kmer_size,
       uint8_t *ucodes_all, uint8_t *gcodes_all, uint64_t *hashes, int32_t *ulen_all, int32_t *rep_u_all, int32_t *rep_g_all,
       int32_t *d_of_row_all, int32_t *s_of_row_all, int32_t *reps_pos_all, int32_t *reps_len_all,
       int32_t *seqrow_all, int64_t *occ_off_all, int64_t *summary, DsCount dc) {
  const long long q = (long long)BLOCK_ID * DW_WAVES + wave_id();
  if (q >= ds_n(dc, n_views)) return;                 // (per wavefront: nothing below waits for the workgroup)
  const ViewD d = load_view(views, (int)q);
  if (!dw_is_small(d.n_rows, d.n_cols)) return;
  __shared__ DdLds<DW_ROWS, DW_SLOTS> L_all[DW_WAVES];
  ug_hash_rows(arena, d, rowidx, 0, d.n_rows, 0, 1, ucodes_all, hashes, ulen_all, gcodes_all);
  WAVE_SYNC_GLOBAL();
  ug_hash_u_rows(d, 0, d.n_rows, 0, 1, ucodes_all, hashes, ulen_all);
  WAVE_SYNC_GLOBAL();
  dd_view<true, DW_ROWS, DW_SLOTS>((int)q, d, arena, rowidx, kmer_size, ucodes_all, gcodes_all, hashes, ulen_all, rep_u_all, rep_g_all, d_of_row_all,
                                   s_of_row_all, reps_pos_all, reps_len_all, seqrow_all, occ_off_all, summary, L_all[wave_id()]);
}
// K3w'  k_dedupe_wave with the row phase of k_rows_narrow: a lane per row of the small view (at most DW_ROWS = 64 rows: one pass), hashes
//       and lengths straight into the wavefront's LDS arrays
KERNEL(k_rows_wave, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, int n_views, int kmer_size,
       uint8_t *ucodes_all, uint8_t *gcodes_all, uint64_t *hashes, int32_t *ulen_all, int32_t *rep_u_all, int32_t *rep_g_all,
       int32_t *d_of_row_all, int32_t *s_of_row_all, int32_t *reps_pos_all, int32_t *reps_len_all,
       int32_t *seqrow_all, int64_t *occ_off_all, int64_t *summary, DsCount dc) {
  const long long q = (long long)BLOCK_ID * DW_WAVES + wave_id();
  if (q >= ds_n(dc, n_views)) return;                 // (per wavefront: nothing below waits for the workgroup)
  const ViewD d = load_view(views, (int)q);
  if (!dw_is_small(d.n_rows, d.n_cols)) return;
  __shared__ DdLds<DW_ROWS, DW_SLOTS> L_all[DW_WAVES];
  DdLds<DW_ROWS, DW_SLOTS> &L = L_all[wave_id()];
  rv_rows<true>(arena, d, rowidx, ucodes_all, hashes, ulen_all, gcodes_all, L.s_hu, L.s_hg, L.s_len);
  WAVE_SYNC_GLOBAL();                  // the rows' stores before the other lanes' loads of them, in global memory and in LDS
  WAVE_SYNC();
  dd_view<true, DW_ROWS, DW_SLOTS, true>((int)q, d, arena, rowidx, kmer_size, ucodes_all, gcodes_all, hashes, ulen_all, rep_u_all, rep_g_all, d_of_row_all,
                                         s_of_row_all, reps_pos_all, reps_len_all, seqrow_all, occ_off_all, summary, L);
}
#undef DD_EXACT
