// ---------------------------------------------------------------------------------------------------------------
// K9  cluster_further: is some cluster NOT "one-reference-like"?   one clustering problem per workgroup
//     reference from_msa/cluster_sequences.py:59-111 (get_majority_char_in_column: Counter.most_common => ties go to
//     the symbol seen first in the cluster's row order; hamming_distance; threshold 1 if width < 5 else int(0.2*width))
//
// member_label[row position] = cluster of the row (-1: row takes no part), member_key = rank of the row in the order
// in which the reference lists the cluster's gapped rows (distinct sequence index, then row).  A thread per (cluster,
// column, slice of the cluster's rows) builds per-symbol {count, smallest key}; a thread per row then counts mismatches
// to the majority string.
// ---------------------------------------------------------------------------------------------------------------
#define CF_TILE 256
#define CF_TILE_BIG 32                 // columns per work item of a problem with more than CF_ROWS rows: its workgroups walk thousands of rows
#define CF_ROWS 1024
// column tiles (= k_cluster_majority work items) of a problem of n_rows x n_cols
static_assert(CF_TILE == MPRG_CF_TILE && CF_TILE_BIG == MPRG_CF_TILE_BIG && CF_ROWS == MPRG_CF_ROWS, "include/mprg.h documents the tiles");
MPRG_DEV long long cf_col_tiles(long long n_cols, long long n_rows) {
  const long long tw = n_rows > CF_ROWS ? CF_TILE_BIG : CF_TILE;
  return (n_cols + tw - 1) / tw;
}
// row chunks (= k_cluster_hamming work items) of a problem of n_rows x n_cols: 256 rows; 16 for a WIDE and TALL problem (a group of 16
// lanes takes a row of hundreds of columns, a workgroup 16 such rows at once: 256-row chunks made the 10 000 x 20 000 alignment's check
// 40 workgroups that each walked 5 MB; a wide problem of a hundred rows stays one work item — 16-row chunks of those cost a level of
// 7 500 pan-genome alignments 0.4 ms in fixed cost per workgroup)
#ifndef CFH_WIDE
#define CFH_WIDE MPRG_CF_WIDE          // columns from which a row goes to a group of CFH_G lanes
#endif
#define CFH_G 16
#define CFH_ROWS_WIDE 16
static_assert(CFH_ROWS_WIDE == MPRG_CF_ROWS_WIDE, "include/mprg.h documents the chunks");
MPRG_DEV int cf_chunk_rows(long long n_cols, long long n_rows) { return (n_cols >= CFH_WIDE && n_rows > CF_ROWS) ? CFH_ROWS_WIDE : CF_TILE; }
MPRG_DEV long long cf_row_chunks(long long n_cols, long long n_rows) { const int ch = cf_chunk_rows(n_cols, n_rows); return (n_rows + ch - 1) / ch; }
// problems whose rows, cluster and distinct-sequence indices, k majority strings and cells fit CFO_POOL bytes of LDS take ONE workgroup
// for the whole check (k_cluster_further_one, k_kloop.inc); the kernels below skip them when `one_form` is set
#define CFO_THREADS 128
#define CFO_POOL 8192
MPRG_DEV long long cf_lds_bytes(long long S, long long n, long long k) {
  const long long cp = (n + 3) & ~3LL;
  return ((S + 3) & ~3LL) + ((2 * S + 3) & ~3LL) + k * cp + S * cp;
}
// (cls: the launch was given rep_g — the one-workgroup form then keeps a class size and a list entry per row, 4 S bytes more, and stages
//  ONLY the representatives' cells, representative j at slot j: G rows of cells, G = the view's distinct gapped rows, where the tables
//  stay sized by the S rows)
MPRG_DEV long long cf_lds_bytes_cls(long long S, long long n, long long k, long long G) {
  const long long cp = (n + 3) & ~3LL;
  return ((S + 3) & ~3LL) + ((2 * S + 3) & ~3LL) + 4 * S + k * cp + G * cp;
}
MPRG_DEV bool cf_one_fits(long long S, long long n, long long k) { return S >= 1 && S < 65536 && n >= 1 && cf_lds_bytes(S, n, k) <= CFO_POOL; }
MPRG_DEV bool cf_one_fits_cls(long long S, long long n, long long k, long long G) {
  return S >= 1 && S < 65536 && n >= 1 && G >= 1 && G <= S && cf_lds_bytes_cls(S, n, k, G) <= CFO_POOL;
}
// The tiled launches' work lists (k_forest.inc) leave a view out when the one-workgroup form takes it whatever the call: with every row
// staged and the wider tables of a call with rep_g (what fits so fits without rep_g too), for every k up to the one given.
MPRG_DEV bool cf_lists_skip(long long S, long long n, long long k, int one_form) { return one_form && cf_one_fits_cls(S, n, k, S); }
// The rule with rep_g (by_reps; MPRG_CF_REP_RULE=0: by the S rows, as without it).  A view that fits with every row staged is the
// one-workgroup form's whatever G is, one that does not fit with a single representative is the tiled kernels'; for the views in
// between (cf_one_asks_g) k_cluster_further_one — the first launch of the call — counts the representatives of rep_g, the very list
// it would stage, and leaves G in the two bytes behind the view's KM_KMAX majority strings in `scratch` (cf_g_slot), where the tiled
// launches behind it read it: one count, one function (cf_one_takes), so a view is claimed by exactly one side.
MPRG_DEV bool cf_one_asks_g(long long S, long long n, long long k) { return !cf_one_fits_cls(S, n, k, S) && cf_one_fits_cls(S, n, k, 1); }
static_assert(KM_KMAX * 1 + 2 <= 12 && (KM_KMAX & 1) == 0, "scratch is 12 bytes per column: two bytes behind the KM_KMAX strings of a one-column view");
MPRG_DEV uint16_t *cf_g_slot(int32_t *scratch_all, const ViewD &d) { return (uint16_t *)((uint8_t *)(scratch_all + d.col_off * 3) + (long long)KM_KMAX * d.n_cols); }
MPRG_DEV bool cf_one_takes(const ViewD &d, long long k, bool cls, bool by_reps, const int32_t *scratch_all) {
  if (!cls) return cf_one_fits(d.n_rows, d.n_cols, k);
  if (!by_reps || !cf_one_asks_g(d.n_rows, d.n_cols, k)) return cf_one_fits_cls(d.n_rows, d.n_cols, k, d.n_rows);
  return cf_one_fits_cls(d.n_rows, d.n_cols, k, *cf_g_slot((int32_t *)scratch_all, d));
}
// rep_g (optional, all three kernels; mprg_ungap_dedupe's table: the smallest row of the view with identical gapped content): rows of one
// gapped class share their cluster, their symbol in every column and their distance to any string, so a class is counted ONCE, by its
// representative (rep_g[i] == i) and with its size as weight; null: every row for itself
MPRG_DEV int cf_rep(const int32_t *rep_g, long long i) {
  const int r = rep_g ? rep_g[i] : (int)i;
  return (unsigned)r > (unsigned)i ? (int)i : r;       // (a representative is the smallest row of its class: never beyond the row)
}
#ifndef CF_THREADS
#define CF_THREADS 128                 // threads of a k_cluster_majority workgroup: a narrow problem offers k x columns ~ 100 items
#endif
// K9 part 1: majority string of every cluster, one (problem, column tile) per workgroup (cf_col_tiles: 256 columns; 32 for a
// problem of more than CF_ROWS rows, which k_cluster_majority_big below takes); thread = (cluster,
// column, slice of rows), the cluster's rows of the row-major copy walked in order (coalesced across the columns); per-thread
// symbol counters live in LDS ([symbol][thread]: conflict-free).
static_assert(12 * CF_THREADS >= CF_ROWS && (long long)CF_ROWS * CF_ROWS <= (1 << 20), "class sizes per row in `first`; key below 2^20, size above");
KERNEL(k_cluster_majority, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, const int64_t *prob_all,
       const int32_t *work, int k, const int32_t *d_of_row_all, const int32_t *labels_all, int32_t *assign_all,
       const double *km_info, int32_t *scratch_all, const uint8_t *gcodes_all, const int32_t *kinfo, int one_form, const int32_t *rep_g_all,
       DsCount dc) {
  DS_GUARD(dc, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  if (kinfo && kinfo[5 * (long long)wk[0] + 1] == 0) return;      // this problem sat the round out (k_kl_advance)
  const int64_t *P = prob_all + (long long)wk[0] * PF;
  const ViewD d = load_view(views, (int)P[0]);
  if (one_form && cf_one_takes(d, k, rep_g_all != nullptr, (one_form & 2) != 0, scratch_all)) return;     // k_cluster_further_one's (one_form: 1 on, 2 by representatives)
  const int n = d.n_cols, S = d.n_rows, D = (int)P[1], tile = S > CF_ROWS ? CF_TILE_BIG : CF_TILE, c0 = wk[1] * tile;
  const int32_t *dor = d_of_row_all + d.row_off;
  const int32_t *labels = labels_all ? labels_all + P[10] : nullptr;      // null: one cluster holding every member
  uint8_t *maj = (uint8_t *)(scratch_all + d.col_off * 3);     // k majority strings of n chars (k <= 10 < 12 bytes/col)
  SHARED(uint32_t, cnt, 12 * CF_THREADS);
  SHARED(int32_t, first, 12 * CF_THREADS);
  // accepted fit: its labels become the problem's assignment.  km_info (optional): the launch follows the KMeans round
  // without a host decision in between, and a fit with fewer than k distinct labels is not accepted (cluster_sequences.py:267-273)
  if (wk[1] == 0 && labels && assign_all && (!km_info || km_info[8 * (long long)wk[0] + 3] >= (double)k)) {
    PAR_FOR(q, D) { assign_all[P[10] + q] = labels[q]; }
  }
  if (S > CF_ROWS) return;                                        // k_cluster_majority_big's (the launch behind this one; 32-column tiles)
  // member rows bucketed by cluster once per workgroup (LDS): each cluster pass then touches only its own rows and can
  // keep several cell loads in flight.  Order inside a bucket is irrelevant: ties go to the smallest key.
  // rep_g: only the representatives are filed; the class sizes add up in `first` (free until the passes below), one entry per row
  const int32_t *rg = rep_g_all ? rep_g_all + d.row_off : nullptr;
  SHARED(int32_t, mrk, 2 * CF_ROWS);
  int32_t *mrow = mrk, *mkey = mrk + CF_ROWS;
  SHARED(int, coff, 16);
  SHARED(int, cfill, 16);
  PAR_FOR(q, 16) { coff[q] = 0; }
  if (rg) { PAR_FOR(i, S) { first[i] = 0; } }
  BARRIER();
  PAR_FOR(i, S) {
    const int dd = dor[i];
    if (dd < 0) continue;
    const int cl = labels ? labels[dd] : 0;
    if (cl < 0 || cl >= k) continue;
    const int r = cf_rep(rg, i);
    if (r == (int)i) ATOMIC_ADD(coff + cl + 1, 1);
    if (rg) ATOMIC_ADD(first + r, 1);
  }
  BARRIER();
  ONE_THREAD { for (int q = 1; q <= k; ++q) coff[q] += coff[q - 1]; for (int q = 0; q < k; ++q) cfill[q] = coff[q]; }
  BARRIER();
  PAR_FOR(i, S) {
    const int dd = dor[i];
    if (dd < 0) continue;
    const int cl = labels ? labels[dd] : 0;
    if (cl < 0 || cl >= k || cf_rep(rg, i) != (int)i) continue;
    const int pos = ATOMIC_ADD(cfill + cl, 1);
    mrow[pos] = gcodes_all ? (int)i : view_row(d, rowidx, i);     // dense copy: rows by their position in the view
    // the reference lists a cluster's rows by distinct sequence, then row (S <= CF_ROWS: the key is below 2^20); above it the rows the entry counts for
    mkey[pos] = (dd * S + (int)i) | ((rg ? first[i] : 1) << 20);
  }
  BARRIER();
#define CF_COUNT(x, kw) do { if ((x) < 12) { cnt[(x) * CF_THREADS + t] += (uint32_t)(kw) >> 20; const int32_t key_ = (kw) & 0xfffff; \
                                             if (key_ < first[(x) * CF_THREADS + t]) first[(x) * CF_THREADS + t] = key_; } } while (0)
  // work item = (cluster, column of the tile, slice of the cluster's rows): clustered sub-alignments are a few dozen columns
  // wide, so columns alone would leave most of the workgroup idle while it walks the clusters — and, before the first
  // KMeans round (k = 1), every row of the view — one after the other.  Slices (only when all items fit one pass) count in
  // their thread's LDS counters; the thread of slice 0 then adds them up (counts add, smallest key wins).
  const int ncols = n - c0 < tile ? n - c0 : tile;
  const int n_items = k * ncols;
  int slices = n_items <= N_THREADS ? N_THREADS / n_items : 1;
  if (slices > 8) slices = 8;
  for (int item0 = 0; item0 < n_items; item0 += N_THREADS) {      // uniform trip count (one pass whenever slices > 1)
    const int t = (int)threadIdx.x;                   // this thread's LDS counters
    const int item = item0 + (slices > 1 ? t % n_items : t), sl = slices > 1 ? t / n_items : 0;
    const bool live = item < n_items && sl < slices;
    const int cl = live ? (int)((unsigned)item / (unsigned)ncols) : 0, c = c0 + (live ? (int)((unsigned)item % (unsigned)ncols) : 0);
    if (live) {
      for (int s = 0; s < 12; ++s) { cnt[s * CF_THREADS + t] = 0; first[s * CF_THREADS + t] = 0x7fffffff; }
      // the view's dense gapped copy (k_ungap_hash) if the caller has one, else the arena
      const uint8_t *col = gcodes_all ? gcodes_all + d.aux0 + c : arena + d.rm + d.col0 + c;
      const long long cpitch = gcodes_all ? u_pitch(n) : d.pitchC;
      const int lo = coff[cl], len = coff[cl + 1] - lo, per = (len + slices - 1) / slices;
      int m = lo + sl * per;
      const int m1 = lo + ((sl + 1) * per < len ? (sl + 1) * per : len);
      for (; m + 8 <= m1; m += 8) {
        unsigned x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = col[(long long)mrow[m + q] * cpitch] & 15u;
#pragma unroll
        for (int q = 0; q < 8; ++q) CF_COUNT(x[q], mkey[m + q]);
      }
      for (; m < m1; ++m) { const unsigned x = col[(long long)mrow[m] * cpitch] & 15u; CF_COUNT(x, mkey[m]); }
    }
    if (slices > 1) BARRIER();                        // (uniform)
    if (live && sl == 0) {
      int best = 0; uint32_t best_n = 0; int32_t best_key = 0x7fffffff;
      for (int s = 0; s < 12; ++s) {
        uint32_t a = cnt[s * CF_THREADS + t]; int32_t key = first[s * CF_THREADS + t];
        for (int o = 1; o < slices; ++o) {
          a += cnt[s * CF_THREADS + t + o * n_items];
          const int32_t ko = first[s * CF_THREADS + t + o * n_items];
          if (ko < key) key = ko;
        }
        if (s == 0 || a > best_n || (a == best_n && key < best_key)) { best = s; best_n = a; best_key = key; }
      }
      maj[(long long)cl * n + c] = (uint8_t)best;
    }
  }
#undef CF_COUNT
}

// K9 part 1b: the majority strings of a BIG problem (more than CF_ROWS rows: the root of an alignment of thousands of sequences), the
// same (problem, 32-column tile) work items by workgroups of CFB_THREADS: thread = (four columns of the tile, slice of the view's rows), 128
// slices.  (Until round 5 k_cluster_majority took these tiles too: 128 threads — 4 slices that each walked a quarter of the rows with their own
// LDS counters, 1.9 ms for the 10 000 x 20 000 alignment.)  Here the slices share the tile's counters — per (cluster, column, symbol) a count and the
// smallest key (distinct sequence, row) of a row showing it, LDS atomics — so their number is not bounded by LDS per thread.  The pick is
// k_cluster_majority's: most frequent symbol, ties to the smallest key.  Problems of at most CF_ROWS rows return at once.
#define CFB_THREADS 1024
KERNEL(k_cluster_majority_big, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, const int64_t *prob_all,
       const int32_t *work, int k, const int32_t *d_of_row_all, const int32_t *labels_all, int32_t *scratch_all,
       const uint8_t *gcodes_all, const int32_t *kinfo, int one_form, const int32_t *rep_g_all, DsCount dc) {
  DS_GUARD(dc, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  if (kinfo && kinfo[5 * (long long)wk[0] + 1] == 0) return;
  const int64_t *P = prob_all + (long long)wk[0] * PF;
  const ViewD d = load_view(views, (int)P[0]);
  const int n = d.n_cols, S = d.n_rows, c0 = wk[1] * CF_TILE_BIG;
  if (S <= CF_ROWS) return;
  if ((one_form & 2) && rep_g_all && cf_one_takes(d, k, true, true, scratch_all)) return;     // (a tall view of a few columns and classes: k_cluster_further_one's by its representatives)
  const int32_t *dor = d_of_row_all + d.row_off;
  const int32_t *labels = labels_all ? labels_all + P[10] : nullptr;
  uint8_t *maj = (uint8_t *)(scratch_all + d.col_off * 3);
  __shared__ uint32_t cnt[KM_KMAX * CF_TILE_BIG * 12];
  __shared__ unsigned long long key[KM_KMAX * CF_TILE_BIG * 12];
  const int ncols = n - c0 < CF_TILE_BIG ? n - c0 : CF_TILE_BIG;
  PAR_FOR(e, k * CF_TILE_BIG * 12) { cnt[e] = 0; key[e] = ~0ULL; }
  BARRIER();
  // thread = (four columns of the tile, slice of rows): a lane's load is a word of its row — a byte per lane made the walk 6 x 10^6
  // wavefront loads of 64 bytes for the 10 000 x 20 000 alignment, the address unit's time —, 128 slices of the rows
  const int t = (int)threadIdx.x, cg = t % (CF_TILE_BIG / 4), sl = t / (CF_TILE_BIG / 4), slices = N_THREADS / (CF_TILE_BIG / 4), cb = 4 * cg;
  if (cb < ncols && sl < slices) {
    const uint8_t *col = gcodes_all ? gcodes_all + d.aux0 + c0 + cb : arena + d.rm + d.col0 + c0 + cb;      // (rows are padded: the word exists)
    const long long cpitch = gcodes_all ? u_pitch(n) : d.pitchC;
    const int per = (S + slices - 1) / slices, i0 = sl * per, i1 = (sl + 1) * per < S ? (sl + 1) * per : S;
#define CFB_ROW(w_, dd_, i_, cl_) do {                                                                                                \
      const unsigned long long key_ = ((unsigned long long)(uint32_t)(dd_) << 32) | (uint32_t)(i_);                                   \
      _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_) {                                                                              \
        const unsigned x_ = ((w_) >> (8 * u_)) & 15u;                                                                                 \
        if (cb + u_ < ncols && x_ < 12) {                                                                                             \
          const int at_ = (((cl_) * CF_TILE_BIG + cb + u_) * 12) + (int)x_;                                                           \
          atomicAdd(&cnt[at_], 1u);                                                                                                   \
          if (key_ < key[at_]) atomicMin(&key[at_], key_);                                                                            \
        } } } while (0)
    int i = i0;
    for (; i + 8 <= i1; i += 8) {                      // eight rows per round trip
      int dd8[8], lab8[8]; uint32_t w8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) dd8[q] = dor[i + q];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        lab8[q] = (labels && dd8[q] >= 0) ? labels[dd8[q]] : 0;
        __builtin_memcpy(&w8[q], col + (long long)(gcodes_all ? i + q : view_row(d, rowidx, i + q)) * cpitch, 4);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) if (dd8[q] >= 0 && lab8[q] >= 0 && lab8[q] < k) CFB_ROW(w8[q], dd8[q], i + q, lab8[q]);
    }
    for (; i < i1; ++i) {
      const int dd = dor[i];
      if (dd < 0) continue;
      const int cl = labels ? labels[dd] : 0;
      if (cl < 0 || cl >= k) continue;
      uint32_t w;
      __builtin_memcpy(&w, col + (long long)(gcodes_all ? i : view_row(d, rowidx, i)) * cpitch, 4);
      CFB_ROW(w, dd, i, cl);
    }
#undef CFB_ROW
  }
  BARRIER();
  PAR_FOR(e, k * ncols) {
    const int cl = (int)e / ncols, c = (int)e % ncols;
    const uint32_t *cn = cnt + (cl * CF_TILE_BIG + c) * 12;
    const unsigned long long *ky = key + (cl * CF_TILE_BIG + c) * 12;
    int best = 0; uint32_t best_n = 0; unsigned long long best_key = ~0ULL;
    for (int s = 0; s < 12; ++s)
      if (s == 0 || cn[s] > best_n || (cn[s] == best_n && ky[s] < best_key)) { best = s; best_n = cn[s]; best_key = ky[s]; }
    maj[(long long)cl * n + c0 + c] = (uint8_t)best;
  }
}

// K9 part 2: Hamming distance of every member row to its cluster's majority string, one (problem, row chunk: cf_chunk_rows) per
// workgroup; thread = row over the transposed copy (wide problems with a dense copy: a group of lanes per row, below).  out_further[problem] (zeroed by the entry point) is set when a
// row is farther than the one-reference-like threshold.
KERNEL(k_cluster_hamming, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, const int64_t *prob_all,
       const int32_t *work, const int32_t *d_of_row_all, const int32_t *labels_all, const int32_t *scratch_all,
       int32_t *out_further, const uint8_t *gcodes_all, const int32_t *kinfo, int one_form_k, const int32_t *rep_g_all, DsCount dc) {
  DS_GUARD(dc, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  if (kinfo && kinfo[5 * (long long)wk[0] + 1] == 0) return;
  const int64_t *P = prob_all + (long long)wk[0] * PF;
  const ViewD d = load_view(views, (int)P[0]);
  if (one_form_k && cf_one_takes(d, one_form_k & 255, rep_g_all != nullptr, (one_form_k & 256) != 0, scratch_all)) return;     // (one_form_k: the round's k when the one-workgroup form is on, + 256: by representatives)
  const int32_t *rg = rep_g_all ? rep_g_all + d.row_off : nullptr;      // a row that is not its class's representative has nothing to decide
  const int n = d.n_cols, S = d.n_rows, chunk = cf_chunk_rows(n, S), r0 = wk[1] * chunk;
  const int32_t *dor = d_of_row_all + d.row_off;
  const int32_t *labels = labels_all ? labels_all + P[10] : nullptr;
  const uint8_t *maj = (const uint8_t *)(scratch_all + d.col_off * 3);
  const int thresh = n < 5 ? 1 : (int)(0.2 * (double)n);
  if (gcodes_all && n >= CFH_WIDE && (N_THREADS % CFH_G) == 0) {
    // WIDE rows (the dense copy): a group of CFH_G lanes per row, 8 cells per lane and step — a wavefront reads 128 contiguous bytes of
    // each of its four rows instead of 64 lines, one per lane (0.69 ms for the 10 000 x 20 000 alignment's root, whose lanes each walked
    // a row of their own, 40 workgroups in all).  The kernel's ONLY output is the problem's flag, and the flag only ever goes 0 -> 1: a
    // group that finds it set has nothing left to decide and leaves (which rows set it first changes nothing).
    const int gl = (int)threadIdx.x % CFH_G, rows_per_pass = N_THREADS / CFH_G;
    for (int ib = r0; ib < r0 + chunk && ib < S; ib += rows_per_pass) {        // uniform per workgroup (a 16-row chunk: one pass of 16 groups)
      const int i = ib + (int)threadIdx.x / CFH_G;
      int stop = (gl == 0) ? *(volatile int32_t *)(out_further + wk[0]) : 0;
      stop = __shfl(stop, 0, CFH_G);
      const int dd = (i < S && i < r0 + chunk && cf_rep(rg, i) == i) ? dor[i] : -1;
      const bool active = !stop && dd >= 0;             // (uniform per group; every lane runs the loop: its votes and shuffles are wave-wide)
      const int cl = (active && labels) ? labels[dd] : 0;
      const uint8_t *m = maj + (long long)cl * n;
      const uint8_t *grow = gcodes_all + d.aux0 + (long long)(active ? i : 0) * u_pitch(n);
      int dist = 0;
      bool far = false;
      for (int c0 = 0; c0 < n; c0 += 8 * CFH_G * 4) {   // four steps per round trip, then the group's running total
        if (active && !far) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = c0 + (q * CFH_G + gl) * 8;
            if (c < n) {
              uint64_t x, y;
              __builtin_memcpy(&x, grow + c, 8);                   // (the row's pitch is a multiple of 16: in bounds)
              __builtin_memcpy(&y, m + c, 8);                      // (the majority strings are followed by scratch: in bounds)
              uint64_t v = (x ^ y) & 0x0f0f0f0f0f0f0f0fULL;
              if (c + 8 > n) v &= 0xffffffffffffffffULL >> (8 * (c + 8 - n));
              const uint64_t nz = (((v & 0x7f7f7f7f7f7f7f7fULL) + 0x7f7f7f7f7f7f7f7fULL) | v) & 0x8080808080808080ULL;
              dist += __popcll(nz);
            }
          }
        }
        int tot = dist;
#pragma unroll
        for (int dlt = CFH_G >> 1; dlt >= 1; dlt >>= 1) tot += __shfl_xor(tot, dlt, CFH_G);
        far = far || (active && tot > thresh);
        if (!__any(active && !far)) break;              // every row of this wavefront is settled
      }
      if (far && gl == 0) out_further[wk[0]] = 1;
    }
    return;
  }
  PAR_FOR(t, chunk) {
    const int i = r0 + (int)t;
    if (i >= S || cf_rep(rg, i) != i) continue;
    const int dd = dor[i];
    if (dd < 0) continue;
    const int cl = labels ? labels[dd] : 0;
    const int row = view_row(d, rowidx, i);
    const uint8_t *m = maj + (long long)cl * n;
    int dist = 0;
    if (gcodes_all) {                                        // dense copy: 8 cells of the row and of the majority string per load
      const uint8_t *grow = gcodes_all + d.aux0 + (long long)i * u_pitch(n);
      for (int c = 0; c < n && dist <= thresh; c += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, grow + c, 8);                   // (the row's pitch is a multiple of 16: in bounds)
        __builtin_memcpy(&y, m + c, 8);                      // (the majority strings are followed by scratch: in bounds)
        uint64_t v = (x ^ y) & 0x0f0f0f0f0f0f0f0fULL;        // majority symbols are codes 0..11; cells carry them in the low nibble
        if (c + 8 > n) v &= 0xffffffffffffffffULL >> (8 * (c + 8 - n));
        const uint64_t nz = (((v & 0x7f7f7f7f7f7f7f7fULL) + 0x7f7f7f7f7f7f7f7fULL) | v) & 0x8080808080808080ULL;
        dist += __popcll(nz);
      }
    } else
    for (int c = 0; c < n && dist <= thresh; c += 8) {       // 8 columns per round trip; the early exit only saves work
      unsigned x[8], y[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { const int cc = c + q < n ? c + q : n - 1; x[q] = cell_t(arena, d, row, cc); y[q] = m[cc]; }
#pragma unroll
      for (int q = 0; q < 8; ++q) dist += (c + q < n && x[q] != y[q]) ? 1 : 0;
    }
    if (dist > thresh) out_further[wk[0]] = 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// K9b  children of a MultiClusterNode: row lists of the clusters, in the reference's order
//     reference cluster_sequences.py:287-296 (extract_clusters by label; every short sequence group is a cluster of
//     its own; merge_clusters moves the cluster holding the first row to the front) and recursion_tree.py:558-572
//     (a child keeps its rows in original order).  One splitting problem per WAVEFRONT: a stable counting sort by
//     (cluster rank, row).  64 rows at a time, the lanes that hold the same rank find each other with a ballot; their
//     places are the rank's running offset + the number of such lanes below them (popcount), so no lane ever waits for
//     another.  Offsets live in LDS (SC_RANKS ranks; more than that — hundreds of one-row clusters — falls back to one lane).
// sp: {kfin (number of KMeans clusters), offset of this problem's S entries in pool_out, offset in child_sizes}
// ---------------------------------------------------------------------------------------------------------------
#define SC_RANKS 1024
#define SC_THREADS 64
MPRG_DEV int sc_rank(const int32_t *dor, const int32_t *sor, const int32_t *assign, int kfin, int c0, int i) {
  const int c = dor[i] >= 0 ? assign[dor[i]] : kfin + sor[i];
  return c == c0 ? 0 : (c < c0 ? c + 1 : c);            // the cluster holding the first row goes first
}
KERNEL(k_split_children, const int64_t *views, const int32_t *rowidx, const int64_t *prob_all, const int64_t *sp_all,
       const int32_t *d_of_row_all, const int32_t *s_of_row_all, const int32_t *assign_all, int32_t *pool_out,
       int32_t *child_sizes, DsCount dc) {
  DS_GUARD(dc, 1);
  const int64_t *P = prob_all + (long long)BLOCK_ID * PF;
  const int64_t *sp = sp_all + 3 * (long long)BLOCK_ID;
  const ViewD d = load_view(views, (int)P[0]);
  const int S = d.n_rows, kfin = (int)sp[0];
  const int32_t *dor = d_of_row_all + d.row_off, *sor = s_of_row_all + d.row_off, *assign = assign_all + P[10];
  int32_t *out = pool_out + sp[1], *sizes = child_sizes + sp[2];
  const int lane = wave_lane();
  SHARED(int, off_s, SC_RANKS);
  int nshort = 0;
  for (int i = lane; i < S; i += WAVE) nshort = sor[i] + 1 > nshort ? sor[i] + 1 : nshort;
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) { const int y = __shfl_xor(nshort, dlt); nshort = y > nshort ? y : nshort; }
  const int nc = kfin + nshort;
  const int c0 = dor[0] >= 0 ? assign[dor[0]] : kfin + sor[0];
  if (nc > SC_RANKS) {                                  // (rare) serial form
    if (lane == 0) {
      for (int c = 0; c < nc; ++c) sizes[c] = 0;
      for (int i = 0; i < S; ++i) ++sizes[sc_rank(dor, sor, assign, kfin, c0, i)];
      int run = 0;
      for (int r = 0; r < nc; ++r) { const int t = sizes[r]; sizes[r] = run; run += t; }
      for (int i = 0; i < S; ++i) out[sizes[sc_rank(dor, sor, assign, kfin, c0, i)]++] = view_row(d, rowidx, i);
      for (int r = nc - 1; r > 0; --r) sizes[r] -= sizes[r - 1];   // back to sizes (sizes[r] held the END offsets)
    }
    return;
  }
  for (int r = lane; r < nc; r += WAVE) off_s[r] = 0;
  __syncthreads();
  // two passes over the rows: count per rank, then place.  In both, a chunk's lanes are peeled off rank by rank.
  for (int pass = 0; pass < 2; ++pass) {
    for (int i0 = 0; i0 < S; i0 += WAVE) {              // uniform trip count
      const int i = i0 + lane;
      const bool live = i < S;
      const int rank = live ? sc_rank(dor, sor, assign, kfin, c0, i) : -1;
      unsigned long long todo = __ballot(live);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(rank, leader);
        const unsigned long long same = __ballot(live && rank == r0);
        const int below = __popcll(same & ((1ull << lane) - 1ull));
        const int base = off_s[r0];                     // every lane reads it before the leader updates it
        if (pass == 1 && live && rank == r0) out[base + below] = view_row(d, rowidx, i);
        __syncthreads();
        if (lane == leader) off_s[r0] = base + __popcll(same);
        __syncthreads();
        todo &= ~same;
      }
    }
    if (pass == 0) {                                    // counts -> sizes out, exclusive offsets in LDS
      int run = 0;                                      // (uniform: every lane keeps the same running total)
      for (int r0 = 0; r0 < nc; r0 += WAVE) {
        const int r = r0 + lane;
        const int cnt = r < nc ? off_s[r] : 0;
        if (r < nc) sizes[r] = cnt;
        const int incl = wave_scan_incl(cnt);
        __syncthreads();
        if (r < nc) off_s[r] = run + incl - cnt;
        run += __shfl(incl, WAVE - 1);
      }
      __syncthreads();
    }
  }
}
