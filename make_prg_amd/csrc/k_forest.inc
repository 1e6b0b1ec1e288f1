// ---------------------------------------------------------------------------------------------------------------
// KF  the recursion forest's bookkeeping ON THE DEVICE
//     reference recursion_tree.py:401-471 (NodeFactory.build: leaf / multi-interval / multi-cluster decision, children),
//     cluster_sequences.py:235-274 (when to cluster, the k = 2..10 loop's control), recursion_tree.py:48-55 (preorder node
//     ids), :194-300 + prg_builder.py:100-119 (site numbers, where every node's text sits in the PRG string).
//
// Rounds 1-2 kept these per-NODE arrays in NumPy on the host: a level was a chain host -> device -> host, and one host
// process could keep the device busy a sixth of the time.  Here the node table, the view / problem / work-item tables of
// every launch and the k-loop's state live in HBM; every step is "count per item -> exclusive prefix sums -> fill", the
// host reads back a 512-byte header of totals per step (it needs them to size the next buffers) and nothing else.
//
// node table: MPRG_NODE_FIELDS int64 per node (include/mprg.h MPRG_N_*); a recursion level's nodes are one contiguous
// index range and the children of a node are contiguous inside the next level's range.
// F: the forest state (MPRG_F_*), a HOST array of int64 (device addresses and sizes) read when an entry point is called.
// vals: int64 [KF_VC][n] scratch of a step (column-major: column c of item j at vals[c * n + j], so that the items' writes and
// the prefix sums run over contiguous memory): per-item counts, turned into exclusive prefix sums in place.
// ---------------------------------------------------------------------------------------------------------------
#define KF_VC MPRG_FOREST_VALS_COLS      // columns of a step's count table
#define KF_HDR MPRG_FOREST_HDR          // int64 words of a step's header
enum { NF_PURE = MPRG_NF_PURE, NF_SPECIAL = MPRG_NF_SPECIAL, NF_FORCED = MPRG_NF_FORCED, NF_CAND = MPRG_NF_CAND, NF_DLEAF = MPRG_NF_DLEAF,
       NF_PQ = MPRG_NF_PQ, NF_SELF = MPRG_NF_SELF };
#define NODE(nodes, i) ((nodes) + (long long)(i) * MPRG_NODE_FIELDS)
#define KF_GID ((long long)blockIdx.x * blockDim.x + threadIdx.x)
#define KF_GRID(n) (unsigned)(((long long)(n) + 255) / 256)

// ---- exclusive prefix sums of the first m columns of vals[KF_VC][n], in place; totals[c] = column sums ---------------
// (block sums: [blocks][KF_VC])
struct KfRow {                          // item j's row of a step's count table
  int64_t *base; long long n, j;
  MPRG_DEVM int64_t &operator[](int c) const { return base[(long long)c * n + j]; }
};
#define KF_ROW(vals, n, j) KfRow{(int64_t *)(vals), (long long)(n), (long long)(j)}
MPRG_DEV long long block_scan_excl_ll(long long v, long long *scratch, long long *total) {
  const long long incl = wave_scan_incl_ll(v);
  const int nw = (int)((blockDim.x + WAVE - 1) >> 6);
  if (wave_lane() == WAVE - 1 || threadIdx.x == blockDim.x - 1) scratch[wave_id()] = incl;
  __syncthreads();
  if (threadIdx.x == 0) { long long run = 0; for (int w = 0; w < nw; ++w) { const long long t = scratch[w]; scratch[w] = run; run += t; } scratch[16] = run; }
  __syncthreads();
  const long long out = scratch[wave_id()] + incl - v;
  *total = scratch[16];
  __syncthreads();
  return out;
}
#define SCN_THREADS 256
#define SCN_PER 8                        // consecutive rows a thread sums by itself
#define SCN_ROWS (SCN_THREADS * SCN_PER)
// ---- capacity check of a step's totals, done by the kernel that writes them (mprg_forest_level: the device state `ds`) --------
// totals[c] <= cap[c] for the m columns of a step; sum checks: totals[col] + ds[field] <= cap (node table rows, row pool entries).
// A total that does not fit sets ds[MPRG_DS_OVERFLOW] = code (sticky, first one wins) BEFORE any kernel writes beyond a buffer.
struct DsCaps { long long cap[16]; };
struct KfCheck { int m; long long code; int col_a, field_a; long long cap_a; int col_b, field_b; long long cap_b; DsCaps caps; };
// (threads 0 .. 63 of one workgroup, after the totals are visible to them)
MPRG_DEV void kf_check_totals(int64_t *ds, const int64_t *totals, const KfCheck &ck) {
  const int c = (int)threadIdx.x;
  if (!ds || c >= 64) return;
  bool bad = c < ck.m && totals[c] > ck.caps.cap[c];
  if (c == 0 && ck.col_a >= 0 && totals[ck.col_a] + ds[ck.field_a] > ck.cap_a) bad = true;
  if (c == 0 && ck.col_b >= 0 && totals[ck.col_b] + ds[ck.field_b] > ck.cap_b) bad = true;
  if (bad) atomicCAS((unsigned long long *)ds + MPRG_DS_OVERFLOW, 0ull, (unsigned long long)ck.code);
}
// pass 1: column sums of every block of SCN_ROWS rows
// (n: rows the table is laid out for; with device-side counts only the first ds_n(dc, n) of them hold values)
KERNEL(k_scan_reduce, const int64_t *vals, long long n, int m, int64_t *block_sums, DsCount dc) {
  SHARED(long long, scratch, 17);
  const long long nv = ds_n(dc, n);
  const long long r0 = (long long)BLOCK_ID * SCN_ROWS + (long long)threadIdx.x * SCN_PER;
  for (int c = 0; c < m; ++c) {
    long long s = 0;
    for (int q = 0; q < SCN_PER; ++q) if (r0 + q < nv) s += vals[(long long)c * n + r0 + q];
    long long tot;
    block_scan_excl_ll(s, scratch, &tot);
    ONE_THREAD { block_sums[(long long)BLOCK_ID * KF_VC + c] = tot; }
  }
}
// pass 2 (one workgroup): exclusive prefix sums of the block sums, totals (+ their capacity check: ds != nullptr)
KERNEL(k_scan_blocks, int64_t *block_sums, long long n_blocks, int m, int64_t *totals, int64_t *ds, KfCheck ck) {
  SHARED(long long, scratch, 17);
  for (int c = 0; c < m; ++c) {
    long long base = 0;
    for (long long b0 = 0; b0 < n_blocks; b0 += N_THREADS) {      // uniform trip count
      const long long b = b0 + threadIdx.x;
      const long long v = b < n_blocks ? block_sums[b * KF_VC + c] : 0;
      long long tot;
      const long long ex = block_scan_excl_ll(v, scratch, &tot);
      if (b < n_blocks) block_sums[b * KF_VC + c] = base + ex;
      base += tot;
    }
    ONE_THREAD { totals[c] = base; }
  }
  __syncthreads();
  kf_check_totals(ds, totals, ck);
}
// pass 3: prefix sums inside every block + the block's offset
KERNEL(k_scan_apply, int64_t *vals, long long n, int m, const int64_t *block_sums, DsCount dc) {
  SHARED(long long, scratch, 17);
  const long long nv = ds_n(dc, n);
  const long long r0 = (long long)BLOCK_ID * SCN_ROWS + (long long)threadIdx.x * SCN_PER;
  for (int c = 0; c < m; ++c) {
    long long v[SCN_PER], s = 0;
    for (int q = 0; q < SCN_PER; ++q) { v[q] = r0 + q < nv ? vals[(long long)c * n + r0 + q] : 0; s += v[q]; }
    long long tot;
    long long run = block_sums[(long long)BLOCK_ID * KF_VC + c] + block_scan_excl_ll(s, scratch, &tot);
    for (int q = 0; q < SCN_PER; ++q) if (r0 + q < nv) { vals[(long long)c * n + r0 + q] = run; run += v[q]; }
  }
}
// the three passes in ONE launch for a table of at most SCS_ROWS rows (most steps of most levels: selected views, clustering
// problems, splits; a forest is ~100 such scans, each three launches of ~12 us on the stream's critical path before): a thread
// sums 8 consecutive rows, the wavefronts' sums meet in LDS — one barrier for all columns
#define SCS_THREADS 1024
#define SCS_ROWS (SCS_THREADS * SCN_PER)
KERNEL(k_scan_small, int64_t *vals, long long n, int m, int64_t *totals, DsCount dc, int64_t *ds, KfCheck ck) {
  SHARED(long long, wsum, KF_VC * (SCS_THREADS / WAVE));
  const long long nv = ds_n(dc, n);
  const int w = wave_id(), nw = SCS_THREADS / WAVE;
  const long long r0 = (long long)threadIdx.x * SCN_PER;
  for (int c = 0; c < m; ++c) {
    long long s = 0;
    for (int q = 0; q < SCN_PER; ++q) if (r0 + q < nv) s += vals[(long long)c * n + r0 + q];
    const long long incl = wave_scan_incl_ll(s);
    if (wave_lane() == WAVE - 1) wsum[c * nw + w] = incl;
  }
  __syncthreads();
  for (int c = 0; c < m; ++c) {
    long long v[SCN_PER], s = 0;
    for (int q = 0; q < SCN_PER; ++q) { v[q] = r0 + q < nv ? vals[(long long)c * n + r0 + q] : 0; s += v[q]; }
    long long run = wave_scan_incl_ll(s) - s;
    for (int x = 0; x < w; ++x) run += wsum[c * nw + x];
    for (int q = 0; q < SCN_PER; ++q) if (r0 + q < nv) { vals[(long long)c * n + r0 + q] = run; run += v[q]; }
  }
  if ((int)threadIdx.x < m) {
    long long t = 0;
    for (int x = 0; x < nw; ++x) t += wsum[(int)threadIdx.x * nw + x];
    totals[threadIdx.x] = t;
  }
  __syncthreads();
  kf_check_totals(ds, totals, ck);
}
static inline KfCheck kf_no_check() { KfCheck ck; ck.m = 0; ck.code = 0; ck.col_a = ck.col_b = -1; ck.field_a = ck.field_b = 0; ck.cap_a = ck.cap_b = 0; return ck; }
// ds + ck: the totals' capacity check rides in the launch that writes them
static int kf_scan(int64_t *vals, long long n, int m, int64_t *totals, int64_t *block_sums, void *stream, DsCount dc = DS_HOST,
                   int64_t *ds = nullptr, const KfCheck *ck = nullptr) {
  const KfCheck none = kf_no_check();
  if (!ck) { ck = &none; ds = nullptr; }
  if (n <= 0) {
    if (hipMemsetAsync(totals, 0, sizeof(int64_t) * m, (hipStream_t)stream) != hipSuccess) return -1;
    return 0;                            // (nothing counted: nothing to check)
  }
  if (n <= SCS_ROWS) {
    LAUNCH(k_scan_small, 1, SCS_THREADS, stream, vals, n, m, totals, dc, ds, *ck);
    return 0;
  }
  const long long nb = (n + SCN_ROWS - 1) / SCN_ROWS;
  LAUNCH(k_scan_reduce, nb, SCN_THREADS, stream, (const int64_t *)vals, n, m, block_sums, dc);
  LAUNCH(k_scan_blocks, 1, 1024, stream, block_sums, nb, m, totals, ds, *ck);
  LAUNCH(k_scan_apply, nb, SCN_THREADS, stream, vals, n, m, (const int64_t *)block_sums, dc);
  return 0;
}
// a step's header, published to HOST-VISIBLE pinned memory by the device itself: the host then only waits for the stream
// (no copy of its own: a small device-to-host copy queues behind the PRG text's 2.5 GB on the DMA engine)
KERNEL(k_hdr_publish, const int64_t *hdr, int64_t *hdr_host) {
  PAR_FOR(i, KF_HDR) { hdr_host[i] = hdr[i]; }
}
static inline long long kf_scan_blocks_needed(long long n) { return (n + SCN_ROWS - 1) / SCN_ROWS + 1; }

// ---- device state of a forest whose levels are enqueued without host waits (mprg_forest_level) ---------------------------------
// the same check as a launch of its own (totals that atomics wrote, not a scan: the LDS needs of the sizes step)
KERNEL(k_ds_check, int64_t *ds, const int64_t *totals, int m, DsCaps caps, long long code, int col_a, int field_a, long long cap_a,
       int col_b, int field_b, long long cap_b) {
  const int c = (int)threadIdx.x;
  bool bad = c < m && totals[c] > caps.cap[c];
  if (c == 0 && col_a >= 0 && totals[col_a] + ds[field_a] > cap_a) bad = true;
  if (c == 0 && col_b >= 0 && totals[col_b] + ds[field_b] > cap_b) bad = true;
  if (bad) atomicCAS((unsigned long long *)ds + MPRG_DS_OVERFLOW, 0ull, (unsigned long long)code);
}
// start of a level: the frontier fits its capacity?  the frontier block remembers the level's first node and size — and what
// the forest's state was when the level began (words 15-17: frontier size, node-table rows, row-pool entries), so that a level
// whose totals did not fit can be enqueued again with larger buffers (k_ds_rewind) while the levels before it are kept
KERNEL(k_ds_begin, int64_t *ds, int64_t *frontier_block, long long cap_n, long long code) {
  ONE_THREAD {
    if (ds[MPRG_DS_OVERFLOW]) return;              // (an earlier level did not fit: this level's snapshot would be of a dead state)
    frontier_block[15] = ds[MPRG_DS_N]; frontier_block[16] = ds[MPRG_DS_NNODES]; frontier_block[17] = ds[MPRG_DS_POOL_USED];
    if (ds[MPRG_DS_N] > cap_n) atomicCAS((unsigned long long *)ds + MPRG_DS_OVERFLOW, 0ull, (unsigned long long)code);
    frontier_block[13] = ds[MPRG_DS_F0]; frontier_block[14] = ds[MPRG_DS_OVERFLOW] ? 0 : ds[MPRG_DS_N];
  }
}
// back to the start of level `level` (whose frontier block holds the snapshot): the overflow flag is cleared, the levels before
// it stand as they are — a level writes nothing that its own second run would read differently before its last step
// (k_sp_children, which comes after the level's last capacity check)
KERNEL(k_ds_rewind, int64_t *ds, long long level, long long n_words) {
  // (the sizes blocks of the levels enqueued again collect atomics: back to the zeroes mprg_forest_state_init left)
  for (long long l = level; MPRG_DS_GLOBAL + (l + 1) * MPRG_DS_LEVEL_WORDS <= n_words; ++l)
    PAR_FOR(q, MPRG_FOREST_HDR) { ds[MPRG_DS_GLOBAL + l * MPRG_DS_LEVEL_WORDS + MPRG_STEP_SIZES * MPRG_FOREST_HDR + q] = 0; }
  ONE_THREAD {
    const int64_t *fb = ds + MPRG_DS_GLOBAL + level * MPRG_DS_LEVEL_WORDS;
    ds[MPRG_DS_F0] = fb[13]; ds[MPRG_DS_N] = fb[15]; ds[MPRG_DS_NNODES] = fb[16]; ds[MPRG_DS_POOL_USED] = fb[17];
    ds[MPRG_DS_LEVEL] = level; ds[MPRG_DS_OVERFLOW] = 0;
  }
}
KERNEL(k_ds_init, int64_t *ds, long long n_roots) {
  ONE_THREAD { ds[MPRG_DS_N] = n_roots; ds[MPRG_DS_NNODES] = n_roots; }
}
KERNEL(k_ds_add, int64_t *ds, int field, const int64_t *word) {
  ONE_THREAD { if (!ds[MPRG_DS_OVERFLOW]) ds[field] += word[0]; }
}
// end of a level: the next frontier = the children of this level's multi-interval nodes (already counted into the node table's
// size) + those of its new cluster nodes
KERNEL(k_ds_advance, int64_t *ds, const int64_t *classify_block, const int64_t *splits_block) {
  ONE_THREAD {
    if (ds[MPRG_DS_OVERFLOW]) { ds[MPRG_DS_N] = 0; }
    else {
      ds[MPRG_DS_F0] += ds[MPRG_DS_N];
      ds[MPRG_DS_N] = classify_block[0] + splits_block[2];
      ds[MPRG_DS_NNODES] += splits_block[2];
      ds[MPRG_DS_POOL_USED] += splits_block[1];
    }
    ds[MPRG_DS_LEVEL] += 1;
  }
}

// ---- S1  the frontier's views ----------------------------------------------------------------------------------------
// A frontier node that is a match interval straight from its parent's scan (NF_PURE) needs no kernel: for the same rows
// every column is one plain base, so it is a one-allele leaf (recursion_tree.py:414-420 would find one match interval).
// A frontier node that is a non-match interval whose own scan the parent's partition kernel has already run (NF_SELF, from
// MPRG_IV_SELF) needs no partition: the result is the one non-match interval (0, columns - 1).  It still gets a view — k_lv_sub, the
// row groups and everything after them read it — but no column slots, no place in the fused / other lists and no mask / gap-run work
// items: columns 1, 3-10 and 12 do not count it, 0, 2 and 11 do.  No partition kernel writes its n_iv / status / view_out words: the
// hosts hand those buffers over zeroed (k_pack_scan, k_pack_copy and k_lv_status read them for every view), k_lv_classify goes by the flag.
// columns: 0 active, 1 columns, 2 rows, 3 fused, 4 other, 5-9 mask items for row chunks of 1024/512/256/128/64, 10 gap-run
// row chunks, 11 cells, 12 cells of the other (non-fused) views
MPRG_DEV bool kf_is_fused(long long S, long long n, int L, int enabled) {
  long long pitch = (n + 3) / 4 * 4;
  if ((pitch / 4) % 2 == 0) pitch += 4;
  return enabled && S <= 512 && n <= 1024 && S * pitch <= 8192 && n / (L > 1 ? L - 1 : 1) + 4 <= 128 && S > 0 && n > 0;
}
// (device-side counts, here and below: n is the table's row capacity, ds_n(dc, n) the rows that exist; the frontier's first node,
//  the node table's size, the row pool's fill and the level come from the device state then)
KERNEL(k_fr_count, const int64_t *nodes, long long f0, long long n, int L, int fused_enabled, int64_t *vals, DsCount dc) {
  const long long j = KF_GID;
  if (j >= ds_n(dc, n)) return;
  if (dc.ds) f0 = dc.ds[MPRG_DS_F0];
  const int64_t *nd = NODE(nodes, f0 + j);
  const KfRow v = KF_ROW(vals, n, j);
  const bool active = !(nd[MPRG_N_FLAGS] & NF_PURE), part = active && !(nd[MPRG_N_FLAGS] & NF_SELF);
  const long long S = nd[MPRG_N_NROWS], nc = nd[MPRG_N_NCOLS];
  const bool fused = part && kf_is_fused(S, nc, L, fused_enabled), other = part && !fused;
  v[0] = active; v[1] = part ? nc : 0; v[2] = active ? S : 0; v[3] = fused; v[4] = other;
  const long long lead = nd[MPRG_N_COL0] % 4, ntile = (nc + lead + CM_TILE_COLS - 1) / CM_TILE_COLS;
  for (int q = 0; q < 5; ++q) { const long long rpc = 1024 >> q; v[5 + q] = other ? ntile * ((S + rpc - 1) / rpc) : 0; }
  v[10] = other ? gr_items(S, nc) : 0;
  v[11] = active ? S * nc : 0; v[12] = other ? S * nc : 0;
}
KERNEL(k_fr_fill, int64_t *nodes, long long f0, long long n, int L, int fused_enabled, const int64_t *vals, const int64_t *meta,
       int rpc_idx, int64_t *views, int64_t *view2node, int32_t *fused_list, int32_t *other_list, int32_t *mask_work,
       int32_t *gap_work, DsCount dc) {
  const long long j = KF_GID;
  if (j >= ds_n(dc, n)) return;
  if (dc.ds) f0 = dc.ds[MPRG_DS_F0];
  int64_t *nd = NODE(nodes, f0 + j);
  const KfRow v = KF_ROW(vals, n, j);
  const bool active = !(nd[MPRG_N_FLAGS] & NF_PURE);
  nd[MPRG_N_AUX] = active ? v[0] : -1;                 // the node's view in this level's table
  if (!active) return;
  const long long S = nd[MPRG_N_NROWS], nc = nd[MPRG_N_NCOLS], vi = v[0];
  const int64_t *M = meta + nd[MPRG_N_MSA] * 6;
  int64_t *o = views + vi * VF;
  o[0] = M[0]; o[1] = M[1]; o[2] = M[2]; o[3] = M[3]; o[4] = nd[MPRG_N_ROWS_OFF]; o[5] = S; o[6] = nd[MPRG_N_COL0]; o[7] = nc;
  o[8] = v[1]; o[9] = v[2]; o[10] = 0; o[11] = 0;
  view2node[vi] = f0 + j;
  if (nd[MPRG_N_FLAGS] & NF_SELF) return;
  if (kf_is_fused(S, nc, L, fused_enabled)) { fused_list[v[3]] = (int32_t)vi; return; }
  other_list[v[4]] = (int32_t)vi;
  const long long lead = nd[MPRG_N_COL0] % 4, ntile = (nc + lead + CM_TILE_COLS - 1) / CM_TILE_COLS, rpc = 1024 >> rpc_idx;
  const long long nchunk = (S + rpc - 1) / rpc;
  int32_t *w = mask_work + 3 * v[5 + rpc_idx];
  for (long long t = 0; t < ntile; ++t)
    for (long long c = 0; c < nchunk; ++c) { w[0] = (int32_t)vi; w[1] = (int32_t)(t * CM_TILE_COLS - lead); w[2] = (int32_t)(c * rpc); w += 3; }
  int32_t *g = gap_work + 2 * v[10];
  for (long long c = 0; c < gr_items(S, nc); ++c) { g[0] = (int32_t)vi; g[1] = (int32_t)c; g += 2; }
}

// ---- S2  after mprg_partition: leaf / multi-interval / clustering candidate (recursion_tree.py:401-471) -------------
// per-locus policy: a view whose partition failed drops its locus (the first such view in frontier order names the error)
KERNEL(k_lv_status, const int64_t *nodes, long long f0, long long n_views, const int64_t *view2node, const int32_t *view_out,
       int32_t *failed, int64_t *err_first, DsCount dc) {
  const long long v = KF_GID;
  if (v >= ds_n(dc, n_views)) return;
  if (dc.ds) f0 = dc.ds[MPRG_DS_F0];
  const int st = view_out[8 * v + 1];
  if (!st) return;
  const long long node = view2node[v], msa = NODE(nodes, node)[MPRG_N_MSA];
  atomicMin((unsigned long long *)err_first + msa, (unsigned long long)((node - f0) * 4 + ((st & MPRG_ST_BAD_LAUNCH) ? 3 : ((st & 2) ? 2 : 1))));
  failed[msa] = 1;
  if (dc.ds) ((int64_t *)dc.ds)[MPRG_DS_NFAILED] = 1;          // (the host fetches the per-locus flags only then)
}
// columns: 0 children of multi-interval nodes, 1 selected (candidate or leaf with several distinct rows), 2 rows, 3 bytes of
// ungapped rows, 4 columns, 5 row chunks of the dedupe launch, 6 cells
KERNEL(k_lv_classify, int64_t *nodes, long long f0, long long n, int lvl, const int32_t *view_out, const int32_t *failed,
       int64_t *vals, DsCount dc) {
  const long long j = KF_GID;
  if (j >= ds_n(dc, n)) return;
  if (dc.ds) { f0 = dc.ds[MPRG_DS_F0]; lvl = (int)dc.ds[MPRG_DS_LEVEL]; }
  int64_t *nd = NODE(nodes, f0 + j);
  const KfRow v = KF_ROW(vals, n, j);
  long long n_iv = 1; int first_type = 0, has_star = 0, special = 0;
  const long long vi = nd[MPRG_N_AUX];
  if (nd[MPRG_N_FLAGS] & NF_SELF) { n_iv = 1; first_type = 1; has_star = 1; special = 0; }      // (no partition kernel ran: k_fr_count)
  else if (vi >= 0) {
    const int32_t *o = view_out + 8 * vi;
    // a leaf's rows are its alleles unless every column is one plain base in ALL of them: a column of one base and N is a match
    // column (N never counts towards the consensus), yet the rows with N are left out (or no row is left: the host's expansion raises)
    n_iv = o[0]; first_type = o[2]; has_star = (o[3] & 5) != 0; special = (o[3] & 2) != 0;
  }
  const bool alive = !failed[nd[MPRG_N_MSA]];
  const bool is_leaf = alive && n_iv == 1 && first_type == 0;
  const bool is_interval = alive && !is_leaf && (n_iv > 1 || (nd[MPRG_N_FLAGS] & NF_FORCED));
  const bool is_cand = alive && !is_leaf && !is_interval, dleaf = is_leaf && has_star, sel = is_cand || dleaf;
  const long long S = nd[MPRG_N_NROWS], nc = nd[MPRG_N_NCOLS];
  nd[MPRG_N_KIND] = is_interval ? MPRG_KIND_INTERVAL : MPRG_KIND_LEAF;
  nd[MPRG_N_FIRST_CHILD] = -1; nd[MPRG_N_NCHILD] = 0; nd[MPRG_N_LVL] = lvl; nd[MPRG_N_REPS_OFF] = -1; nd[MPRG_N_NSEQ] = 1;
  nd[MPRG_N_ACHARS] = nc;
  nd[MPRG_N_FLAGS] = (nd[MPRG_N_FLAGS] & (NF_PURE | NF_FORCED | NF_SELF)) | (special ? NF_SPECIAL : 0) | (is_cand ? NF_CAND : 0) | (dleaf ? NF_DLEAF : 0);
  v[0] = is_interval ? n_iv : 0; v[1] = sel; v[2] = sel ? S : 0; v[3] = sel ? S * u_pitch((int)nc) : 0; v[4] = sel ? nc : 0;
  v[5] = sel ? ug_chunks(S, nc) : 0; v[6] = sel ? S * nc : 0;
}
// children of multi-interval nodes: one child per interval, same rows (recursion_tree.py:439-451); a wavefront per node
// (iv_self = 0: the MPRG_IV_SELF hints are ignored, every non-match child is partitioned)
KERNEL(k_lv_children, int64_t *nodes, long long f0, long long n, long long child_base, const int64_t *vals,
       const int32_t *view_out, const int32_t *iv_packed, int iv_self, DsCount dc) {
  const long long j = (long long)BLOCK_ID * (N_THREADS / WAVE) + wave_id();
  if (j >= ds_n(dc, n)) return;
  if (dc.ds) { f0 = dc.ds[MPRG_DS_F0]; child_base = dc.ds[MPRG_DS_NNODES]; }
  int64_t *nd = NODE(nodes, f0 + j);
  if (nd[MPRG_N_KIND] != MPRG_KIND_INTERVAL) return;
  const int32_t *o = view_out + 8 * nd[MPRG_N_AUX];
  const long long cnt = o[0], first = child_base + vals[j];
  if (wave_lane() == 0) { nd[MPRG_N_FIRST_CHILD] = first; nd[MPRG_N_NCHILD] = cnt; }
  const int32_t *tr = iv_packed + 3 * (long long)o[4];
  for (long long e = wave_lane(); e < cnt; e += WAVE) {
    int64_t *c = NODE(nodes, first + e);
    c[MPRG_N_MSA] = nd[MPRG_N_MSA]; c[MPRG_N_PARENT] = f0 + j; c[MPRG_N_LEVEL] = nd[MPRG_N_LEVEL];
    c[MPRG_N_ROWS_OFF] = nd[MPRG_N_ROWS_OFF]; c[MPRG_N_NROWS] = nd[MPRG_N_NROWS];
    c[MPRG_N_COL0] = nd[MPRG_N_COL0] + tr[3 * e]; c[MPRG_N_NCOLS] = tr[3 * e + 1] - tr[3 * e] + 1;
    c[MPRG_N_FLAGS] = (tr[3 * e + 2] & MPRG_IV_PURE) ? NF_PURE : (((tr[3 * e + 2] & MPRG_IV_SELF) && iv_self) ? NF_SELF : 0);
    c[MPRG_N_KIND] = MPRG_KIND_LEAF; c[MPRG_N_FIRST_CHILD] = -1; c[MPRG_N_NCHILD] = 0; c[MPRG_N_LVL] = -1; c[MPRG_N_REPS_OFF] = -1;
    c[MPRG_N_NSEQ] = 1; c[MPRG_N_ACHARS] = c[MPRG_N_NCOLS]; c[MPRG_N_AUX] = -1;
  }
}
// the selected views' own table (row / column / ungapped-byte offsets of their own) + the dedupe launch's row chunks
KERNEL(k_lv_sub, const int64_t *nodes, long long f0, long long n, const int64_t *vals, const int64_t *views, int64_t *sub,
       int64_t *selnode, int32_t *dd_work, DsCount dc) {
  const long long j = KF_GID;
  if (j >= ds_n(dc, n)) return;
  if (dc.ds) f0 = dc.ds[MPRG_DS_F0];
  const int64_t *nd = NODE(nodes, f0 + j);
  if (!(nd[MPRG_N_FLAGS] & (NF_CAND | NF_DLEAF))) return;
  const KfRow v = KF_ROW(vals, n, j);
  const int64_t *src = views + nd[MPRG_N_AUX] * VF;
  const long long q = v[1];
  int64_t *o = sub + q * VF;
  for (int f = 0; f < 8; ++f) o[f] = src[f];
  o[8] = v[4]; o[9] = v[2]; o[10] = v[3]; o[11] = 0;
  selnode[q] = f0 + j;
  int32_t *w = dd_work + 2 * v[5];
  for (long long c = 0; c < ug_chunks(nd[MPRG_N_NROWS], nd[MPRG_N_NCOLS]); ++c) { w[0] = (int32_t)q; w[1] = (int32_t)c; w += 2; }
}

// ---- S3  after mprg_ungap_dedupe: which candidates go on to clustering (recursion_tree.py:538-556 / :475-494,
//      cluster_sequences.py:235-246) ------------------------------------------------------------------------------------
// columns: 0 problem of the k = 1 check, 1 its column tiles, 2 its row chunks, 3 cells of clustering candidates, 4 cells of
// the problems of the check
// (cf_one: mprg_cluster_further's one-workgroup form is on — a problem it takes at k = 1, cf_lists_skip, has no tiles and no chunks: its
//  workgroups of the tiled launches would only find that out and leave)
KERNEL(k_cl_classify, int64_t *nodes, long long nsel, const int64_t *selnode, const int64_t *sub, const int64_t *summary,
       int max_nesting, int cf_one, int64_t *vals, DsCount dc) {
  const long long q = KF_GID;
  if (q >= ds_n(dc, nsel)) return;
  int64_t *nd = NODE(nodes, selnode[q]);
  const int64_t *sm = summary + 8 * q, *sv = sub + q * VF;
  const KfRow v = KF_ROW(vals, nsel, q);
  // every selected view can end as a leaf whose alleles are its distinct rows (recursion_tree.py:272-274)
  nd[MPRG_N_REPS_OFF] = sv[9]; nd[MPRG_N_NSEQ] = sm[0]; nd[MPRG_N_ACHARS] = sm[4];
  const bool cand = (nd[MPRG_N_FLAGS] & NF_CAND) != 0;
  const bool leaf_now = nd[MPRG_N_LEVEL] + 1 >= max_nesting || sm[0] <= 2 || sm[0] < sm[1] || sm[2] <= 2;
  const bool pq = cand && !leaf_now;
  if (pq) nd[MPRG_N_FLAGS] |= NF_PQ;
  const bool tiled = pq && !cf_lists_skip(sv[5], sv[7], 1, cf_one);
  v[0] = pq; v[1] = tiled ? cf_col_tiles(sv[7], sv[5]) : 0; v[2] = tiled ? cf_row_chunks(sv[7], sv[5]) : 0;
  v[3] = cand ? sv[5] * sv[7] : 0; v[4] = pq ? sv[5] * sv[7] : 0;
}
KERNEL(k_cl_fill_pq, const int64_t *nodes, long long nsel, const int64_t *selnode, const int64_t *sub, const int64_t *summary,
       const int64_t *vals, int cf_one, int64_t *t1, int32_t *work_cols, int32_t *work_rows, DsCount dc) {
  const long long q = KF_GID;
  if (q >= ds_n(dc, nsel) || !(NODE(nodes, selnode[q])[MPRG_N_FLAGS] & NF_PQ)) return;
  const KfRow v = KF_ROW(vals, nsel, q);
  const long long i = v[0];
  const int64_t *sv = sub + q * VF;
  int64_t *o = t1 + i * PF;
  for (int f = 0; f < PF; ++f) o[f] = 0;
  o[0] = q; o[1] = summary[8 * q + 2];
  if (cf_lists_skip(sv[5], sv[7], 1, cf_one)) return;
  int32_t *w = work_cols + 2 * v[1];
  for (long long c = 0; c < cf_col_tiles(sv[7], sv[5]); ++c) { w[0] = (int32_t)i; w[1] = (int32_t)c; w += 2; }
  w = work_rows + 2 * v[2];
  for (long long c = 0; c < cf_row_chunks(sv[7], sv[5]); ++c) { w[0] = (int32_t)i; w[1] = (int32_t)c; w += 2; }
}

// ---- S4  after the k = 1 check (cluster_sequences.py:256: `while cluster_further(...)` comes before any KMeans): the
//      clustering problems and their k-mer tables -----------------------------------------------------------------------
// columns: 0 problem, 1 bytes of its k-mer table, 2 bytes of its first-appearance flags, 3 distinct long sequences
MPRG_DEV long long kf_table_cap(long long T) { long long cap = 16; while (cap < 2 * T) cap <<= 1; return cap; }
KERNEL(k_pr_count, long long n_pq, const int64_t *t1, const int32_t *further, const int64_t *summary, int64_t *vals, DsCount dc) {
  const long long i = KF_GID;
  if (i >= ds_n(dc, n_pq)) return;
  const long long q = t1[i * PF];
  const bool f = further[i] != 0;
  const long long T = summary[8 * q + 3];
  const KfRow v = KF_ROW(vals, n_pq, i);
  v[0] = f; v[1] = f ? 16 * kf_table_cap(T) : 0; v[2] = f ? (T + 15) / 16 * 16 : 0; v[3] = f ? summary[8 * q + 2] : 0;
}
KERNEL(k_pr_fill, long long n_pq, const int64_t *t1, const int32_t *further, const int64_t *summary, const int64_t *sub,
       const int64_t *vals, int64_t *ptab, DsCount dc) {
  const long long i = KF_GID;
  if (i >= ds_n(dc, n_pq) || !further[i]) return;
  const KfRow v = KF_ROW(vals, n_pq, i);
  const long long q = t1[i * PF], T = summary[8 * q + 3];
  int64_t *o = ptab + v[0] * PF;
  o[0] = q; o[1] = summary[8 * q + 2]; o[2] = sub[q * VF + 9]; o[3] = T; o[4] = v[1]; o[5] = kf_table_cap(T);
  o[6] = sub[q * VF + 9] + q; o[7] = 0; o[8] = 0; o[9] = 0; o[10] = v[3]; o[11] = v[2];
}

// ---- S5  after mprg_kmer_dictionary: matrices, workspaces, launch classes of mprg_kmeans_prepare, biggest fits first ----
// columns: 0 doubles of the count matrix, 1 doubles of the KMeans workspace, 2-6 member of prepare class 0..3 / global form,
// 7 column tiles, 8 row chunks of mprg_cluster_further
// hdr[16 + c]: largest LDS need of class c; hdr[24 + b]: problems of size bucket b (D * V, powers of 4, biggest first);
// hdr[15]: a matrix has more features than the kernels' pairwise-sum stack holds
#define KF_BUCKETS 24
MPRG_DEV int kf_prepare_class(long long need) {
  return need <= 12 * 1024 ? 0 : (need <= 24 * 1024 ? 1 : (need <= 64 * 1024 ? 2 : (need <= MPRG_KMEANS_PREPARE_LDS_MAX ? 3 : 4)));
}
MPRG_DEV int kf_size_bucket(long long dv) {     // 0 = biggest
  int lg = 0;
  while (lg < 2 * (KF_BUCKETS - 1) && (dv >> (lg + 1)) > 0) ++lg;
  return KF_BUCKETS - 1 - lg / 2;
}
// (cf_one: as in k_cl_classify, for the rounds k = 2 .. KM_KMAX: a problem the one-workgroup form takes at KM_KMAX it takes in every round)
KERNEL(k_sz_count, long long P, const int64_t *ptab, const int32_t *dV, const int64_t *sub, int n_init, int cf_one, int64_t *vals, int64_t *hdr, DsCount dc) {
  const long long p = KF_GID;
  if (p >= ds_n(dc, P)) return;
  const long long D = ptab[p * PF + 1], V = dV[p] & 0xffffff;
  if ((dV[p] >> 24) == 0x7f) hdr[14] = 1;          // no hash seed separated the k-mers (k > 16)
  const KfRow v = KF_ROW(vals, P, p);
  const long long need = 8 * (D * (V | 1) + 2 * V);
  const int cls = kf_prepare_class(need);
  v[0] = D * V; v[1] = km_common_doubles(D, V) + (long long)n_init * km_restart_doubles(D, V);
  for (int c = 0; c < 5; ++c) v[2 + c] = c == cls;
  const int64_t *sv = sub + ptab[p * PF] * VF;
  const bool tiled = !cf_lists_skip(sv[5], sv[7], KM_KMAX, cf_one);
  v[7] = tiled ? cf_col_tiles(sv[7], sv[5]) : 0; v[8] = tiled ? cf_row_chunks(sv[7], sv[5]) : 0;
  atomicMax((unsigned long long *)hdr + 16 + cls, (unsigned long long)need);
  atomicAdd((unsigned long long *)hdr + 24 + kf_size_bucket(D * V), 1ull);
  if (V > (128LL << (KM_PW_DEPTH - 1))) hdr[15] = 1;
}
// the final problem table in launch order (row b = fit b of every round), the prepare lists, the k-loop's state
KERNEL(k_sz_fill, long long P, const int64_t *ptab0, const int32_t *dV, const int64_t *sub, const int64_t *vals, int64_t *hdr, int64_t *ptab,
       int32_t *cls_lists, int32_t *num_clusters, int32_t *active, int cf_one, int32_t *work_cols, int32_t *work_rows, DsCount dc) {
  const long long p = KF_GID;
  if (p >= ds_n(dc, P)) return;
  const KfRow v = KF_ROW(vals, P, p);
  const int64_t *src = ptab0 + p * PF;
  const long long D = src[1], V = dV[p] & 0xffffff;
  const int bucket = kf_size_bucket(D * V);
  long long base = 0;
  for (int b = 0; b < bucket; ++b) base += hdr[24 + b];
  const long long row = base + (long long)atomicAdd((unsigned long long *)hdr + 24 + KF_BUCKETS + bucket, 1ull);
  int64_t *o = ptab + row * PF;
  for (int f = 0; f < PF; ++f) o[f] = src[f];
  o[7] = V; o[8] = v[0]; o[9] = v[1];
  o[5] |= (long long)(dV[p] >> 24) << 40;          // the k-mer hash seed rides in the capacity field's high bits (k_kmer_counts)
  const int cls = kf_prepare_class(8 * (D * (V | 1) + 2 * V));
  cls_lists[(long long)cls * P + v[2 + cls]] = (int32_t)row;
  num_clusters[row] = 1; active[row] = 1;
  if (!work_cols) return;                  // (the fused clustering loop needs no per-round work items)
  const int64_t *sv = sub + src[0] * VF;
  if (cf_lists_skip(sv[5], sv[7], KM_KMAX, cf_one)) return;
  int32_t *w = work_cols + 2 * v[7];
  for (long long c = 0; c < cf_col_tiles(sv[7], sv[5]); ++c) { w[0] = (int32_t)row; w[1] = (int32_t)c; w += 2; }
  w = work_rows + 2 * v[8];
  for (long long c = 0; c < cf_row_chunks(sv[7], sv[5]); ++c) { w[0] = (int32_t)row; w[1] = (int32_t)c; w += 2; }
}

// ---- S6  the reference's loop `while cluster_further: k += 1; KMeans(k)` (cluster_sequences.py:256-274) without the
//      host: before round k this kernel reads what round k-1 left (km_info, km_status, out_further), settles every
//      problem's state and writes the round's fit descriptors; a problem that is done gets k = 0 and its workgroups of the
//      round's launches return at once.
// hdr (atomics): 80 fits run, 81 / 85 / 93 KMeans bytes of the fits run in the wave / general / small workgroup form (doubles), 82 a fit needed the median-of-medians fallback, 83 problems still
// active after this call, 84 cells the rounds' mprg_cluster_further calls visit (double), 86-90 (per call) fits of the round per
// launch list: wave form by LDS class 0..3 (86-89), general workgroup form (90), small workgroup form k <= 6 / any k (91, 92)
MPRG_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
// mode: bit 0 = small fits take the wave form, bit 1 = small fits take the 128-thread workgroup form (else: the general form),
// bit 2 (round 6) = the LDS form (k_kmeans_fit_lds) takes every fit it has a class for, before the other two are asked; its four
// classes use the wave form's list slots, its last two the small form's (so with bit 2 set, bits 0 and 1 are ignored: a fit
// without an LDS class takes the general form, never slots 5 / 6, which the hosts launch as LDS classes 4 / 5)
#define KL_LISTS 7                      // launch lists: wave / LDS classes 0-3, general workgroup form, small workgroup form k <= 6 / any k
KERNEL(k_kl_advance, long long P, int k, int n_init, int mode, const int64_t *ptab, const int64_t *sub, int32_t *num_clusters,
       int32_t *active, int32_t *kinfo, const double *km_info, int32_t *km_status, const int32_t *further, int uoff,
       int32_t *fit_lists, int64_t *hdr, const double *ws_all) {
  const long long b = KF_GID;
  const bool valid = b < P;              // (no early return: the wave-level sums and ballots below need every lane)
  const long long D = valid ? ptab[b * PF + 1] : 0, V = valid ? ptab[b * PF + 7] : 0;
  int act = valid ? active[b] : 0, nc = valid ? num_clusters[b] : 0;
  const double *ws = (valid && ws_all) ? ws_all + ptab[b * PF + 9] : nullptr;          // (the LDS form asks whether K6 made the seeding's tables)
  double kb_wave = 0, kb_wg = 0, kb_small = 0, cf = 0;
  int ran = 0, bad = 0;
  if (act && k > 2) {                                   // round k - 1 ran for this problem
    const double *info = km_info + 8 * b;
    if (km_status[b] & MPRG_KM_UNSUPPORTED) bad = 1;
    ran = 1;
    const double kb = 8.0 * (double)D * (double)V * (info[4] + (double)n_init);
    if ((mode & 4) && kml_class_ws(D, V, k - 1, n_init, false, ws) >= 0) kb_wave = kb;
    else if ((mode & 1) && km_wave_class(D, V, k - 1) >= 0) kb_wave = kb;
    else if ((mode & 2) && !(mode & 4) && km_small_class(D, V, k - 1, n_init) >= 0) kb_small = kb;
    else kb_wg = kb;
    if (!(info[3] >= (double)(k - 1))) { nc -= 1; act = 0; }       // fewer than k distinct labels: revert and stop (:267-273)
    else if (!further[b]) act = 0;                                 // every cluster is one-reference-like: accepted
  }
  if (act) {
    nc += 1;
    if (nc > KM_KMAX || nc == D) act = 0;                          // :258-261
  }
  const bool runs = act && k <= KM_KMAX;
  int cls = -1;
  if (valid) {
    num_clusters[b] = nc; active[b] = act;
    int32_t *ki = kinfo + 5 * b;
    ki[0] = (int32_t)b; ki[1] = runs ? k : 0; ki[2] = 0; ki[3] = uoff; ki[4] = 0;
    km_status[b] = 0;
    if (runs) {                          // the round's launch lists
      cls = 4;
      const int wc = (mode & 4) ? kml_class_ws(D, V, k, n_init, false, ws) : ((mode & 1) ? km_wave_class(D, V, k) : -1);
      if (wc >= 0) cls = wc < 4 ? wc : wc + 1;        // (the LDS form's fifth and sixth class take the small form's list slots: the two are not combined)
      else if ((mode & 2) && !(mode & 4)) { const int sc = km_small_class(D, V, k, n_init); if (sc >= 0) cls = 5 + sc; }
      const int64_t *sv = sub + ptab[b * PF] * VF;
      cf = (double)(sv[5] * sv[7]);
    }
  }
  // one atomic per wavefront and counter (a million lanes on one address serialise: 23 ms per step before)
  const int lane = wave_lane();
  for (int c = 0; c < KL_LISTS; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (!m) continue;
    const int leader = __ffsll((long long)m) - 1;
    long long base = 0;
    if (lane == leader) base = (long long)atomicAdd((unsigned long long *)hdr + 86 + c, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    if (cls == c) fit_lists[(long long)c * P + base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)b;
  }
  const unsigned long long m_ran = __ballot(ran), m_act = __ballot(act), m_bad = __ballot(bad);
  kb_wave = wave_sum_f64(kb_wave); kb_wg = wave_sum_f64(kb_wg); kb_small = wave_sum_f64(kb_small); cf = wave_sum_f64(cf);
  if (lane == 0) {
    if (m_ran) atomicAdd((unsigned long long *)hdr + 80, (unsigned long long)__popcll(m_ran));
    if (kb_wave != 0) atomicAdd((double *)hdr + 81, kb_wave);
    if (kb_wg != 0) atomicAdd((double *)hdr + 85, kb_wg);
    if (kb_small != 0) atomicAdd((double *)hdr + 93, kb_small);
    if (m_bad) hdr[82] = 1;
    if (m_act) atomicAdd((unsigned long long *)hdr + 83, (unsigned long long)__popcll(m_act));
    if (cf != 0) atomicAdd((double *)hdr + 84, cf);
  }
}

// ---- S6s  every round of a problem's loop at once (levels that hold a few BIG problems: a round's general-form fits are a
//      wide workgroup per restart — ten workgroups per problem, a handful of CUs of 256 for nine rounds one after the other).  The
//      fits of different k share nothing but the problem's read-only data: the general-form fit of EVERY k = 2 .. min(10, D - 1)
//      goes out in one launch (restart slots (k - 2) n_init .., labels and results in round k's slice), and the loop's rounds then
//      settle, in the reference's order, on results that are already there (k_kl_advance, mprg_cluster_further: unchanged).  A fit
//      of a round the loop never reaches is wasted work on otherwise idle CUs.
// kinfo_out: int32 [9][P][5]; row (k - 2) P + b = {b, k or 0, (k - 2) n_init, offset of k's uniforms, (k - 2) labels_per_k}
struct KlUoffs { int32_t v[KM_KMAX + 1]; };
KERNEL(k_kl_speculate, long long P, int n_init, int mode, const int64_t *ptab, KlUoffs uoff, long long labels_per_k, int32_t *kinfo_out,
       const double *ws_all) {
  const long long e = KF_GID;
  if (e >= P * (KM_KMAX - 1)) return;
  const long long b = e % P;
  const int k = 2 + (int)(e / P);
  const long long D = ptab[b * PF + 1], V = ptab[b * PF + 7];
  bool general = k < D;                                 // (round k runs only while k < D: cluster_sequences.py:258-261)
  if (general && (mode & 4) && kml_class_ws(D, V, k, n_init, false, ws_all ? ws_all + ptab[b * PF + 9] : nullptr) >= 0) general = false;
  if (general && (mode & 1) && !(mode & 4) && km_wave_class(D, V, k) >= 0) general = false;
  if (general && (mode & 2) && !(mode & 4) && km_small_class(D, V, k, n_init) >= 0) general = false;
  int32_t *ki = kinfo_out + 5 * e;
  ki[0] = (int32_t)b; ki[1] = general ? k : 0; ki[2] = (k - 2) * n_init; ki[3] = uoff.v[k]; ki[4] = (int32_t)((k - 2) * labels_per_k);
}

// ---- S7  MultiClusterNodes and their children (cluster_sequences.py:276-296, recursion_tree.py:457-469) --------------
// columns: 0 split, 1 rows, 2 children
KERNEL(k_sp_count, long long P, const int64_t *ptab, const int32_t *num_clusters, const int64_t *sub, const int64_t *summary,
       int64_t *vals, DsCount dc) {
  const long long b = KF_GID;
  if (b >= ds_n(dc, P)) return;
  const long long q = ptab[b * PF], D = ptab[b * PF + 1], nc = num_clusters[b];
  const bool split = nc != 1 && nc != D;
  const KfRow v = KF_ROW(vals, P, b);
  v[0] = split; v[1] = split ? sub[q * VF + 5] : 0; v[2] = split ? (nc < KM_KMAX ? nc : KM_KMAX) + summary[8 * q + 5] : 0;
}
KERNEL(k_sp_fill, long long P, const int64_t *ptab, const int32_t *num_clusters, const int64_t *selnode, const int64_t *vals,
       long long pool_used, int64_t *spt, int64_t *sp, int64_t *splitnode, DsCount dc) {
  const long long b = KF_GID;
  if (b >= ds_n(dc, P)) return;
  if (dc.ds) pool_used = dc.ds[MPRG_DS_POOL_USED];
  const long long D = ptab[b * PF + 1], nc = num_clusters[b];
  if (!(nc != 1 && nc != D)) return;
  const KfRow v = KF_ROW(vals, P, b);
  const long long s = v[0];
  for (int f = 0; f < PF; ++f) spt[s * PF + f] = ptab[b * PF + f];
  sp[3 * s] = nc < KM_KMAX ? nc : KM_KMAX; sp[3 * s + 1] = pool_used + v[1]; sp[3 * s + 2] = v[2];
  splitnode[s] = selnode[ptab[b * PF]];
}
// a wavefront per new MultiClusterNode: the node itself sits one nesting level down (recursion_tree.py:459), its children
// take the row lists mprg_split_children wrote
KERNEL(k_sp_children, int64_t *nodes, long long n_splits, long long child_base, const int64_t *sp, const int64_t *splitnode,
       const int32_t *child_sizes, const int64_t *spt, const int64_t *summary, DsCount dc) {
  const long long s = (long long)BLOCK_ID * (N_THREADS / WAVE) + wave_id();
  if (s >= ds_n(dc, n_splits)) return;
  if (dc.ds) child_base = dc.ds[MPRG_DS_NNODES];
  int64_t *nd = NODE(nodes, splitnode[s]);
  const long long nchild = sp[3 * s] + summary[8 * spt[s * PF] + 5], pool_off = sp[3 * s + 1], child_off = sp[3 * s + 2];
  const long long level = nd[MPRG_N_LEVEL] + 1, first = child_base + child_off;
  __syncthreads();                                       // (every lane has read the node's level before lane 0 rewrites it)
  if (wave_lane() == 0) { nd[MPRG_N_KIND] = MPRG_KIND_CLUSTER; nd[MPRG_N_LEVEL] = level; nd[MPRG_N_FIRST_CHILD] = first; nd[MPRG_N_NCHILD] = nchild; }
  long long run = 0;
  for (long long e0 = 0; e0 < nchild; e0 += WAVE) {     // uniform trip count per wave
    const long long e = e0 + wave_lane();
    const long long size = e < nchild ? child_sizes[child_off + e] : 0;
    const long long incl = wave_scan_incl_ll(size);
    if (e < nchild) {
      int64_t *c = NODE(nodes, first + e);
      c[MPRG_N_MSA] = nd[MPRG_N_MSA]; c[MPRG_N_PARENT] = splitnode[s]; c[MPRG_N_LEVEL] = level;
      c[MPRG_N_ROWS_OFF] = pool_off + run + incl - size; c[MPRG_N_NROWS] = size;
      c[MPRG_N_COL0] = nd[MPRG_N_COL0]; c[MPRG_N_NCOLS] = nd[MPRG_N_NCOLS]; c[MPRG_N_FLAGS] = 0;
      c[MPRG_N_KIND] = MPRG_KIND_LEAF; c[MPRG_N_FIRST_CHILD] = -1; c[MPRG_N_NCHILD] = 0; c[MPRG_N_LVL] = -1; c[MPRG_N_REPS_OFF] = -1;
      c[MPRG_N_NSEQ] = 1; c[MPRG_N_ACHARS] = nd[MPRG_N_NCOLS]; c[MPRG_N_AUX] = -1;
    }
    run += __shfl(incl, WAVE - 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// KA  PRG assembly: preorder node ids, site numbers, where every node's text goes — over the device node table
//     reference PrgBuilder.build_prg prg_builder.py:100-105; traversals recursion_tree.py:194-201, :222-239, :266-300
// asm table: MPRG_ASM_FIELDS int64 per node {subtree size, preorder rank, site number, text length, text start, alleles,
// allele characters, first allele copy job}
// ---------------------------------------------------------------------------------------------------------------
enum { A_SIZE = MPRG_ASM_SIZE, A_PRE = MPRG_ASM_PRE, A_SITE = MPRG_ASM_SITE, A_TOTAL = MPRG_ASM_TOTAL, A_START = MPRG_ASM_START,
       A_NSEQ = MPRG_ASM_NSEQ, A_ACHARS = MPRG_ASM_ACHARS, A_JOB = MPRG_ASM_JOB };
#define ASM(a, i) ((a) + (long long)(i) * MPRG_ASM_FIELDS)
MPRG_DEV int kf_digits(long long v) { int nd = 1; for (long long t = v; t >= 10; t /= 10) ++nd; return nd; }
// leaves whose columns hold ambiguity codes or N: the host expands them (utils/seq_utils.py:116-153; rare)
KERNEL(k_as_special, const int64_t *nodes, long long n, const int32_t *failed, int64_t *list, int64_t cap, int64_t *hdr) {
  const long long i = KF_GID;
  if (i >= n) return;
  const int64_t *nd = NODE(nodes, i);
  if (nd[MPRG_N_KIND] != MPRG_KIND_LEAF || nd[MPRG_N_REPS_OFF] < 0 || !(nd[MPRG_N_FLAGS] & NF_SPECIAL) || failed[nd[MPRG_N_MSA]]) return;
  const long long at = (long long)atomicAdd((unsigned long long *)hdr, 1ull);
  if (at >= cap) return;
  list[at * (MPRG_NODE_FIELDS + 1)] = i;
  for (int f = 0; f < MPRG_NODE_FIELDS; ++f) list[at * (MPRG_NODE_FIELDS + 1) + 1 + f] = nd[f];
}
// patches: {node, alleles, allele characters} of the host-expanded leaves (alleles < 0: the expansion failed, locus dropped)
KERNEL(k_as_init, const int64_t *nodes, long long n, const int32_t *failed, int64_t *A) {
  const long long i = KF_GID;
  if (i >= n) return;
  const int64_t *nd = NODE(nodes, i);
  int64_t *a = ASM(A, i);
  const bool leaf = nd[MPRG_N_KIND] == MPRG_KIND_LEAF && !failed[nd[MPRG_N_MSA]];
  a[A_SIZE] = 1; a[A_PRE] = 0; a[A_SITE] = 0; a[A_TOTAL] = 0; a[A_START] = 0;
  a[A_NSEQ] = leaf ? nd[MPRG_N_NSEQ] : 0; a[A_ACHARS] = leaf ? nd[MPRG_N_ACHARS] : 0; a[A_JOB] = 0;
}
KERNEL(k_as_patch, long long n_patch, const int64_t *patch, int64_t *A) {
  const long long t = KF_GID;
  if (t >= n_patch) return;
  int64_t *a = ASM(A, patch[3 * t]);
  a[A_NSEQ] = patch[3 * t + 1]; a[A_ACHARS] = patch[3 * t + 2]; a[A_JOB] = -1;       // -1: the host writes this leaf's text
}
// bottom-up: field[p] += sum over p's children, one level of parents per launch
KERNEL(k_as_up, const int64_t *nodes, long long f0, long long n, int64_t *A, int field) {
  const long long j = KF_GID;
  if (j >= n) return;
  const int64_t *nd = NODE(nodes, f0 + j);
  const long long nch = nd[MPRG_N_NCHILD], fc = nd[MPRG_N_FIRST_CHILD];
  if (nch <= 0) return;
  long long s = 0;
  for (long long c = 0; c < nch; ++c) s += ASM(A, fc + c)[field];
  ASM(A, f0 + j)[field] += s;
}
// top-down: preorder rank inside each tree
KERNEL(k_as_pre, const int64_t *nodes, long long f0, long long n, int64_t *A) {
  const long long j = KF_GID;
  if (j >= n) return;
  const int64_t *nd = NODE(nodes, f0 + j);
  const long long nch = nd[MPRG_N_NCHILD], fc = nd[MPRG_N_FIRST_CHILD];
  long long run = ASM(A, f0 + j)[A_PRE] + 1;
  for (long long c = 0; c < nch; ++c) { ASM(A, fc + c)[A_PRE] = run; run += ASM(A, fc + c)[A_SIZE]; }
}
// per alignment: nodes of its tree (column 0) — the prefix sums place the trees one after the other in preorder
KERNEL(k_as_tree_sizes, long long n_msas, const int64_t *root_of, const int64_t *A, int64_t *vals) {
  const long long m = KF_GID;
  if (m >= n_msas) return;
  vals[m] = root_of[m] >= 0 ? ASM(A, root_of[m])[A_SIZE] : 0;
}
// openers (cluster nodes, leaves with several alleles) flagged at their preorder place: column 0 of vals2[n]
KERNEL(k_as_openers, const int64_t *nodes, long long n, const int32_t *failed, const int64_t *A, const int64_t *tree_base,
       int64_t *vals2, int64_t *n_sites) {
  const long long i = KF_GID;
  if (i >= n) return;
  const int64_t *nd = NODE(nodes, i);
  const long long msa = nd[MPRG_N_MSA];
  const bool valid = !failed[msa];
  const bool opener = valid && (nd[MPRG_N_KIND] == MPRG_KIND_CLUSTER || (nd[MPRG_N_KIND] == MPRG_KIND_LEAF && ASM(A, i)[A_NSEQ] > 1));
  vals2[tree_base[msa] + ASM(A, i)[A_PRE]] = opener;
  if (opener) atomicAdd((unsigned long long *)n_sites + msa, 1ull);
}
// site numbers (5, 7, 9 ... in preorder inside each tree) and the nodes' own text lengths
KERNEL(k_as_sites, const int64_t *nodes, long long n, const int32_t *failed, int64_t *A, const int64_t *tree_base,
       const int64_t *vals2) {
  const long long i = KF_GID;
  if (i >= n) return;
  const int64_t *nd = NODE(nodes, i);
  int64_t *a = ASM(A, i);
  const long long msa = nd[MPRG_N_MSA], tb = tree_base[msa];
  const bool valid = !failed[msa];
  const long long site = 5 + 2 * (vals2[tb + a[A_PRE]] - vals2[tb]);
  a[A_SITE] = site;
  const long long open_len = kf_digits(site) + 2, mid_len = kf_digits(site + 1) + 2;
  long long total = 0;
  if (valid && nd[MPRG_N_KIND] == MPRG_KIND_LEAF) {
    total = a[A_ACHARS];
    if (a[A_NSEQ] > 1) total += 2 * open_len + (a[A_NSEQ] - 1) * mid_len;
  } else if (valid && nd[MPRG_N_KIND] == MPRG_KIND_CLUSTER) total = 2 * open_len + (nd[MPRG_N_NCHILD] - 1) * mid_len;
  a[A_TOTAL] = total;
}
// per alignment: length of its PRG (column 0); per node: allele copy jobs of device leaves (column 0 of valsn)
KERNEL(k_as_msa_len, long long n_msas, const int64_t *root_of, const int32_t *failed, const int64_t *A, int64_t *vals) {
  const long long m = KF_GID;
  if (m >= n_msas) return;
  vals[m] = (root_of[m] >= 0 && !failed[m]) ? ASM(A, root_of[m])[A_TOTAL] : 0;
}
// allele copy jobs per node, at the node's PREORDER place (tree base + rank): after the prefix sums a locus's jobs — and its
// PRG index entries — are one contiguous run, leaves in preorder
KERNEL(k_as_job_count, const int64_t *nodes, long long n, const int64_t *A, const int64_t *tree_base, int64_t *valsn) {
  const long long i = KF_GID;
  if (i >= n) return;
  valsn[tree_base[NODE(nodes, i)[MPRG_N_MSA]] + ASM(A, i)[A_PRE]] = ASM(A, i)[A_JOB] < 0 ? 0 : ASM(A, i)[A_NSEQ];
}
// per alignment (columns of msa_base): 0 start of its PRG in the batch text, 1 its first allele copy job (= PRG index entry),
// 2 its first node in the preorder layouts, 3 (written by the export) its first entry of the exported row array
KERNEL(k_as_root_start, long long n_msas, const int64_t *root_of, const int32_t *failed, int64_t *A, int64_t *msa_base,
       const int64_t *tree_base, const int64_t *valsn) {
  const long long m = KF_GID;
  if (m >= n_msas) return;
  const long long tb = tree_base[m];
  msa_base[2 * n_msas + m] = tb;
  msa_base[n_msas + m] = root_of[m] >= 0 ? valsn[tb] : -1;
  if (root_of[m] < 0 || failed[m]) return;
  ASM(A, root_of[m])[A_START] = msa_base[m];
}
// top-down: text starts; the children of a cluster node are separated by its site markers
KERNEL(k_as_start, const int64_t *nodes, long long f0, long long n, int64_t *A) {
  const long long j = KF_GID;
  if (j >= n) return;
  const int64_t *nd = NODE(nodes, f0 + j);
  const long long nch = nd[MPRG_N_NCHILD], fc = nd[MPRG_N_FIRST_CHILD];
  if (nch <= 0) return;
  const int64_t *a = ASM(A, f0 + j);
  const bool pc = nd[MPRG_N_KIND] == MPRG_KIND_CLUSTER;
  const long long open_len = kf_digits(a[A_SITE]) + 2, mid_len = kf_digits(a[A_SITE] + 1) + 2;
  long long run = a[A_START] + (pc ? open_len : 0);
  for (long long c = 0; c < nch; ++c) {
    int64_t *ca = ASM(A, fc + c);
    ca[A_START] = run;
    run += ca[A_TOTAL] + (pc ? (c == nch - 1 ? open_len : mid_len) : 0);
  }
}
// leaves of one level -> allele copy jobs + the leaves' own site markers (k_leaf_jobs over the node table); cluster
// nodes of the level write their own markers (" s " before the first child, " s+1 " between children, " s " at the end)
// index_out (optional): 3 int32 per job {start, end of the allele inside its locus's PRG, node id} — the PRG index
// (recursion_tree.py:276-300), per locus contiguous like the jobs
#define LJ_BIG 128                     // a leaf of more alleles than this is laid out by its wavefront's 64 lanes together
KERNEL(k_as_leaf_jobs, const int64_t *nodes, long long f0, long long n, const int32_t *failed, const int64_t *A,
       const int64_t *valsn, const int64_t *tree_base, const int64_t *msa_base, const int64_t *meta, const int32_t *rowidx,
       const int32_t *reps_pos, const int32_t *reps_len, int64_t *jobs, uint8_t *out, int32_t *index_out) {
  const long long j = KF_GID;
  bool big = false;                      // this lane's leaf waits for the wavefront (no lane returns before the loop below)
  if (j < n && !failed[NODE(nodes, f0 + j)[MPRG_N_MSA]]) {
    const int64_t *nd = NODE(nodes, f0 + j), *a = ASM(A, f0 + j);
    if (nd[MPRG_N_KIND] == MPRG_KIND_CLUSTER) {
      const long long nch = nd[MPRG_N_NCHILD], fc = nd[MPRG_N_FIRST_CHILD], site = a[A_SITE];
      write_marker(out, a[A_START], site);
      for (long long c = 0; c < nch; ++c) {
        const int64_t *ca = ASM(A, fc + c);
        write_marker(out, ca[A_START] + ca[A_TOTAL], c == nch - 1 ? site : site + 1);
      }
    } else if (nd[MPRG_N_KIND] == MPRG_KIND_LEAF && a[A_JOB] >= 0) {
      if (a[A_NSEQ] > LJ_BIG) big = true;
      else {
        const int64_t *M = meta + nd[MPRG_N_MSA] * 6;
        const long long rm = M[0], pitch = M[2], rows_off = nd[MPRG_N_ROWS_OFF], col0 = nd[MPRG_N_COL0], ncols = nd[MPRG_N_NCOLS];
        const long long reps_off = nd[MPRG_N_REPS_OFF], na = a[A_NSEQ], site = na > 1 ? a[A_SITE] : 0;
        long long pos = a[A_START];
        const long long job0 = valsn[tree_base[nd[MPRG_N_MSA]] + a[A_PRE]], text0 = msa_base[nd[MPRG_N_MSA]];
        int64_t *J = jobs + 4 * job0;
        if (site) pos += write_marker(out, pos, site);
        for (long long q = 0; q < na; ++q) {
          const long long rp = reps_off < 0 ? 0 : reps_pos[reps_off + q];
          const long long len = reps_off < 0 ? ncols : reps_len[reps_off + q];
          const long long row = rows_off < 0 ? rp : rowidx[rows_off + rp];
          J[4 * q] = rm + row * pitch + col0; J[4 * q + 1] = ncols; J[4 * q + 2] = pos; J[4 * q + 3] = len;
          if (index_out) { int32_t *ix = index_out + 3 * (job0 + q); ix[0] = (int32_t)(pos - text0); ix[1] = (int32_t)(pos - text0 + len); ix[2] = (int32_t)a[A_PRE]; }
          pos += len;
          if (site) pos += write_marker(out, pos, q < na - 1 ? site + 1 : site);
        }
      }
    }
  }
  // the big leaves of this wavefront, one after the other: allele q's place = the leaf's start + the lengths (and markers) of the
  // alleles before it — a prefix sum over 64 alleles per step instead of one thread's walk over thousands (the root of a tall
  // alignment that does not cluster: 10 000 alleles in BASELINE config D)
  unsigned long long todo = __ballot(big);
  const int lane = wave_lane();
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const long long jj = __shfl(j, src);
    const int64_t *nd = NODE(nodes, f0 + jj), *a = ASM(A, f0 + jj);
    const int64_t *M = meta + nd[MPRG_N_MSA] * 6;
    const long long rm = M[0], pitch = M[2], rows_off = nd[MPRG_N_ROWS_OFF], col0 = nd[MPRG_N_COL0], ncols = nd[MPRG_N_NCOLS];
    const long long reps_off = nd[MPRG_N_REPS_OFF], na = a[A_NSEQ], site = a[A_SITE];           // (na > 1: a site)
    const long long job0 = valsn[tree_base[nd[MPRG_N_MSA]] + a[A_PRE]], text0 = msa_base[nd[MPRG_N_MSA]];
    int64_t *J = jobs + 4 * job0;
    const long long mid_len = kf_digits(site + 1) + 2, last_len = kf_digits(site) + 2;
    long long base = a[A_START] + last_len;                // behind the opening marker
    if (lane == 0) write_marker(out, a[A_START], site);
    for (long long q0 = 0; q0 < na; q0 += WAVE) {
      const long long q = q0 + lane;
      const bool live = q < na;
      long long len = 0, row = 0;
      if (live) {
        const long long rp = reps_off < 0 ? 0 : reps_pos[reps_off + q];
        len = reps_off < 0 ? ncols : reps_len[reps_off + q];
        row = rows_off < 0 ? rp : rowidx[rows_off + rp];
      }
      const long long step = live ? len + (q < na - 1 ? mid_len : last_len) : 0;
      const long long incl = wave_scan_incl_ll(step);
      const long long pos = base + incl - step;
      if (live) {
        J[4 * q] = rm + row * pitch + col0; J[4 * q + 1] = ncols; J[4 * q + 2] = pos; J[4 * q + 3] = len;
        if (index_out) { int32_t *ix = index_out + 3 * (job0 + q); ix[0] = (int32_t)(pos - text0); ix[1] = (int32_t)(pos - text0 + len); ix[2] = (int32_t)a[A_PRE]; }
        write_marker(out, pos + len, q < na - 1 ? site + 1 : site);
      }
      base += __shfl(incl, WAVE - 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// KE  export of the trees for the update data structure (reference subcommands/from_msa.py:114-127 pickles every locus's
//     PrgBuilder; here a locus's record is a slice of three device-built arrays)
// records: 8 int32 per node at its preorder place {parent's node id (-1: root), kind, nesting level, rows (-1: every row of the
// alignment, -2: its parent's rows), first of its rows in the locus's row array, first column, columns, alleles};
// rows: the MSA rows of the nodes that own a list (children of cluster nodes), per locus contiguous, nodes in preorder.
// ---------------------------------------------------------------------------------------------------------------
MPRG_DEV bool ex_owns_rows(const int64_t *nodes, const int64_t *nd) {
  return nd[MPRG_N_ROWS_OFF] >= 0 && nd[MPRG_N_PARENT] >= 0 && NODE(nodes, nd[MPRG_N_PARENT])[MPRG_N_KIND] == MPRG_KIND_CLUSTER;
}
KERNEL(k_ex_count, const int64_t *nodes, long long n, const int64_t *A, const int64_t *tree_base, int64_t *valsp) {
  const long long i = KF_GID;
  if (i >= n) return;
  const int64_t *nd = NODE(nodes, i);
  valsp[tree_base[nd[MPRG_N_MSA]] + ASM(A, i)[A_PRE]] = ex_owns_rows(nodes, nd) ? nd[MPRG_N_NROWS] : 0;
}
KERNEL(k_ex_fill, const int64_t *nodes, long long n, const int64_t *A, const int64_t *tree_base, const int64_t *valsp,
       const int32_t *pool, int32_t *records, int32_t *rows_out, int64_t *msa_base, long long n_msas) {
  const long long i = KF_GID;
  if (i >= n) return;
  const int64_t *nd = NODE(nodes, i), *a = ASM(A, i);
  const long long tb = tree_base[nd[MPRG_N_MSA]], pos = tb + a[A_PRE];
  int32_t *r = records + 8 * pos;
  const bool owns = ex_owns_rows(nodes, nd);
  const long long at = valsp[pos];
  r[0] = nd[MPRG_N_PARENT] < 0 ? -1 : (int32_t)ASM(A, nd[MPRG_N_PARENT])[A_PRE];
  r[1] = (int32_t)nd[MPRG_N_KIND]; r[2] = (int32_t)nd[MPRG_N_LEVEL];
  r[3] = nd[MPRG_N_ROWS_OFF] < 0 ? -1 : (owns ? (int32_t)nd[MPRG_N_NROWS] : -2);
  r[4] = (int32_t)(at - valsp[tb]);
  if (a[A_PRE] == 0) msa_base[3 * n_msas + nd[MPRG_N_MSA]] = at;
  r[5] = (int32_t)nd[MPRG_N_COL0]; r[6] = (int32_t)nd[MPRG_N_NCOLS]; r[7] = (int32_t)a[A_NSEQ];
  if (owns) for (long long q = 0; q < nd[MPRG_N_NROWS]; ++q) rows_out[at + q] = pool[nd[MPRG_N_ROWS_OFF] + q];
}

// KE'  the alignments of the exported loci at FOUR BITS per cell (the update data structure keeps every locus's alignment: 96 % of a
//      member's bytes, 6.5 GB of ASCII for a 30 000-gene pan-genome — the cell codes 0..11 fit a nibble).  Row r of alignment m:
//      ceil(C / 2) bytes at out_off[m] + r * ceil(C / 2), cell 2j in the low nibble of byte j, a last odd cell's partner 15.
//      One workgroup per row (row_base: the alignments' first rows in the launch, n_msas + 1 entries), a thread packs 8 cells.
KERNEL(k_ex_pack_rows, const uint8_t *arena, const int64_t *meta, const int64_t *row_base, const int64_t *out_off, long long n_msas,
       uint8_t *out) {
  const long long R = BLOCK_ID;
  long long lo = 0, hi = n_msas;
  while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (row_base[mid] <= R) lo = mid; else hi = mid; }
  const int64_t *M = meta + lo * 6;
  const long long r = R - row_base[lo], C = M[5], nb = (C + 1) >> 1;
  const uint8_t *src = arena + M[0] + r * M[2];          // row-major copy: pitch a multiple of 16, cells past C hold 15
  uint8_t *dst = out + out_off[lo] + r * nb;
  PAR_FOR(q, (nb + 3) >> 2) {
    uint32_t w0, w1;
    __builtin_memcpy(&w0, src + 8 * q, 4);
    __builtin_memcpy(&w1, src + 8 * q + 4, 4);          // (inside the row's pitch: C <= pitch, 8 q + 7 < 2 nb + 6 <= pitch + 8; the arena ends in 256 spare bytes)
    const uint32_t n0 = (w0 & 15u) | ((w0 >> 4) & 0xf0u) | ((w0 >> 8) & 0xf00u) | ((w0 >> 12) & 0xf000u);
    const uint32_t n1 = (w1 & 15u) | ((w1 >> 4) & 0xf0u) | ((w1 >> 8) & 0xf00u) | ((w1 >> 12) & 0xf000u);
    const uint32_t p = n0 | (n1 << 16);
    for (int b = 0; b < 4; ++b) if (4 * q + b < nb) dst[4 * q + b] = (uint8_t)(p >> (8 * b));
  }
}
