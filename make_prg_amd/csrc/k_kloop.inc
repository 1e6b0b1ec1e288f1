// ---------------------------------------------------------------------------------------------------------------
// KL  the reference's clustering loop of ONE problem inside ONE workgroup
//     reference from_msa/cluster_sequences.py:256-274:
//         while cluster_further(...): num_clusters += 1; KMeans(num_clusters).fit(X).predict(X); accept / revert
//
// Rounds 1-3 ran this loop as one set of launches per ROUND k for all problems of a recursion level (control step, two or
// three KMeans launch lists, cluster_further: ~4 launches and one host wait per round).  A launch lasts as long as its slowest
// workgroup, so a level paid ~9 x 3 fit latencies however few problems it held — the cost that decides small batches (one GPU of
// an 8-GPU run sees 3 750 alignments per step: 37 of 61 ms of device time were KMeans launches, 24 ms of them tails).
// Here a problem's workgroup walks k = 2, 3, ... itself: fit (the same body as mprg_kmeans_fit / _fit_small), best restart +
// predict, then cluster_further on the problem's dense gapped copy, then the reference's accept / revert / stop rules — no
// launch, no header, no host in between; a level is one launch per workgroup FORM (general 256-thread form; small form with a
// 6 x 6 centre table for k <= 6, continued by the 10 x 10 variant for the rare problem that goes on to k = 7).
// The decisions are k_kl_advance's (k_forest.inc), which this replaces on the batch host's path.
// ---------------------------------------------------------------------------------------------------------------

// ---- K9f  cluster_further of one problem by its own workgroup ---------------------------------------------------------
// cluster_sequences.py:59-111.  Majority strings: item = (cluster, column); a thread walks the view's rows once and counts the
// cluster's symbols in PACKED registers (12 symbols x FB bits: no LDS table, no run-time indexed array), so the phase needs no
// LDS beyond one byte per row (the row's cluster, staged in the fit's pool when it fits).  Narrow problems — the rule: a few
// dozen columns — would leave most lanes idle, so an item's rows are split over SLICES of threads whose packed words the item's
// first thread adds up from LDS (fields cannot overflow: every field counts rows of one view; plain stores and loads — a 64-bit
// atomic add through a generic pointer into LDS faulted on gfx950).  Counter.most_common's tie-break (the symbol seen
// first in the reference's row order: distinct sequence, then row) only needs the smallest key among the rows that hold a
// TIED symbol: a second walk by the deciding thread, only when two symbols tie.
// (KL_CF_FN: inlined; as a function of its own — tried: registers allocated apart from the fit.s — the kernel spilled four times as much)
#ifndef KL_CF_FN
#define KL_CF_FN MPRG_DEV
#endif
#ifdef MPRG_TEST_CF_GLOBAL                // test-only build: every problem takes the form for views beyond the LDS pool
#define KL_CF_IN_LDS(fits) false
#else
#define KL_CF_IN_LDS(fits) (fits)
#endif
#define KL_CF_FIELD_BITS 32             // one instantiation for any number of rows (16: three words instead of six, views below 65 536 rows)
MPRG_DEV int cf_row_cluster(int i, const uint8_t *mlab_s, const int32_t *dor, const int32_t *labels) {
  if (mlab_s) return mlab_s[i];
  const int dd = dor[i];
  return dd < 0 ? 255 : labels[dd];
}
template <int FB> struct CfWords {
  static constexpr int PER = 64 / FB, W = 12 / PER;
  unsigned long long w[W];
  MPRG_DEVM void clear() {
#pragma unroll
    for (int q = 0; q < W; ++q) w[q] = 0;
  }
  MPRG_DEVM void add(unsigned x) {                       // x >= 12 (padding, rows of other clusters): nothing
    const unsigned long long inc = x < 12 ? 1ull << (FB * (x % PER)) : 0ull;
    const unsigned sel = x / PER;
#pragma unroll
    for (int q = 0; q < W; ++q) w[q] += sel == (unsigned)q ? inc : 0ull;
  }
  MPRG_DEVM void addw(unsigned x, unsigned wgt) {        // the same for a row that stands for wgt identical rows
    const unsigned long long inc = x < 12 ? (unsigned long long)wgt << (FB * (x % PER)) : 0ull;
    const unsigned sel = x / PER;
#pragma unroll
    for (int q = 0; q < W; ++q) w[q] += sel == (unsigned)q ? inc : 0ull;
  }
  MPRG_DEVM unsigned long long count(int s) const {      // s: compile-time after unrolling
    return (w[s / PER] >> (FB * (s % PER))) & ((FB == 32) ? 0xffffffffull : 0xffffull);
  }
};
// returns (to every thread) whether some member row is farther than the one-reference-like threshold from its cluster's majority
// string.  pool: POOLB bytes of LDS free for this phase; maj: k strings of n codes (global scratch of the view); G: the view's dense
// gapped rows (row i at G + i * u_pitch(n)).  labels -> assign (the fit is accepted: the caller checked the label count).
template <int FB, int POOLB>
KL_CF_FN bool cf_problem_fb(const int S, const int n, const int D, const int k, const int32_t *dor, const int32_t *labels, int32_t *assign,
                            uint8_t *maj, const uint8_t *G, uint8_t *pool, int *flag_s) {
  typedef CfWords<FB> Words;
  const int cpitch = u_pitch(n);
  const bool staged = S <= POOLB;
  uint8_t *mlab_w = staged ? pool : nullptr;
  const uint8_t *mlab_s = mlab_w;
  const int items = k * n;
  // slices: only when every (item, slice) pair fits one pass and the accumulators fit behind the row labels
  const long long acc_off = staged ? ((S + 7) & ~7) : 0;
  int slices = 1;
#ifndef KL_NO_SLICES
  if (items * 2 <= N_THREADS) {
    slices = N_THREADS / items; if (slices > 16) slices = 16;
    if (acc_off + (long long)items * slices * Words::W * 8 > POOLB) slices = 1;          // (every slice's words get their own place)
  }
#endif
  unsigned long long *acc = (unsigned long long *)(pool + acc_off);
  PAR_FOR(q, D) { assign[q] = labels[q]; }
  if (staged) { PAR_FOR(i, S) { const int dd = dor[i]; mlab_w[i] = dd < 0 ? (uint8_t)255 : (uint8_t)labels[dd]; } }
  ONE_THREAD { flag_s[0] = 0; }
  BARRIER();
  for (int e0 = 0; e0 < items * slices; e0 += N_THREADS) {          // uniform trip count (one pass whenever slices > 1)
    const int e = e0 + (int)threadIdx.x;
    const bool live = e < items * slices;
    const int item = live ? (slices > 1 ? e % items : e) : 0, sl = slices > 1 ? e / items : 0;
    const int cl = (int)((unsigned)item / (unsigned)n), c = (int)((unsigned)item % (unsigned)n);
    Words cw;
    cw.clear();
    const uint8_t *col = G + c;
    if (live) {
      const int per = (S + slices - 1) / slices;
      int i = sl * per;
      const int i1 = (sl + 1) * per < S ? (sl + 1) * per : S;
      for (; i + 4 <= i1; i += 4) {
        int rc[4]; unsigned x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rc[q] = cf_row_cluster(i + q, mlab_s, dor, labels);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = rc[q] == cl ? (unsigned)col[(long long)(i + q) * cpitch] & 15u : 15u;
#pragma unroll
        for (int q = 0; q < 4; ++q) cw.add(x[q]);
      }
      for (; i < i1; ++i) if (cf_row_cluster(i, mlab_s, dor, labels) == cl) cw.add((unsigned)col[(long long)i * cpitch] & 15u);
      if (slices > 1 && sl > 0) {
#pragma unroll
        for (int q = 0; q < Words::W; ++q) acc[((long long)sl * items + item) * Words::W + q] = cw.w[q];
      }
    }
    if (slices > 1) {
      BARRIER();                                                     // (uniform: slices > 1 means a single pass)
      if (live && sl == 0) {                                         // packed fields add up: every field counts rows of this view
        for (int o = 1; o < slices; ++o)
#pragma unroll
          for (int q = 0; q < Words::W; ++q) cw.w[q] += acc[((long long)o * items + item) * Words::W + q];
      }
    }
    if (live && sl == 0) {
      unsigned long long best_n = 0;
#pragma unroll
      for (int s = 0; s < 12; ++s) { const unsigned long long a = cw.count(s); best_n = a > best_n ? a : best_n; }
      unsigned tied = 0;
#pragma unroll
      for (int s = 0; s < 12; ++s) if (cw.count(s) == best_n) tied |= 1u << s;
      int best = __ffs(tied) - 1;
      if (best_n > 0 && (tied & (tied - 1))) {                       // several symbols share the maximum: the one seen first wins
        long long best_key = 0x7fffffffffffffffLL;
#pragma nounroll
        for (int i = 0; i < S; ++i) {
          if (cf_row_cluster(i, mlab_s, dor, labels) != cl) continue;
          const unsigned x = (unsigned)col[(long long)i * cpitch] & 15u;
          if (!((tied >> x) & 1u)) continue;
          const long long key = (long long)dor[i] * S + i;
          if (key < best_key) { best_key = key; best = (int)x; }
        }
      }
      maj[(long long)cl * n + c] = (uint8_t)best;
    }
  }
  BARRIER();
  const int thresh = n < 5 ? 1 : (int)(0.2 * (double)n);
  PAR_FOR(i, S) {
    const int cl = cf_row_cluster((int)i, mlab_s, dor, labels);
    if (cl == 255) continue;
    const uint8_t *m = maj + (long long)cl * n;
    const uint8_t *grow = G + (long long)i * cpitch;
    int dist = 0;
#pragma nounroll
    for (int c = 0; c < n && dist <= thresh; c += 8) {               // 8 cells of the row and of the majority string per load
      uint64_t x, y;
      __builtin_memcpy(&x, grow + c, 8);                             // (the row's pitch is a multiple of 16: in bounds)
      __builtin_memcpy(&y, m + c, 8);                                // (the majority strings are followed by scratch: in bounds)
      uint64_t v = (x ^ y) & 0x0f0f0f0f0f0f0f0fULL;
      if (c + 8 > n) v &= 0xffffffffffffffffULL >> (8 * (c + 8 - n));
      const uint64_t nz = (((v & 0x7f7f7f7f7f7f7f7fULL) + 0x7f7f7f7f7f7f7f7fULL) | v) & 0x8080808080808080ULL;
      dist += __popcll(nz);
    }
    if (dist > thresh) flag_s[0] = 1;
  }
  BARRIER();
  const bool further = flag_s[0] != 0;
  BARRIER();                                                         // (flag_s and the pool are free again)
  return further;
}

// The same for a problem whose cells fit the pool next to its row labels (the rule: ~100 rows x a few dozen columns): the dense
// gapped rows (low nibbles, pitch = columns rounded up to 4), each row's cluster and distinct-sequence index and the k majority
// strings all live in LDS, so the per-row walks — and the tie-break's second walk, which small clusters need on most variant
// columns — are LDS reads instead of dependent global loads (measured before: 69 k cycles per fit in this phase, the tie-break's
// row-by-row global round trips most of it).
// (cf_lds_bytes: k_cluster.inc)
// OPT (mprg_cluster_further's one-workgroup launch only; the fused loops instantiate it without, unchanged): labels may be null — one
// cluster holding every member, the k = 1 check — and assign may be null (the fit was not accepted: nothing to copy)
// CLS (the same launch, given mprg_ungap_dedupe's rep_g: the smallest row of the view with identical gapped content): rows of one gapped
// class share their distinct sequence — hence their cluster —, their symbol in every column and their distance to any string, so only
// the REPRESENTATIVES (rep_g[i] == i) are listed, staged and walked, each counting for its class's size: a column's counts are sums of
// class sizes, the tie-break's smallest key (distinct sequence, row) is a representative's — the smallest row of its class —, and
// "some row is too far" is decided by the representatives.  A pan-genome view of ~100 rows holds ~16 such classes.  Tables: the row's
// distinct-sequence index widens to 32 bits (class size in the high half, LDS atomics) and a 16-bit list of the representatives'
// rows follows it: 4 S bytes more (cf_lds_bytes_cls); flag_s[1] counts the list.
template <bool OPT = false, bool CLS = false>
MPRG_DEV bool cf_problem_lds(const int S, const int n, const int D, const int k, const int32_t *dor, const int32_t *labels, int32_t *assign,
                             const uint8_t *G, uint8_t *pool, int *flag_s, const int32_t *rep_g = nullptr, uint8_t *maj_out = nullptr) {
  typedef CfWords<16> Words;
  const int cpitch = u_pitch(n), cp = (n + 3) & ~3, cw4 = cp >> 2;
  uint8_t *mlab = pool;
  if constexpr (CLS) {
    uint32_t *dkw = (uint32_t *)(pool + ((S + 3) & ~3));
    uint16_t *list = (uint16_t *)(dkw + S);
    uint8_t *majs = (uint8_t *)list + ((2 * S + 3) & ~3);
    uint8_t *cells = majs + k * cp;
    if (assign) { PAR_FOR(q, D) { assign[q] = labels[q]; } }
    PAR_FOR(i, S) { const int dd = dor[i]; mlab[i] = dd < 0 ? (uint8_t)255 : (!labels ? (uint8_t)0 : (uint8_t)labels[dd]); dkw[i] = (uint32_t)dd & 0xffffu; }
    ONE_THREAD { flag_s[0] = 0; flag_s[1] = 0; }
    BARRIER();
    PAR_FOR(i, S) {
      int r = rep_g[i];
      if ((unsigned)r > (unsigned)i) r = (int)i;                       // (a representative is the smallest row of its class: never beyond the row)
      atomicAdd(dkw + r, 0x10000u);
      if (r == (int)i) list[atomicAdd(flag_s + 1, 1)] = (uint16_t)i;   // (any order: counts add, the smallest key wins, the flag only goes 0 -> 1)
    }
    BARRIER();
    const int R = flag_s[1];
    PAR_FOR(e, R * cw4) {                                              // representative j's cells at cells + j * cp
      const int j = (int)((unsigned)e / (unsigned)cw4), w = (int)((unsigned)e % (unsigned)cw4);
      *(uint32_t *)(cells + j * cp + 4 * w) = *(const uint32_t *)(G + (long long)list[j] * cpitch + 4 * w) & 0x0f0f0f0fu;
    }
    BARRIER();
    PAR_FOR(item, k * n) {
      const int cl = (int)((unsigned)item / (unsigned)n), c = (int)((unsigned)item % (unsigned)n);
      Words cw;
      cw.clear();
      const uint8_t *col = cells + c;
      int j = 0;
      for (; j + 4 <= R; j += 4) {
        unsigned ri[4], rc[4], wt[4], x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ri[q] = list[j + q]; x[q] = col[(j + q) * cp]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) { rc[q] = mlab[ri[q]]; wt[q] = dkw[ri[q]] >> 16; }
#pragma unroll
        for (int q = 0; q < 4; ++q) cw.addw(rc[q] == (unsigned)cl ? x[q] : 15u, wt[q]);
      }
      for (; j < R; ++j) { const int i = list[j]; cw.addw(mlab[i] == cl ? (unsigned)col[j * cp] : 15u, dkw[i] >> 16); }
      unsigned long long best_n = 0;
#pragma unroll
      for (int s_ = 0; s_ < 12; ++s_) { const unsigned long long a = cw.count(s_); best_n = a > best_n ? a : best_n; }
      unsigned tied = 0;
#pragma unroll
      for (int s_ = 0; s_ < 12; ++s_) if (cw.count(s_) == best_n) tied |= 1u << s_;
      int best = __ffs(tied) - 1;
      if (best_n > 0 && (tied & (tied - 1))) {                         // several symbols share the maximum: the one seen first wins
        int best_key = 0x7fffffff;
#pragma nounroll
        for (int r = 0; r < R; ++r) {
          const unsigned x = col[r * cp];
          const int i = list[r];
          if (mlab[i] != cl || !((tied >> x) & 1u)) continue;
          const int key = (int)(dkw[i] & 0xffffu) * S + i;
          if (key < best_key) { best_key = key; best = (int)x; }
        }
      }
      majs[cl * cp + c] = (uint8_t)best;
      if (maj_out) maj_out[cl * n + c] = (uint8_t)best;
    }
    BARRIER();
    const int thresh = n < 5 ? 1 : (int)(0.2 * (double)n);
    PAR_FOR(j, R) {
      const int cl = mlab[list[j]];
      if (cl == 255) continue;
      const uint8_t *m = majs + cl * cp, *row = cells + j * cp;
      int dist = 0;
#pragma nounroll
      for (int c = 0; c < n; c += 4) {
        uint32_t v = *(const uint32_t *)(row + c) ^ *(const uint32_t *)(m + c);
        if (c + 4 > n) v &= 0xffffffffu >> (8 * (c + 4 - n));
        const uint32_t nz = (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;
        dist += __popc(nz);
      }
      if (dist > thresh) flag_s[0] = 1;
    }
    BARRIER();
    const bool further = flag_s[0] != 0;
    BARRIER();
    return further;
  }
  uint16_t *dk = (uint16_t *)(pool + ((S + 3) & ~3));
  uint8_t *majs = (uint8_t *)dk + ((2 * S + 3) & ~3);
  uint8_t *cells = majs + k * cp;
  if (!OPT || assign) { PAR_FOR(q, D) { assign[q] = labels[q]; } }
  PAR_FOR(i, S) { const int dd = dor[i]; mlab[i] = dd < 0 ? (uint8_t)255 : ((OPT && !labels) ? (uint8_t)0 : (uint8_t)labels[dd]); dk[i] = (uint16_t)dd; }
  PAR_FOR(e, S * cw4) {                                              // (a row of G is u_pitch(n) >= cp bytes: in bounds)
    const int i = (int)((unsigned)e / (unsigned)cw4), w = (int)((unsigned)e % (unsigned)cw4);
    *(uint32_t *)(cells + i * cp + 4 * w) = *(const uint32_t *)(G + (long long)i * cpitch + 4 * w) & 0x0f0f0f0fu;
  }
  ONE_THREAD { flag_s[0] = 0; }
  BARRIER();
  PAR_FOR(item, k * n) {
    const int cl = (int)((unsigned)item / (unsigned)n), c = (int)((unsigned)item % (unsigned)n);
    Words cw;
    cw.clear();
    const uint8_t *col = cells + c;
    int i = 0;
    for (; i + 4 <= S; i += 4) {
      unsigned rc[4], x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { rc[q] = mlab[i + q]; x[q] = col[(i + q) * cp]; }
#pragma unroll
      for (int q = 0; q < 4; ++q) cw.add(rc[q] == (unsigned)cl ? x[q] : 15u);
    }
    for (; i < S; ++i) cw.add(mlab[i] == cl ? (unsigned)col[i * cp] : 15u);
    unsigned long long best_n = 0;
#pragma unroll
    for (int s_ = 0; s_ < 12; ++s_) { const unsigned long long a = cw.count(s_); best_n = a > best_n ? a : best_n; }
    unsigned tied = 0;
#pragma unroll
    for (int s_ = 0; s_ < 12; ++s_) if (cw.count(s_) == best_n) tied |= 1u << s_;
    int best = __ffs(tied) - 1;
    if (best_n > 0 && (tied & (tied - 1))) {                         // several symbols share the maximum: the one seen first wins
      int best_key = 0x7fffffff;
#pragma nounroll
      for (int r = 0; r < S; ++r) {
        const unsigned x = col[r * cp];
        if (mlab[r] != cl || !((tied >> x) & 1u)) continue;
        const int key = (int)dk[r] * S + r;
        if (key < best_key) { best_key = key; best = (int)x; }
      }
    }
    majs[cl * cp + c] = (uint8_t)best;
  }
  BARRIER();
  const int thresh = n < 5 ? 1 : (int)(0.2 * (double)n);
  PAR_FOR(i, S) {
    const int cl = mlab[i];
    if (cl == 255) continue;
    const uint8_t *m = majs + cl * cp, *row = cells + i * cp;
    int dist = 0;
#pragma nounroll
    for (int c = 0; c < n; c += 4) {
      uint32_t v = *(const uint32_t *)(row + c) ^ *(const uint32_t *)(m + c);
      if (c + 4 > n) v &= 0xffffffffu >> (8 * (c + 4 - n));
      const uint32_t nz = (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;
      dist += __popc(nz);
    }
    if (dist > thresh) flag_s[0] = 1;
  }
  BARRIER();
  const bool further = flag_s[0] != 0;
  BARRIER();
  return further;
}

// ---- the loop ---------------------------------------------------------------------------------------------------------
struct KlUoff { int32_t v[KM_KMAX + 1]; };               // offset (doubles) of k's uniforms in uniforms_dev, k = 2..10
// stats (device, int64 / double words; the forest's step header): 80 fits run, 85 / 93 KMeans algorithmic bytes of the fits run
// in the general / small form (double), 82 a fit's relocation ran out of frames, 84 cells visited by cluster_further (double)
enum { KL_ST_FITS = 80, KL_ST_BAD = 82, KL_ST_CF = 84, KL_ST_BYTES_GENERAL = 85, KL_ST_BYTES_SMALL = 93 };
// K_LO..K_HI: the k this form runs (a problem that wants a k beyond K_HI stays active for the next form)
template <int RMAX, int NEEDCAP, int LAB8, int POOLB, int KCH, int K_HI>
MPRG_DEV void kl_problem(const int b, const int64_t *prob_all, int n_init, const double *uniforms_all, const KlUoff &uoff,
                         const double *xcounts, double *ws_all, const int64_t *views, const int32_t *d_of_row_all,
                         const uint8_t *gcodes_all, int32_t *scratch_all, int32_t *labels_all, int32_t *assign_all, double *km_info,
                         int32_t *km_status, int32_t *num_clusters, int32_t *active, int64_t *stats, int bytes_slot, uint8_t *pool,
                         int sel_lab_cap) {
  // (what the loop carries from round to round lives in LDS, and what a phase needs it derives when it gets there: the fit's body
  //  already wants more registers than a wave has at four waves per SIMD)
  SHARED(int32_t, ki_s, 8);
  SHARED(int, cf_flag, 1);
  SHARED(int, st_i, 4);                  // 0 accepted clusters so far, 1 still active, 2 fits run, 3 a fit ran out of frames
  SHARED(double, st_d, 2);               // 0 KMeans bytes, 1 cluster_further cells
  ONE_THREAD { st_i[0] = num_clusters[b]; st_i[1] = 1; st_i[2] = 0; st_i[3] = 0; st_d[0] = 0; st_d[1] = 0; }
  BARRIER();
  for (;;) {
    const int k = st_i[0] + 1;
    const int D = (int)prob_all[(long long)b * PF + 1];
    BARRIER();                                                        // (every thread has read the round's state)
    if (k > KM_KMAX || k == D) { ONE_THREAD { st_i[0] = k; st_i[1] = 0; } break; }      // cluster_sequences.py:258-261
    if (k > K_HI) break;                                              // the next form goes on from here (still active)
    ONE_THREAD { ki_s[0] = b; ki_s[1] = k; ki_s[2] = 0; ki_s[3] = uoff.v[k]; ki_s[4] = 0; km_status[b] = 0; }
    BARRIER();
    km_restarts_body<RMAX, NEEDCAP, LAB8, POOLB, KCH>(0, prob_all, ki_s, n_init, uniforms_all, xcounts, ws_all, nullptr, km_status + b, pool);
    BARRIER();
    KM_T0();
    km_select_body(0, prob_all, ki_s, n_init, xcounts, ws_all, nullptr, labels_all, km_info + 8 * (long long)b, (int32_t *)pool, sel_lab_cap);
    BARRIER(); KM_T(12);
    const int64_t *P = prob_all + (long long)b * PF;
    const double *info = km_info + 8 * (long long)b;
    const bool accepted = info[3] >= (double)k;                       // fewer than k distinct labels: revert and stop (:267-273)
    const ViewD d = load_view(views, (int)P[0]);
    ONE_THREAD {
      st_i[2] += 1;
      st_d[0] += 8.0 * (double)P[1] * (double)P[7] * (info[4] + (double)n_init);
      if (km_status[b] & MPRG_KM_UNSUPPORTED) st_i[3] = 1;
      if (accepted) { st_i[0] = k; st_d[1] += (double)d.n_rows * (double)d.n_cols; }
      else st_i[1] = 0;
    }
    if (!accepted) break;
    const int32_t *dor = d_of_row_all + d.row_off;
    int32_t *labels = labels_all + P[10], *assign = assign_all + P[10];
    uint8_t *maj = (uint8_t *)(scratch_all + d.col_off * 3);
    const uint8_t *G = gcodes_all + d.aux0;
#ifdef KL_DEBUG_NO_CF
    const bool further = false && dor && labels && assign && maj && G;
#else
    const bool further = KL_CF_IN_LDS(cf_lds_bytes(d.n_rows, d.n_cols, k) <= POOLB)
                             ? cf_problem_lds(d.n_rows, d.n_cols, (int)P[1], k, dor, labels, assign, G, pool, cf_flag)
                             : cf_problem_fb<KL_CF_FIELD_BITS, POOLB>(d.n_rows, d.n_cols, (int)P[1], k, dor, labels, assign, maj, G, pool, cf_flag);
#endif
    KM_T(13);
    if (!further) { ONE_THREAD { st_i[1] = 0; } break; }              // every cluster is one-reference-like: accepted, done
  }
  BARRIER();
  ONE_THREAD {
    num_clusters[b] = st_i[0]; active[b] = st_i[1];
    if (st_i[2]) {
      atomicAdd((unsigned long long *)stats + KL_ST_FITS, (unsigned long long)st_i[2]);
      atomicAdd((double *)stats + bytes_slot, st_d[0]);
      if (st_d[1] != 0) atomicAdd((double *)stats + KL_ST_CF, st_d[1]);
      if (st_i[3]) stats[KL_ST_BAD] = 1;
    }
  }
}

// general form: any problem (the ones the small form takes return at once when `skip_small`)
KERNEL_OCC(k_cluster_loop, KM_WAVES, const int64_t *prob_all, int n_init, const double *uniforms_all, KlUoff uoff, const double *xcounts,
           double *ws_all, const int64_t *views, const int32_t *d_of_row_all, const uint8_t *gcodes_all, int32_t *scratch_all,
           int32_t *labels_all, int32_t *assign_all, double *km_info, int32_t *km_status, int32_t *num_clusters, int32_t *active,
           int64_t *stats, int skip_small, DsCount dc) {
  DS_GUARD(dc, 1);
  __shared__ __attribute__((aligned(16))) uint8_t pool[KM_XL_BYTES];
  const int b = BLOCK_ID;
  if (!active[b]) return;
  const int64_t *P = prob_all + (long long)b * PF;
  if ((skip_small & 1) && km_small_class(P[1], P[7], 2, n_init) >= 0) return;
  if ((skip_small & 2) && kml_class_ws(P[1], P[7], num_clusters[b] + 1, n_init, true, ws_all + P[9]) >= 0) return;          // (its next round is the LDS form's)
  kl_problem<KM_RMAX, KM_NEED_CAP, KM_LAB8, KM_XL_BYTES, KM_KMAX * KM_KMAX, KM_KMAX>(
      b, prob_all, n_init, uniforms_all, uoff, xcounts, ws_all, views, d_of_row_all, gcodes_all, scratch_all, labels_all, assign_all, km_info,
      km_status, num_clusters, active, stats, KL_ST_BYTES_GENERAL, pool, KM_SEL_LABELS);
}
// small form (128 threads, 8 KB pool): KCH = 36 runs k = 2..6, KCH = 100 continues the problems still active with k = 7..10
// (the k = 7..10 variant's 24 KB of LDS hold a CU to six workgroups = three waves per SIMD: it is given the registers of three —
//  left at four the compiler took 231 and two waves per SIMD, four workgroups per CU, for the rounds that carry 40 % of the work)
#ifndef KL_WAVES_HIGH
#define KL_WAVES_HIGH 3
#endif
template <int KCH, int K_HI>
__attribute__((amdgpu_flat_work_group_size(64, 128), amdgpu_waves_per_eu((KCH > 36 ? KL_WAVES_HIGH : KM_WAVES), (KCH > 36 ? KL_WAVES_HIGH : KM_WAVES)))) __global__ void k_cluster_loop_small(
    const int64_t *prob_all, int n_init, const double *uniforms_all, KlUoff uoff, const double *xcounts, double *ws_all,
    const int64_t *views, const int32_t *d_of_row_all, const uint8_t *gcodes_all, int32_t *scratch_all, int32_t *labels_all,
    int32_t *assign_all, double *km_info, int32_t *km_status, int32_t *num_clusters, int32_t *active, int64_t *stats, DsCount dc) {
  DS_GUARD(dc, 1);
  __shared__ __attribute__((aligned(16))) uint8_t pool[KMS_POOL];
  const int b = BLOCK_ID;
  if (!active[b]) return;
  const int64_t *P = prob_all + (long long)b * PF;
  if (km_small_class(P[1], P[7], 2, n_init) < 0) return;
  kl_problem<KMS_RMAX, KMS_NEEDCAP, KMS_LAB8, KMS_POOL, KCH, K_HI>(
      b, prob_all, n_init, uniforms_all, uoff, xcounts, ws_all, views, d_of_row_all, gcodes_all, scratch_all, labels_all, assign_all, km_info,
      km_status, num_clusters, active, stats, KL_ST_BYTES_SMALL, pool, KMS_POOL / 4);
}

// ---- the loop on the LDS form of the fit (round 6; k_kmeans_lds.inc): a launch per LDS class, in ascending order.  A problem's
//      workgroup runs its rounds while the round's fit is of a class this launch's dynamic LDS holds (kml_class(D, V, k) <= cls) and
//      leaves the problem ACTIVE when the next round needs more — the next class's launch goes on from there (the state a fit keeps
//      in LDS grows with k); a round no class holds is the general form's (launched after the classes).  cluster_further takes the
//      same dynamic pool (cf_problem_lds when the view's cells fit it).
MPRG_DEV void kll_problem(const int b, const int64_t *prob_all, int n_init, const double *uniforms_all, const KlUoff &uoff,
                          const double *xcounts, double *ws_all, const int64_t *views, const int32_t *d_of_row_all,
                          const uint8_t *gcodes_all, int32_t *scratch_all, int32_t *labels_all, int32_t *assign_all, double *km_info,
                          int32_t *km_status, int32_t *num_clusters, int32_t *active, int64_t *stats, uint8_t *pool, const int lds_bytes,
                          const int cls) {
  SHARED(int32_t, ki_s, 8);
  SHARED(int, cf_flag, 1);
  SHARED(int, st_i, 4);                  // 0 accepted clusters so far, 1 still active, 2 fits run, 3 a fit ran out of frames
  SHARED(double, st_d, 2);               // 0 KMeans bytes, 1 cluster_further cells
  ONE_THREAD { st_i[0] = num_clusters[b]; st_i[1] = 1; st_i[2] = 0; st_i[3] = 0; st_d[0] = 0; st_d[1] = 0; }
  BARRIER();
  const int64_t *P = prob_all + (long long)b * PF;
  const int D = (int)P[1], V = (int)P[7];
  // the problem's counts (bytes) and feature means are staged by its first round here and stay at the head of the pool for the later
  // ones: everything else — the seeding's rows, the restarts' state, cluster_further's tables — lives behind them (kml_layout's `keep`)
  const int lds_size = lds_bytes & 0xffffff, head = kml_layout(D, V, 2, n_init, true).lb;
  bool staged = false;                                                // (uniform: every thread takes the same decisions)
  for (;;) {
    const int k = st_i[0] + 1;
    BARRIER();                                                        // (every thread has read the round's state)
    if (k > KM_KMAX || k == D) { ONE_THREAD { st_i[0] = k; st_i[1] = 0; } break; }      // cluster_sequences.py:258-261
    const int c = kml_class_ws(D, V, k, n_init, true, ws_all + P[9]);
    if (c < 0 || c > cls) break;                                      // a later launch goes on from here (still active)
    ONE_THREAD { ki_s[0] = b; ki_s[1] = k; ki_s[2] = 0; ki_s[3] = uoff.v[k]; ki_s[4] = 0; ki_s[5] = n_init; km_status[b] = 0; }
    BARRIER();
    kml_fit_body(0, prob_all, ki_s, n_init, uniforms_all, xcounts, ws_all, labels_all, km_info + 8 * (long long)b, km_status + b, pool,
                 lds_bytes | (2 << 24) | (staged ? (4 << 24) : 0));
    staged = true;
    BARRIER();
    KM_T0();
    const double *info = km_info + 8 * (long long)b;
    const bool accepted = info[3] >= (double)k;                       // fewer than k distinct labels: revert and stop (:267-273)
    const ViewD d = load_view(views, (int)P[0]);
    ONE_THREAD {
      st_i[2] += 1;
      st_d[0] += 8.0 * (double)P[1] * (double)P[7] * (info[4] + (double)ki_s[5]);          // (8 D V from the problem's row here: a value kept for this across the fit costs a register)
      if (km_status[b] & MPRG_KM_UNSUPPORTED) st_i[3] = 1;
      if (accepted) { st_i[0] = k; st_d[1] += (double)d.n_rows * (double)d.n_cols; }
      else st_i[1] = 0;
    }
    if (!accepted) break;
    const int32_t *dor = d_of_row_all + d.row_off;
    int32_t *labels = labels_all + P[10], *assign = assign_all + P[10];
    uint8_t *maj = (uint8_t *)(scratch_all + d.col_off * 3);
    const uint8_t *G = gcodes_all + d.aux0;
    // (cluster_further behind the counts where its tables fit there; else over the whole pool, and the next round stages the counts again)
    const bool cf_behind = KL_CF_IN_LDS(cf_lds_bytes(d.n_rows, d.n_cols, k) <= lds_size - head);
    const bool further = cf_behind ? cf_problem_lds(d.n_rows, d.n_cols, D, k, dor, labels, assign, G, pool + head, cf_flag)
                                   : cf_problem_fb<KL_CF_FIELD_BITS, KML_C0>(d.n_rows, d.n_cols, D, k, dor, labels, assign, maj, G, pool, cf_flag);
    if (!cf_behind) staged = false;
    KM_T(13);
    if (!further) { ONE_THREAD { st_i[1] = 0; } break; }              // every cluster is one-reference-like: accepted, done
  }
  BARRIER();
  ONE_THREAD {
    num_clusters[b] = st_i[0]; active[b] = st_i[1];
    if (st_i[2]) {
      atomicAdd((unsigned long long *)stats + KL_ST_FITS, (unsigned long long)st_i[2]);
      atomicAdd((double *)stats + KL_ST_BYTES_SMALL, st_d[0]);
      if (st_d[1] != 0) atomicAdd((double *)stats + KL_ST_CF, st_d[1]);
      if (st_i[3]) stats[KL_ST_BAD] = 1;
    }
  }
}
__attribute__((amdgpu_flat_work_group_size(64, 1024), amdgpu_waves_per_eu(KM_WAVES, KM_WAVES))) __global__ void k_cluster_loop_lds(
    const int64_t *prob_all, int n_init, const double *uniforms_all, KlUoff uoff, const double *xcounts, double *ws_all,
    const int64_t *views, const int32_t *d_of_row_all, const uint8_t *gcodes_all, int32_t *scratch_all, int32_t *labels_all,
    int32_t *assign_all, double *km_info, int32_t *km_status, int32_t *num_clusters, int32_t *active, int64_t *stats, int cls, int lds_bytes,
    DsCount dc) {
  DS_GUARD(dc, 1);
  HIP_DYNAMIC_SHARED(uint8_t, pool)
  const int b = BLOCK_ID;
  if (!active[b]) return;
  const int64_t *P = prob_all + (long long)b * PF;
  const int c = kml_class_ws(P[1], P[7], num_clusters[b] + 1, n_init, true, ws_all + P[9]);
  if (c < 0 || c > cls) return;                            // (its next round is a later launch's)
  kll_problem(b, prob_all, n_init, uniforms_all, uoff, xcounts, ws_all, views, d_of_row_all, gcodes_all, scratch_all, labels_all, assign_all, km_info,
              km_status, num_clusters, active, stats, pool, lds_bytes, cls);
}

// ---- K9o  mprg_cluster_further for a problem whose cells fit CFO_POOL bytes of LDS (the rule: ~100 rows x a few dozen columns): ONE
//      workgroup does what k_cluster_majority + k_cluster_hamming do in two launches over (problem, tile) / (problem, chunk) grids —
//      cf_problem_lds, the form the fused loops run (rows, clusters, majority strings and cells in LDS; packed register counters).
//      The two-launch kernels leave these problems alone (cf_one_fits, same rule on both sides).
KERNEL(k_cluster_further_one, const int64_t *views, const int64_t *prob_all, int n_probs, int k, const int32_t *d_of_row_all,
       const int32_t *labels_all, int32_t *assign_all, const double *km_info, int32_t *out_further, const uint8_t *gcodes_all,
       const int32_t *kinfo, const int32_t *rep_g_all, int by_reps, int32_t *scratch_all, DsCount dc) {
  DS_GUARD(dc, 1);
  const int b = BLOCK_ID;
  if (kinfo && kinfo[5 * (long long)b + 1] == 0) return;          // this problem sat the round out (k_kl_advance)
  const int64_t *P = prob_all + (long long)b * PF;
  const ViewD d = load_view(views, (int)P[0]);
  __shared__ __attribute__((aligned(16))) uint8_t pool[CFO_POOL];
  SHARED(int, flag, 2);                                           // 0 some row is too far, 1 representatives listed (rep_g)
  // a view that only fits if few of its rows are representatives (cf_one_asks_g): count them — cf_rep, the test cf_problem_lds lists them
  // by, so the list it stages cannot be longer than the G the rule admitted, whatever rep_g holds — and leave G for the launches behind
  const bool asks = rep_g_all && by_reps && cf_one_asks_g(d.n_rows, d.n_cols, k);
  int reps = 0;
  if (asks) {
    ONE_THREAD { flag[1] = 0; }
    BARRIER();
    const int32_t *rg = rep_g_all + d.row_off;
    int mine = 0;
    PAR_FOR(i, d.n_rows) { mine += cf_rep(rg, i) == (int)i ? 1 : 0; }
    if (mine) ATOMIC_ADD(flag + 1, mine);
    BARRIER();
    reps = flag[1];
    ONE_THREAD { *cf_g_slot(scratch_all, d) = (uint16_t)reps; }
    BARRIER();                                                    // (everyone has read the count: cf_problem_lds starts the list over)
  }
  if (!(asks ? cf_one_fits_cls(d.n_rows, d.n_cols, k, reps) : cf_one_takes(d, k, rep_g_all != nullptr, false, scratch_all))) return;
  const int32_t *labels = labels_all ? labels_all + P[10] : nullptr;
  // accepted fit: its labels become the problem's assignment (a fit with fewer than k distinct labels is not: cluster_sequences.py:267-273)
  int32_t *assign = (labels && assign_all && (!km_info || km_info[8 * (long long)b + 3] >= (double)k)) ? assign_all + P[10] : nullptr;
  // (a view admitted by its representatives leaves its majority strings in `scratch`, where the tiled kernels left them before the rule)
  uint8_t *maj_out = asks ? (uint8_t *)(scratch_all + d.col_off * 3) : nullptr;
  const bool further = rep_g_all ? cf_problem_lds<true, true>(d.n_rows, d.n_cols, (int)P[1], k, d_of_row_all + d.row_off, labels, assign, gcodes_all + d.aux0,
                                                              pool, flag, rep_g_all + d.row_off, maj_out)
                                 : cf_problem_lds<true>(d.n_rows, d.n_cols, (int)P[1], k, d_of_row_all + d.row_off, labels, assign, gcodes_all + d.aux0, pool, flag);
  ONE_THREAD { out_further[b] = further ? 1 : 0; }
}
