// ---------------------------------------------------------------------------------------------------------------
// K7l + K8l  the LDS form of a SMALL KMeans fit (round 6): the form every pan-genome fit takes
//     reference call site from_msa/cluster_sequences.py:262-266; arithmetic = scikit-learn's, as k_kmeans.inc restates it
//     (_kmeans.py:174-272 k-means++, _k_means_elkan.pyx:24-97 / :186-350 / :352-427 Elkan, _k_means_common.pyx:95-295,
//      _kmeans.py:1500-1531 best restart, _k_means_lloyd.pyx:168-218 predict) — every sum in the order the CPU kernel runs it.
//
// Why a new body.  The workgroup forms of k_kmeans.inc keep the state of a fit's ten restarts — lower bounds, this iteration's
// distances, upper bounds, labels, centre shifts and norms — in the problem's WORKSPACE (global memory): 217 KB of regions for a
// median fit of 14 sequences x 90 k-mers.  Every one of the ~45 barrier-separated phases of a fit then starts with a round trip to
// L2 (0.8 us under load, 22-29 cache lines per load instruction: profiles/r05/counters/) for a few hundred bytes that the
// workgroup itself wrote a phase earlier; a wave waits 78 % of its life.  Here the state of ALL restarts lives in LDS for the whole
// fit, sized by the fit (dynamic LDS, four classes), and so do the k-means++ seeding's inputs (the restarts' uniforms, the row
// norms and — where they fit — the sample-sample tables g1 / g4 of K6): the E-step, the bound updates, the list of needed pairs,
// init_bounds, the seeding's pick / score / sum rounds, the inertia sums, best restart and predict() touch no global memory.
// What stays global: the centres (two buffers of k x V doubles per restart: 58 KB for the median fit) and the rare relocation.
// Also less WORK per fit than the forms it replaces:
//   * M-step: a thread owns (restart, feature) and walks the restart's samples SORTED BY CLUSTER (a list the E-step's labels
//     give: members of cluster 0 in sample order, then cluster 1, ...) — one running sum, D additions; before: k running sums
//     and a select per (sample, cluster), k D additions.  Every per-cluster sum still adds its members in sample order.
//   * index arithmetic: 32-bit LDS offsets; divisions of item indices by D, k, V, D k ... are multiplications by a reciprocal
//     computed once per fit (KmlDiv: exact for the ranges the class rule admits).
// ---------------------------------------------------------------------------------------------------------------
#define KML_RMAX 10                    // restarts side by side
#define KML_DMAX 64                    // samples (sorted-member lists hold a sample index in six bits)
#define KML_VMAX 1024                  // features (KmlDiv's exactness, the pairwise-sum stack)
#define KML_CLASSES 6
// dynamic LDS of the classes (bytes).  With the body's 6.5 KB of static LDS: 8 / 6 / 4 / 3 / 2 / 1 workgroups per CU (160 KB of LDS; 8 is
// also what 128 VGPRs x 2 waves allow).  The last two classes take the handful of fits of k = 8..10 on several dozen sequences: a
// workgroup or two per CU still beat the general form's trips to its workspace (their launches are a fit's latency long).
#define KML_C0 13824
#define KML_C1 20480
#define KML_C2 34304
#define KML_C3 47872
#define KML_C4 75264
#define KML_C5 131072
#define KML_HD __host__ __device__ inline                 // (the class rule runs on the host too: mprg_kmeans_lds_class)
struct KmlLayout {
  int means, counts, lb, dist, ub, chd, lab, labo, ord, clist;   // Elkan stage (byte offsets into the dynamic pool)
  int uni, pool, g1, g4;                                  // seeding stage (before the counts are staged: the same bytes)
  int bestc, pdist;                                       // best restart + predict (after the restarts: over lb ..)
  int need, need_tables;                                  // bytes without / with the sample-sample tables in LDS
  int ordp;                                               // pitch of a restart's sorted-member list (bytes)
};
KML_HD int kml_up16(long long x) { return (int)((x + 15) & ~15LL); }
KML_HD int kml_xl_pitch(int V) { int p = (V + 3) & ~3; if (((p >> 2) & 1) == 0) p += 4; return p; }
// keep: the seeding's rows go BEHIND the counts instead of over them — the fused loop stages a problem's counts once for all its rounds
KML_HD KmlLayout kml_layout(int D, int V, int k, int NR, bool keep = false) {
  KmlLayout L;
  const int T = k < 3 ? 2 : (k < 8 ? 3 : 4), nu = 1 + (k - 1) * T;
  L.means = 0;
  L.counts = 8 * ((V + 1) & ~1);
  const int e0 = kml_up16((long long)L.counts + (long long)D * kml_xl_pitch(V));
  L.lb = e0;
  L.dist = L.lb + 8 * NR * D * k;
  L.ub = L.dist + 8 * NR * D * k;
  L.chd = L.ub + 8 * NR * D;
  L.lab = L.chd + 8 * NR * k * k;
  L.labo = L.lab + kml_up16(NR * D);
  L.ordp = (D + 7) & ~7;
  L.ord = L.labo + kml_up16(NR * D);
  L.clist = L.ord + kml_up16(NR * L.ordp);               // the pairs that need a distance, listed PER CENTRE: (restart, centre) -> up to D samples
  const int elkan_end = L.clist + kml_up16(NR * k * D);
  L.bestc = e0;
  L.pdist = L.bestc + 8 * k * V;
  const int predict_end = kml_up16(L.pdist + 8 * D * k);
  L.uni = keep ? e0 : 0;
  L.pool = L.uni + 8 * NR * nu;
  L.g1 = L.pool + 8 * NR * 5 * D;
  L.g4 = L.g1 + 8 * D * D;
  const int seed_end = L.g1, seed_end_tables = L.g4 + 8 * D * D;
  int need = elkan_end > predict_end ? elkan_end : predict_end;
  if (seed_end > need) need = seed_end;
  L.need = need;
  L.need_tables = seed_end_tables > need ? seed_end_tables : need;
  return L;
}
KML_HD int kml_class_bytes(int c) { return c == 0 ? KML_C0 : (c == 1 ? KML_C1 : (c == 2 ? KML_C2 : (c == 3 ? KML_C3 : (c == 4 ? KML_C4 : KML_C5)))); }
// the class of a fit: the smallest whose dynamic LDS holds it; -1: the fit takes one of the other forms
KML_HD int kml_class(long long D, long long V, int k, int n_init, bool keep = false) {
  if (k < 2 || k > 10 || n_init < 1 || n_init > KML_RMAX || D < 2 || D > KML_DMAX || V < 1 || V > KML_VMAX) return -1;
  const KmlLayout L = kml_layout((int)D, (int)V, k, n_init, keep);
  for (int c = 0; c < KML_CLASSES; ++c) if (L.need <= kml_class_bytes(c)) return c;
  return -1;
}

// The class of a fit of a PREPARED problem (ws: the problem's workspace; nullptr: not looked at).  The body reads K6's sample-sample
// tables (g1 / g4 / gv / ge): a problem that mprg_kmeans_prepare_big prepared WITHOUT them (scal[2] of its workspace; a level of big
// problems beyond forest.KM_NO_TABLES_BYTES) has no class — it is the general / wide forms' whatever its k.  Every place that sorts
// fits into forms asks through this function (k_kl_advance, k_kl_speculate, the fused loops).
MPRG_DEV int kml_class_ws(long long D, long long V, int k, int n_init, bool keep, const double *ws) {
  const int c = kml_class(D, V, k, n_init, keep);
  if (c >= 0 && ws && ws[D * V + 2 * V + D + 2] == 1.0) return -1;          // (km_ws: Xc[D V] mean[V] tmpV[V] xsq[D] scal[8])
  return c;
}

// n / d for 0 <= n with n * d < 2^32, d >= 1: one multiplication (m = floor(2^32 / d) + 1)
struct KmlDiv {
  unsigned d, m;
  MPRG_DEVM void init(int d_) { d = (unsigned)d_; m = d_ > 1 ? (unsigned)(0x100000000ULL / (unsigned long long)d_) + 1u : 0u; }
  MPRG_DEVM int div(int n) const { return d > 1 ? (int)(((unsigned long long)(unsigned)n * m) >> 32) : n; }
};
#define KML_FOR(i, n) for (int i = MPRG_TID; i < (int)(n); i += N_THREADS)
// km_gemv_col(v, 1, nullptr, m, j, n) — a column sum in dgemv_t order, x = ones — for m < 2048 (one block of the kernel): four (or, for
// the two columns the 2-column micro-kernel takes, two) interleaved running sums over the first m & ~3 elements, then the tail.  The same
// additions in the same order as KmOnesSum / km_gemv_col, without the per-element bookkeeping.
MPRG_DEV double kml_ones_sum(const double *v, int m, int j, int n) {
  const int n1 = n & ~3, main_end = m & -4, m3 = m & 3;
  const bool two = !(j < n1) && (n & 2) && j < n1 + 2;
  double y = 0;
  if (main_end) {
    double l0 = 0, l1 = 0, l2 = 0, l3 = 0;
    if (two) { for (int i = 0; i < main_end; i += 4) { l0 = l0 + v[i]; l1 = l1 + v[i + 1]; l0 = l0 + v[i + 2]; l1 = l1 + v[i + 3]; } }
    else for (int i = 0; i < main_end; i += 4) { l0 = l0 + v[i]; l1 = l1 + v[i + 1]; l2 = l2 + v[i + 2]; l3 = l3 + v[i + 3]; }
    y = y + (two ? l0 + l1 : (l0 + l2) + (l1 + l3));
  }
  if (m3 == 3) return y + (v[main_end + 2] + (v[main_end] + v[main_end + 1]));
  if (m3 == 2) return y + (v[main_end] + v[main_end + 1]);
  if (m3 == 1) return y + v[main_end];
  return y;
}

// ---- the chains that walk CENTRE rows (global memory) with SIXTEEN operands per round trip: a chain of V operands is V / 16 dependent
// trips to L2 instead of V / 8 — these phases (centre-centre distances, shifts, sample-centre distances, inertia) wait for trips, their
// arithmetic and its order are those of km_chain / km_syrk_dot / km_euclid / km_euclid_xl
MPRG_DEV double kml_chain16(const double *a, const double *b, int k0, int k1) {
  double s = 0;
  int k = k0;
  for (; k + 16 <= k1; k += 16) {
    double x[16], y[16];
#pragma unroll
    for (int q = 0; q < 16; q++) { x[q] = a[k + q]; y[q] = b[k + q]; }
#pragma unroll
    for (int q = 0; q < 16; q++) s = FMA(x[q], y[q], s);
  }
  for (; k + 8 <= k1; k += 8) {
    double x[8], y[8];
#pragma unroll
    for (int q = 0; q < 8; q++) { x[q] = a[k + q]; y[q] = b[k + q]; }
#pragma unroll
    for (int q = 0; q < 8; q++) s = FMA(x[q], y[q], s);
  }
  for (; k < k1; k++) s = FMA(a[k], b[k], s);
  return s;
}
MPRG_DEV double kml_syrk_dot16(const double *a, const double *b, int K) {
  double c = 0;
  for (int ls = 0; ls < K;) {
    int min_l = K - ls;
    if (min_l >= 512) min_l = 256;
    else if (min_l > 256) min_l = (min_l + 1) / 2;
    c = c + kml_chain16(a, b, ls, ls + min_l);
    ls += min_l;
  }
  return c;
}
MPRG_DEV double kml_euclid16(const double *a, const double *b, int nf, bool squared) {
  const int n = nf / 4, rem = nf % 4;
  double result = 0;
  int i = 0;
  for (; i + 4 <= n; i += 4) {                           // 16 features: operands first, then the ordered partial sums
    double x[16], y[16];
#pragma unroll
    for (int q = 0; q < 16; q++) { x[q] = a[4 * i + q]; y[q] = b[4 * i + q]; }
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const double d0 = x[4 * g] - y[4 * g], d1 = x[4 * g + 1] - y[4 * g + 1], d2 = x[4 * g + 2] - y[4 * g + 2], d3 = x[4 * g + 3] - y[4 * g + 3];
      result += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
  }
  for (; i < n; i++) {
    const double d0 = a[4 * i] - b[4 * i], d1 = a[4 * i + 1] - b[4 * i + 1], d2 = a[4 * i + 2] - b[4 * i + 2], d3 = a[4 * i + 3] - b[4 * i + 3];
    result += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
  }
  for (int q = 0; q < rem; q++) { const double t = a[4 * n + q] - b[4 * n + q]; result += t * t; }
  return squared ? result : sqrt(result);
}
// One walk of a NEW centre row for both things the iteration wants of it: how far the centre moved (kml_euclid16 against the old row:
// groups of four squared differences) and its squared norm (km_einsum_sq: blocks of eight, two running sums, pairs (6,7) (4,5) (2,3) (0,1)
// of a block in that order) — the row's operands are fetched once, sixteen per trip, and each result sees its own operations in its own order.
MPRG_DEV double kml_shift_norm16(const double *a, const double *b, int nf, double *norm_out) {
  double result = 0, l0 = 0, l1 = 0;
  int f = 0;
  for (; f + 16 <= nf; f += 16) {
    double x[16], y[16];
#pragma unroll
    for (int q = 0; q < 16; q++) { x[q] = a[f + q]; y[q] = b[f + q]; }
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const double d0 = x[4 * g] - y[4 * g], d1 = x[4 * g + 1] - y[4 * g + 1], d2 = x[4 * g + 2] - y[4 * g + 2], d3 = x[4 * g + 3] - y[4 * g + 3];
      result += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
#pragma unroll
    for (int blk = 0; blk < 2; blk++)
#pragma unroll
      for (int v = 3; v >= 0; v--) {
        const double x0 = x[8 * blk + 2 * v], x1 = x[8 * blk + 2 * v + 1];
        l0 = x0 * x0 + l0; l1 = x1 * x1 + l1;
      }
  }
  {                                                      // the distance's last groups of four and single features
    int i = f;
    for (; i + 4 <= nf; i += 4) {
      const double d0 = a[i] - b[i], d1 = a[i + 1] - b[i + 1], d2 = a[i + 2] - b[i + 2], d3 = a[i + 3] - b[i + 3];
      result += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
    for (; i < nf; i++) { const double t = a[i] - b[i]; result += t * t; }
  }
  {                                                      // the norm's last block of eight, then pairs
    int i = f;
    for (; nf - i >= 8; i += 8)
      for (int v = 3; v >= 0; v--) {
        const double x0 = a[i + 2 * v], x1 = a[i + 2 * v + 1];
        l0 = x0 * x0 + l0; l1 = x1 * x1 + l1;
      }
    for (; i < nf; i += 2) {
      const double x0 = a[i];
      l0 = x0 * x0 + l0;
      if (i + 1 < nf) { const double x1 = a[i + 1]; l1 = x1 * x1 + l1; }
    }
  }
  *norm_out = l0 + l1;
  return sqrt(result);
}
// km_euclid_xl with sixteen features per trip (four LDS words of the sample, sixteen doubles of the centre and of the means)
MPRG_DEV double kml_euclid_xl16(const uint8_t *x0, const double *mean_s, const double *b, int nf, bool squared) {
  const int n = nf / 4, rem = nf % 4;
  double r0 = 0;
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    double y[16], m[16];
    uint32_t u0[4];
#pragma unroll
    for (int q = 0; q < 16; q++) y[q] = b[4 * i + q];
#pragma unroll
    for (int q = 0; q < 4; q++) u0[q] = *(const uint32_t *)(x0 + 4 * (i + q));
#pragma unroll
    for (int q = 0; q < 16; q++) m[q] = mean_s[4 * i + q];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const double d0 = km_xl_value(u0[g], 0, m[4 * g]) - y[4 * g], d1 = km_xl_value(u0[g], 1, m[4 * g + 1]) - y[4 * g + 1],
                   d2 = km_xl_value(u0[g], 2, m[4 * g + 2]) - y[4 * g + 2], d3 = km_xl_value(u0[g], 3, m[4 * g + 3]) - y[4 * g + 3];
      r0 += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
  }
  for (; i < n; i++) {
    const uint32_t u0 = *(const uint32_t *)(x0 + 4 * i);
    double y[4], m[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { y[q] = b[4 * i + q]; m[q] = mean_s[4 * i + q]; }
    const double d0 = km_xl_value(u0, 0, m[0]) - y[0], d1 = km_xl_value(u0, 1, m[1]) - y[1], d2 = km_xl_value(u0, 2, m[2]) - y[2],
                 d3 = km_xl_value(u0, 3, m[3]) - y[3];
    r0 += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
  }
  for (int q = 0; q < rem; q++) {
    const int f = 4 * n + q;
    const double t = ((double)x0[f] - mean_s[f]) - b[f];
    r0 += t * t;
  }
  return squared ? r0 : sqrt(r0);
}

// the body: restarts (k-means++ + Elkan) of one fit side by side, best restart, predict.  pool: the kernel's dynamic LDS
// (lds_bytes of it, the class's size).
MPRG_DEV void kml_fit_body(const int fit, const int64_t *prob_all, const int32_t *kinfo, const int n_init, const double *uniforms_all,
                           const double *xcounts, double *ws_all, int32_t *labels_all, double *km_info, int32_t *km_status,
                           uint8_t *pool, const int lds_bytes_flags) {
  KM_T0();
  // (bits 24.. of the size word: 1: the centred rows from the workspace instead of the counts as bytes in LDS (MPRG_KML_FLAGS, tuning);
  //  2: the fused loop's layout — the seeding's rows behind the counts; 4: the counts and means are already there, staged by an
  //  earlier round of the same problem)
  const int lds_bytes = lds_bytes_flags & 0xffffff, kml_flags = lds_bytes_flags >> 24;
  const bool keep = (kml_flags & 2) != 0, staged = (kml_flags & 4) != 0;
  const int32_t *KI = kinfo + 5 * (long long)fit;
  const int pidx = KI[0], k = KI[1], rbase = KI[2];
  const int T = k < 3 ? 2 : (k < 8 ? 3 : 4);              // 2 + int(ln k) for k = 2..10 (_kmeans.py:209)
  const int64_t *P = prob_all + (long long)pidx * PF;
  const int D = (int)P[1], V = (int)P[7], NR = n_init;
  double *const ws = ws_all + P[9];
  const KmWs G = km_ws(ws, D, V, 0);                      // the problem's read-only part (K6)
  const double *X = G.Xc;
  const int nu = 1 + (k - 1) * T;
  const double *uniforms = uniforms_all + KI[3];
  const KmlLayout L = kml_layout(D, V, k, NR, keep);
  // a fit outside the class rule, or beyond this launch's pool (a host that filed it in the wrong list): an error, and no LDS touched —
  // the arrays below are sized for D <= KML_DMAX and the pool for lds_bytes (uniform across the workgroup: the early return is safe)
  if (kml_class(D, V, k, NR, keep) < 0 || L.need > lds_bytes) {
    ONE_THREAD { ATOMIC_OR(km_status + fit, (int32_t)MPRG_KM_UNSUPPORTED); }
    return;
  }
  const bool tables = L.need_tables <= lds_bytes;         // g1 / g4 of K6 in LDS for the seeding
  const int VP = km_xl_pitch(V), Dk = D * k, kk = k * k;
  KmlDiv dvD, dvK, dvV, dvDk, dvT;
  dvD.init(D); dvK.init(k); dvV.init(V); dvDk.init(Dk); dvT.init(T);
  // per-restart control words: 0..3 candidates, 5 stop code, 6 strict, 7 iterations, 8 buffer parity, 9 flags, 10 argmax cluster,
  // 11 a label changed in the last E-step, 12 an empty cluster needs the slow M-step path, 13 sits the iteration out, 14 runs a
  // full iteration (k_kmeans.inc: km_restarts_body)
  SHARED(int, shi, KML_RMAX * 16);
  SHARED(int, cidx, KML_RMAX * KM_KMAX);                  // k-means++: sample chosen as centre c of restart r
  SHARED(int, cnt_s, KML_RMAX * KM_KMAX);                 // cluster sizes after the E-step
  SHARED(double, pot_s, KML_RMAX * 4);                    // k-means++: potentials of the scored candidates
  SHARED(double, xsq_s, KML_DMAX);                        // row norms of the samples
  SHARED(double, csq_s, KML_RMAX * KM_KMAX);              // norms of the current centres
  SHARED(double, csh_s, KML_RMAX * KM_KMAX);              // how far each centre moved
  SHARED(double, res_s, KML_RMAX * 2);                    // inertia, iterations of every restart
  SHARED(double, inv_s, KML_RMAX * KM_KMAX);              // 1 / cluster size after the E-step (the M-step's means)
  SHARED(int, cn_s, KML_RMAX * KM_KMAX + 1);              // pairs listed per (restart, centre); afterwards their exclusive prefix sums
  SHARED(double, tol_s, 1);                               // the problem's tolerance (K6): read by the stop test
  SHARED(int, ctl, 8);                                    // 0 any_active 1 any_slow 2 need_n 3 live_n 4 act_n 5 xl_ok 6 best restart 7 labels seen
  SHARED(int, live_s, KML_RMAX);                          // restarts that run a full iteration ...
  SHARED(int, live2_s, KML_RMAX);                         // ... and of those, the ones whose E-step moved a label (M-step, shifts, bounds)
  SHARED(int, act_s, KML_RMAX);                           // restarts that are not done
  __shared__ KmPwStack pw_s[1];                           // relocation only
#define SHI(r, q) shi[(r) * 16 + (q)]
  double *const lb_s = (double *)(pool + L.lb), *const dist_s = (double *)(pool + L.dist), *const ub_s = (double *)(pool + L.ub);
  double *const chd_s = (double *)(pool + L.chd);
  uint8_t *const lab_s = pool + L.lab, *const labo_s = pool + L.labo, *const ord_s = pool + L.ord, *const clist_s = pool + L.clist;
  double *const mean_s = (double *)(pool + L.means);
  uint8_t *const xs = pool + L.counts;
  double *const uni_s = (double *)(pool + L.uni), *const seed_s = (double *)(pool + L.pool);
  double *const g1_s = (double *)(pool + L.g1), *const g4_s = (double *)(pool + L.g4);
#define CHD(r) (chd_s + (r) * kk)
#define CUR(w, r) (SHI(r, 8) ? (w).cB : (w).cA)
#define NXT(w, r) (SHI(r, 8) ? (w).cA : (w).cB)
  // centre j of restart r as the current iteration sees it: a sample row while the k-means++ centres are current (phase <= 1)
#define CROW(w, r, j) (phase <= 1 ? X + (long long)cidx[(r) * KM_KMAX + (j)] * V : CUR(w, r) + (long long)(j) * V)
#define WSR(r) km_ws(ws, D, V, rbase + (r))
  // ---------------- stage the seeding's inputs: uniforms, row norms, tables
  KML_FOR(e, NR * nu) { uni_s[e] = uniforms[e]; }
  KML_FOR(i, D) { xsq_s[i] = G.xsq[i]; }
  if (tables) { KML_FOR(e, D * D) { g1_s[e] = G.g1[e]; g4_s[e] = G.g4[e]; } }
  // ---------------- k-means++ (_kmeans.py:174-272; k_kmeans.inc: km_seed) — all restarts side by side
  // first centre of every restart: random_state.choice(n, p=uniform) = bisection of cumsum(p)/last (_kmeans.py:216-224)
  KML_FOR(r, NR) {
    const double uu = uniforms[r * nu];
    const double pval = 1.0 / (double)D;
    double c = 0;
    for (int i = 0; i < D; i++) c += pval;
    const double last = c;
    int c0 = 0;
    c = 0;
    for (int i = 0; i < D; i++) { c += pval; c0 += (c / last <= uu) ? 1 : 0; }   // searchsorted(cdf, uu, side="right")
    c0 = c0 > D - 1 ? D - 1 : c0;
    cidx[r * KM_KMAX] = c0;
    SHI(r, 5) = 0; SHI(r, 6) = 0; SHI(r, 7) = 0; SHI(r, 8) = 0; SHI(r, 9) = 0; SHI(r, 11) = 0; SHI(r, 12) = 0; SHI(r, 13) = 0; SHI(r, 14) = 1;
  }
  if (!staged) { ONE_THREAD { ctl[5] = 1; } }
  ONE_THREAD { tol_s[0] = G.scal[0]; }
  BARRIER();
#define SEED_CLOSEST(r) (seed_s + (r) * 5 * D)
#define SEED_CAND(r) (seed_s + (r) * 5 * D + D)
  KML_FOR(e, NR * D) {                  // euclidean_distances(centers[0], X, squared) (_kmeans.py:224): gv[c0][j]
    const int r = dvD.div(e), j = e - r * D;
    const int c0 = cidx[r * KM_KMAX];
    double dd = -2 * G.gv[(long long)c0 * D + j];
    dd += xsq_s[c0]; dd += xsq_s[j];
    SEED_CLOSEST(r)[j] = dd > 0 ? dd : 0;
  }
  BARRIER(); KM_T(10);
  for (int ci = 1; ci <= k; ci++) {     // round ci settles centre ci-1 and (ci < k) draws and scores candidates for centre ci
    KML_FOR(r, NR) {
      double *closest = SEED_CLOSEST(r), *cands = SEED_CAND(r);
      const double *u = uni_s + r * nu;
      double pot = 0;
      const double *src = closest;
      if (ci == 1) {                     // potential of the first centre: the distances summed in dgemv order
        pot = kml_ones_sum(closest, D, 0, 1);
      } else {                           // best of the T candidates scored in the previous round (_kmeans.py:253-263)
        int best = 0;
        pot = pot_s[r * 4];
#pragma unroll
        for (int t = 1; t < 4; t++) if (t < T) { const double p = pot_s[r * 4 + t]; if (p < pot) { pot = p; best = t; } }
        cidx[r * KM_KMAX + ci - 1] = SHI(r, best);
        src = cands + best * D;
      }
      if (ci < k) {                      // candidates for centre ci (_kmeans.py:240-242): searchsorted(cumsum, rand * pot)
        double rv[4]; int idx[4];
#pragma unroll
        for (int t = 0; t < 4; t++) { rv[t] = t < T ? u[1 + (ci - 1) * T + t] * pot : 0; idx[t] = 0; }
        double sum = 0;
        for (int j0 = 0; j0 < D; j0 += 8) {
          double v[8];
#pragma unroll
          for (int q = 0; q < 8; q++) if (j0 + q < D) v[q] = src[j0 + q];
#pragma unroll
          for (int q = 0; q < 8; q++) if (j0 + q < D) {
            if (ci > 1) closest[j0 + q] = v[q];
            sum += 1.0 * v[q];
#pragma unroll
            for (int t = 0; t < 4; t++) idx[t] += (sum < rv[t]) ? 1 : 0;
          }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) if (t < T) SHI(r, t) = idx[t] > D - 1 ? D - 1 : idx[t];
      }
    }
    BARRIER(); KM_T(0);
    if (ci == k) break;
    // scoring: one element of min(closest, distance to the candidate) per thread (restart x candidate x sample) ...
    KML_FOR(e, NR * T * D) {
      const int rt = dvD.div(e), j = e - rt * D;
      const int r = dvT.div(rt), t = rt - r * T;
      const int cand = SHI(r, t);
      // element (t, j) of euclidean_distances(X[candidates], X): the tables are symmetric, row `cand` is contiguous
      const int j4 = (T & 1) && t == T - 1 ? (D & ~3) : 0;      // km_gemm_use4(j, D, t, T) <=> j < j4
      double dd;
      if (tables) dd = -2 * (j < j4 ? g4_s : g1_s)[cand * D + j];
      else dd = -2 * (j < j4 ? G.g4 : G.g1)[(long long)cand * D + j];
      dd += xsq_s[cand]; dd += xsq_s[j];
      dd = dd > 0 ? dd : 0;
      const double cl = SEED_CLOSEST(r)[j];
      SEED_CAND(r)[t * D + j] = cl < dd ? cl : dd;
    }
    BARRIER();
    KML_FOR(e, NR * T) {                // ... then the candidate's potential: those elements summed in dgemv order
      const int r = dvT.div(e), t = e - r * T;
      pot_s[r * 4 + t] = kml_ones_sum(SEED_CAND(r) + t * D, D, t, T);
    }
    // (no workgroup barrier here: the potentials are written and — by the next round's pick — read by lanes of the first wavefront only,
    //  NR T <= 40 of them; the other wavefronts wait at the pick's barrier)
    if (wave_id() == 0) WAVE_SYNC();
    KM_T(1);
  }
#undef SEED_CLOSEST
#undef SEED_CAND
  // ---------------- the fit's counts into LDS as bytes + the feature means (the seeding's rows are dead: km_seed ended on a barrier)
  if (!staged) {
    const double *Xraw = xcounts + P[8];
    const int VW = VP >> 2;
    KmlDiv dvW; dvW.init(VW);
    // one LDS word = 4 features of one sample; the counts of up to KML_STAGE words per thread are fetched before any is used (a thread's
    // words were a trip to memory each: a median fit has three per thread)
#ifndef KML_STAGE
#define KML_STAGE 4
#endif
    for (int e0 = MPRG_TID; e0 < D * VW; e0 += KML_STAGE * N_THREADS) {
      double c[KML_STAGE][4];
#pragma unroll
      for (int u = 0; u < KML_STAGE; u++) {
        const int e = e0 + u * N_THREADS;
        if (e < D * VW) {
          const int i = dvW.div(e), f0 = 4 * (e - i * VW);
#pragma unroll
          for (int q = 0; q < 4; q++) c[u][q] = f0 + q < V ? Xraw[(long long)i * V + f0 + q] : 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < KML_STAGE; u++) {
        const int e = e0 + u * N_THREADS;
        if (e < D * VW) {
          const int i = dvW.div(e), f0 = 4 * (e - i * VW);
          uint32_t word = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (!(c[u][q] >= 0.0 && c[u][q] <= 255.0)) ctl[5] = 0;
            word |= ((uint32_t)c[u][q] & 255u) << (8 * q);
          }
          *(uint32_t *)(xs + i * VP + f0) = word;
        }
      }
    }
    KML_FOR(f, V) { mean_s[f] = G.mean[f]; }
  }
  KML_FOR(e, NR * k) {                  // ||centre||^2 of a centre that is a sample is that sample's (same order: einsum)
    const int r = dvK.div(e), j = e - r * k;
    csq_s[r * KM_KMAX + j] = xsq_s[cidx[r * KM_KMAX + j]];
  }
  BARRIER(); KM_T(11);
  const bool xl = ctl[5] != 0 && !(kml_flags & 1);          // every count fits a byte: the centred value is formed where it is used (k_kmeans.inc: XL form)
  // ---------------- Elkan (_kmeans.py:456-618, _k_means_elkan.pyx) — the phases of km_restarts_body, state in LDS
  // (the lists of the restarts that are not done / that run a full iteration: all of them now, afterwards what the stop test leaves)
  KML_FOR(r, NR) { act_s[r] = r; live_s[r] = r; }
  ONE_THREAD { ctl[4] = NR; ctl[3] = NR; }
  BARRIER();
  for (int phase = 0;; ++phase) {       // phase 0 = init_bounds, then iterations
    const int n_act = ctl[4], n_live = ctl[3];
    // centre-centre half distances (one item per pair i < j, pairs in row-major order: (0,1) .. (0,k-1), (1,2) ..).  An iteration does
    // not start with them: the table of the centres an iteration RUNS on is made where those centres are made — here for the first
    // centres (samples), and for every later set in the phase that walks the new rows anyway (shifts and norms, below) — so an
    // iteration has one chain phase along the centre rows less, and a barrier less.
    const int npairs = k * (k - 1) / 2;
    KmlDiv dvP; dvP.init(npairs);
#define KML_PAIR(e_, q0_, i_, j_) const int q0_ = dvP.div(e_); int p_ = (e_) - q0_ * npairs, i_ = 0;                                   \
      while (p_ >= k - 1 - i_) { p_ -= k - 1 - i_; ++i_; }                                                                            \
      const int j_ = i_ + 1 + p_
    if (phase == 0) {
      KML_FOR(c, KML_RMAX * KM_KMAX) { cnt_s[c] = 0; }       // cluster sizes (the E-step counts them)
      KML_FOR(c, NR * k + 1) { cn_s[c] = 0; }                // the per-centre pair counters of an iteration's list
      KML_FOR(e, NR * k) { const int r = dvK.div(e), q = e - r * k; CHD(r)[q * k + q] = 0; }          // the diagonal, once
      KML_FOR(e, NR * npairs) {
        KML_PAIR(e, r, i, j);
        // first centres are samples: for V <= 256 the syrk chain is the one-block chain K6 tabulated (g1)
        double dot;
        if (V <= 256) {
          const int ci_ = cidx[r * KM_KMAX + i], cj_ = cidx[r * KM_KMAX + j];
          dot = G.g1[(long long)ci_ * D + cj_];          // (from the workspace: the LDS copy of the seeding is gone, the counts took its place)
        } else dot = kml_syrk_dot16(X + (long long)cidx[r * KM_KMAX + i] * V, X + (long long)cidx[r * KM_KMAX + j] * V, V);
        double dd = -2 * dot; dd += csq_s[r * KM_KMAX + i]; dd += csq_s[r * KM_KMAX + j];
        dd = dd > 0 ? dd : 0; dd = sqrt(dd);
        CHD(r)[i * k + j] = dd / 2; CHD(r)[j * k + i] = dd / 2;
      }
      // init_bounds: the first centres are samples, so every sample-centre distance is one of D x D sample-sample distances (ge of K6)
      KML_FOR(e, NR * Dk) {
        const int r = dvDk.div(e), qq = e - r * Dk;
        const int j = dvD.div(qq), i = qq - j * D;
        const int cj = cidx[r * KM_KMAX + j];
        dist_s[r * Dk + i * k + j] = G.ge[(long long)cj * D + i];
      }
      ONE_THREAD { ctl[1] = 0; ctl[2] = 0; }
      BARRIER(); KM_T(2); KM_T(3);
      KML_FOR(e, NR * D) {               // init_bounds_dense (_k_means_elkan.pyx:24-97)
        const int r = dvD.div(e), i = e - r * D;
        const double *chd = CHD(r);
        const double *drow = dist_s + r * Dk + i * k;
        double *lrow = lb_s + r * Dk + i * k;
        double dr[KM_KMAX];
#pragma unroll
        for (int j = 0; j < KM_KMAX; j++) dr[j] = j < k ? drow[j] : 0;
        int best = 0; double mind = dr[0];
        lrow[0] = mind;
#pragma unroll
        for (int j = 1; j < KM_KMAX; j++) if (j < k) {
          double l = 0;                                       // lower_bounds starts as zeros (_kmeans.py:529)
          if (mind > chd[best * k + j]) {
            l = dr[j];
            if (l < mind) { mind = l; best = j; }
          }
          lrow[j] = l;
        }
        lab_s[r * D + i] = (uint8_t)best; ub_s[r * D + i] = mind; labo_s[r * D + i] = 255;
      }
      BARRIER(); KM_T(4);
      continue;
    }
    // (distance_next_center — np.partition(center_half_distances, kth=1, axis=0)[1], the second smallest of a column of the table — is
    //  formed by the threads that ask for it: k LDS reads, no phase and no barrier of its own)
    if (phase > 1 && xl) {
      // After the first iteration the bounds rule out most pairs.  The pairs that do need their distance are listed first, PER CENTRE
      // (restart, centre) -> its samples, in whatever order the lanes arrive: each result goes to its own place), and walked in list
      // order: full wavefronts whose neighbouring lanes read the SAME centre row — a load instruction of the walk touches the two or
      // three cache lines of the centres its 64 lanes span instead of one line per lane (25 lines per instruction before: the vector
      // L1's line rate was the kernel's nearest roof, profiles/r06/counters/).  A thread per SAMPLE lists: a sample whose upper bound
      // is within distance_next_center of its centre — the rule after an iteration or two — is skipped whole (the E-step does not
      // look at its distances either).  A centre's list holds at most D samples: nothing overflows.
      // (the counters were cleared before the barrier above)
      KML_FOR(e, n_act * D) {
        const int q0 = dvD.div(e), r = act_s[q0], i = e - q0 * D;
        const int lab = lab_s[r * D + i];
        const double up = ub_s[r * D + i];
        if (km_dnext(CHD(r), k, lab) >= up) continue;
        const double *lrow = lb_s + r * Dk + i * k;
        double *drow = dist_s + r * Dk + i * k;
        for (int j = 0; j < k; j++) {
          if (!(j == lab || up > lrow[j])) { drow[j] = NAN; continue; }
          const int slot = ATOMIC_ADD(cn_s + r * k + j, 1);
          clist_s[(r * k + j) * D + slot] = (uint8_t)i;
        }
      }
      BARRIER();
      // exclusive prefix sums of the NR k counts (pf_s[NR k] = the total) by EVERY wavefront for itself — the same values into the same
      // places (the centre shifts' array is free between the stop test and the next shifts) — instead of one wavefront and a barrier
      int *const pf_s = (int *)csh_s;
      {
        int run = 0;
        for (int c0 = 0; c0 < NR * k + 1; c0 += WAVE) {
          const int c = c0 + wave_lane();
          const int v = c < NR * k ? cn_s[c] : 0;
          const int incl = wave_scan_incl(v);
          if (c <= NR * k) pf_s[c] = run + incl - v;
          run += __shfl(incl, WAVE - 1);
        }
      }
      WAVE_SYNC();
      const int n_need = pf_s[NR * k];
#ifdef KML_DEBUG
      ONE_THREAD { printf("NEED D %d V %d k %d phase %d n_act %d pairs %d of %d\n", D, V, k, phase, n_act, n_need, n_act * D * k); }
#endif
      KML_FOR(t, n_need) {
        int lo = 0, hi = NR * k;            // the centre whose list holds item t: the last c with pf_s[c] <= t
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pf_s[mid] <= t) lo = mid; else hi = mid; }
        const int r = dvK.div(lo), j = lo - r * k, i = clist_s[lo * D + (t - pf_s[lo])];
        dist_s[r * Dk + i * k + j] = kml_euclid_xl16(xs + i * VP, mean_s, CUR(WSR(r), r) + (long long)j * V, V, false);
      }
    } else if (phase != 1) {            // counts beyond a byte: the centred rows from the workspace
      KML_FOR(e, n_act * Dk) {
        const int q0 = dvDk.div(e), r = act_s[q0], qq = e - q0 * Dk;
        const int j = dvD.div(qq), i = qq - j * D, q = i * k + j;
        const int lab = lab_s[r * D + i];
        const double up = ub_s[r * D + i];
        const bool need = (j == lab || up > lb_s[r * Dk + q]) && !(km_dnext(CHD(r), k, lab) >= up);
        dist_s[r * Dk + q] = need ? km_euclid(X + (long long)i * V, 1, CUR(WSR(r), r) + (long long)j * V, V, false) : NAN;
      }
    }
    BARRIER(); KM_T(3);
    KML_FOR(e, n_act * D) {              // _update_chunk_dense (_k_means_elkan.pyx:352-427), E-step
      const int q0 = dvD.div(e), r = act_s[q0], i = e - q0 * D;
      const double *chd = CHD(r);
      double upper = ub_s[r * D + i];
      int label = lab_s[r * D + i];
      const int old_label = labo_s[r * D + i];
      bool tight = false;
      if (!(km_dnext(chd, k, label) >= upper)) {
        double *lrow = lb_s + r * Dk + i * k;
        const double *drow = dist_s + r * Dk + i * k;
        double lbr[KM_KMAX], dr[KM_KMAX];
#pragma unroll
        for (int j = 0; j < KM_KMAX; j++) { lbr[j] = j < k ? lrow[j] : 0; dr[j] = j < k ? drow[j] : 0; }
#pragma unroll
        for (int j = 0; j < KM_KMAX; j++) if (j < k) {
          if (j != label && upper > lbr[j] && upper > chd[label * k + j]) {
            if (!tight) {
              upper = drow[label];
              if (upper != upper) upper = km_euclid(X + (long long)i * V, 1, CROW(WSR(r), r, label), V, false);
              lrow[label] = upper; tight = true;
            }
            if (upper > lbr[j] || upper > chd[label * k + j]) {
              double dd = dr[j];
              if (dd != dd) dd = km_euclid(X + (long long)i * V, 1, CROW(WSR(r), r, j), V, false);
              lrow[j] = dd;
              if (dd < upper) { label = j; upper = dd; }
            }
          }
        }
        lab_s[r * D + i] = (uint8_t)label; ub_s[r * D + i] = upper;
      }
      if (label != old_label) SHI(r, 11) = 1;             // some label moved in this E-step (read by the stop test)
      ATOMIC_ADD(cnt_s + r * KM_KMAX + label, 1);         // cluster sizes for the M-step
    }
    BARRIER();
    // A restart whose E-step moved no label has converged (np.array_equal(labels, labels_old), _kmeans.py:575) and sits the rest
    // of its iteration out (k_kmeans.inc).  Beside that: the restarts' samples sorted by cluster for the M-step — position of
    // sample i = members of smaller clusters + members of its own cluster before it; bit 7 marks a cluster's last member.
    if (wave_id() == 0) {                 // (a lane per running restart and a ballot: no thread walks the list alone)
      const int q = MPRG_TID;               // (= the lane: the first wavefront)
      const bool valid = q < n_live;
      const int r = valid ? live_s[q] : 0;
      const bool skip = valid ? (SHI(r, 11) == 0 && SHI(r, 9) == 0) : true;
      if (valid) SHI(r, 13) = skip;
      const unsigned long long m = __ballot(valid && !skip);
      if (valid && !skip) live2_s[__popcll(m & ((1ull << q) - 1ull))] = r;
      if (q == 0) ctl[3] = __popcll(m);
    }
    KML_FOR(e, n_live * D) {
      const int q0 = dvD.div(e), r = live_s[q0], i = e - q0 * D;
      const uint8_t *lr = lab_s + r * D;
      const int lab = lr[i];
      int pos = 0, before = 0;
      for (int j = 0; j < lab; j++) pos += cnt_s[r * KM_KMAX + j];
      for (int i2 = 0; i2 < i; i2++) before += lr[i2] == lab ? 1 : 0;
      ord_s[r * L.ordp + pos + before] = (uint8_t)(i | (before == cnt_s[r * KM_KMAX + lab] - 1 ? 0x80 : 0));
    }
    KML_FOR(e, n_live * k) {              // 1 / cluster size, once per cluster (_average_centers: alpha = 1.0 / weight_in_clusters[j])
      const int q0 = dvK.div(e), r = live_s[q0], j = e - q0 * k;
      const int c = cnt_s[r * KM_KMAX + j];
      inv_s[r * KM_KMAX + j] = c > 0 ? 1.0 / (double)c : 0.0;
    }
    BARRIER(); KM_T(4);
    const int n_live2 = ctl[3];
    // M-step (_k_means_elkan.pyx:296-313 + _average_centers, _k_means_common.pyx:274-295): a thread per (restart, FOUR features — one
    // LDS word of a sample's counts) walks the restart's samples cluster by cluster, each cluster's members in sample order: one
    // running sum per feature, the label / list reads shared by the four.  An empty cluster (rare): raw sums, slow path below.
    {
      const int VG = (V + 3) >> 2;
      KmlDiv dvG; dvG.init(VG);
      KML_FOR(e, n_live2 * VG) {
        const int q0 = dvG.div(e), r = live2_s[q0], f0 = 4 * (e - q0 * VG);
        const KmWs w = WSR(r);
        const int *cnt = cnt_s + r * KM_KMAX;
        bool empty = false;
        for (int j = 0; j < k; j++) empty = empty || cnt[j] == 0;
        double *out = NXT(w, r) + f0;
        const uint8_t *lr = lab_s + r * D;
        const int nf = V - f0 < 4 ? V - f0 : 4;
        double mf[4];
#pragma unroll
        for (int q = 0; q < 4; q++) mf[q] = (xl && q < nf) ? mean_s[f0 + q] : 0.0;
        if (empty) {
          for (int j = 0; j < k; j++)
            for (int q = 0; q < nf; q++) {
              double acc = 0;
              for (int i = 0; i < D; i++) if (lr[i] == j) acc = acc + (xl ? (double)xs[i * VP + f0 + q] - mf[q] : X[(long long)i * V + f0 + q]);
              out[(long long)j * V + q] = acc;
            }
          if (f0 == 0) {
            SHI(r, 12) = 1; ctl[1] = 1;
            for (int j = 0; j < k; j++) KM_WIC(w)[j] = (double)cnt[j];
          }
        } else {
          const uint8_t *ord = ord_s + r * L.ordp;
          const double *inv = inv_s + r * KM_KMAX;
          double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
          int j = 0;
          for (int m0 = 0; m0 < D; m0 += 8) {
            const uint64_t ow = *(const uint64_t *)(ord + m0);
            if (xl) {
              uint32_t xw[8];
#pragma unroll
              for (int q = 0; q < 8; q++) if (m0 + q < D) xw[q] = *(const uint32_t *)(xs + (int)((ow >> (8 * q)) & 63u) * VP + f0);
#pragma unroll
              for (int q = 0; q < 8; q++) if (m0 + q < D) {
                a0 = a0 + (km_xl_value(xw[q], 0, mf[0])); a1 = a1 + (km_xl_value(xw[q], 1, mf[1]));
                a2 = a2 + (km_xl_value(xw[q], 2, mf[2])); a3 = a3 + (km_xl_value(xw[q], 3, mf[3]));
                if ((ow >> (8 * q)) & 0x80u) {
                  const double al = inv[j];
                  double *o = out + (long long)j * V;
                  o[0] = a0 * al; if (nf > 1) o[1] = a1 * al; if (nf > 2) o[2] = a2 * al; if (nf > 3) o[3] = a3 * al;
                  a0 = a1 = a2 = a3 = 0; ++j;
                }
              }
            } else {
#pragma unroll
              for (int q = 0; q < 8; q++) if (m0 + q < D) {
                const double *xr = X + (long long)((ow >> (8 * q)) & 63u) * V + f0;
                a0 = a0 + xr[0]; if (nf > 1) a1 = a1 + xr[1]; if (nf > 2) a2 = a2 + xr[2]; if (nf > 3) a3 = a3 + xr[3];
                if ((ow >> (8 * q)) & 0x80u) {
                  const double al = inv[j];
                  double *o = out + (long long)j * V;
                  o[0] = a0 * al; if (nf > 1) o[1] = a1 * al; if (nf > 2) o[2] = a2 * al; if (nf > 3) o[3] = a3 * al;
                  a0 = a1 = a2 = a3 = 0; ++j;
                }
              }
            }
          }
        }
      }
    }
    BARRIER(); KM_T(5);
#ifdef KML_DEBUG
    ONE_THREAD {
      for (int q0 = 0; q0 < n_live2; q0++) {
        const int r = live2_s[q0];
        const KmWs w = WSR(r);
        printf("phase %d r %d cnt", phase, r); for (int j = 0; j < k; j++) printf(" %d", cnt_s[r * KM_KMAX + j]);
        printf(" lab"); for (int i = 0; i < D; i++) printf(" %d", lab_s[r * D + i]);
        printf(" ord"); for (int i = 0; i < D; i++) printf(" %d%s", ord_s[r * L.ordp + i] & 63, (ord_s[r * L.ordp + i] & 0x80) ? "*" : "");
        printf(" nxt"); for (int j = 0; j < k * V; j++) printf(" %g", NXT(w, r)[j]);
        printf("\n");
      }
    }
#endif
    if (ctl[1]) {                         // uniform over the workgroup: some restart has an empty cluster
      if (phase == 1) {                   // (rare) the relocation reads the current centres as a block: write the sample rows out now
        KML_FOR(e, NR * k * V) {
          const int r = e / (k * V), q = e % (k * V);
          if (!SHI(r, 12)) continue;
          CUR(WSR(r), r)[q] = X[(long long)cidx[r * KM_KMAX + q / V] * V + q % V];
        }
        BARRIER();
      }
      ONE_THREAD {
        for (int r = 0; r < NR; r++) {
          if (!SHI(r, 12)) continue;
          const KmWs w = WSR(r);
          double *wic = KM_WIC(w);
          const uint8_t *lr = lab_s + r * D;
          // _relocate_empty_clusters_dense (_k_means_common.pyx:167-211): a centre that lost all its samples moves to the
          // sample farthest from its own centre.  Rare (duplicate count vectors with small k-mer sizes); serial.
          int n_empty = 0;
          unsigned empty_mask = 0;
          for (int j = 0; j < k; j++) if (wic[j] == 0) { empty_mask |= 1u << j; ++n_empty; }
          if (n_empty > 0) {
            SHI(r, 9) |= 1;
            const double *cold = CUR(w, r);
            double *nx = NXT(w, r);
            double *dist = w.cum;                       // free during Elkan
            int32_t *perm = (int32_t *)w.tmpD;
            double dmax = 0;
            for (int i = 0; i < D; i++) {
              dist[i] = km_pairwise_sqdiff(X + (long long)i * V, 1, cold + (long long)lr[i] * V, V, pw_s);
              if (i == 0 || dist[i] > dmax) dmax = dist[i];
              perm[i] = i;
            }
            if (dmax != 0) {
              if (!km_argpartition(dist, perm, D, D - n_empty, (KmSelFrame *)pw_s)) SHI(r, 9) |= 2;
              for (int e = 0; e < n_empty; e++) {
                const int newc = __ffs(empty_mask) - 1;
                empty_mask &= empty_mask - 1;
                const int far = perm[D - 1 - e], oldc = lr[far];
                for (int f = 0; f < V; f++) {
                  const double xv = X[(long long)far * V + f] * 1.0;
                  nx[(long long)oldc * V + f] -= xv;
                  nx[(long long)newc * V + f] = xv;
                }
                wic[newc] = 1.0;
                wic[oldc] -= 1.0;
              }
            }
          }
          int am = 0;
          for (int j = 1; j < k; j++) if (wic[j] > wic[am]) am = j;
          SHI(r, 10) = am;
        }
      }
      BARRIER();
      // _average_centers walks the clusters in order: a still-empty cluster j takes the row of the biggest cluster as
      // it is at that moment — the raw sums if j comes before it, the mean if after.
      KML_FOR(e, NR * k * V) {
        const int r = e / (k * V), q = e % (k * V);
        if (!SHI(r, 12)) continue;
        const KmWs w = WSR(r);
        const int j = q / V, am = SHI(r, 10);
        if (!(KM_WIC(w)[j] > 0) && j < am) { double *nx = NXT(w, r); nx[q] = nx[(long long)am * V + q % V]; }
      }
      BARRIER();
      KML_FOR(e, NR * k * V) {
        const int r = e / (k * V), q = e % (k * V);
        if (!SHI(r, 12)) continue;
        const KmWs w = WSR(r);
        const double wj = KM_WIC(w)[q / V];
        if (wj > 0) { const double alpha = 1.0 / wj; NXT(w, r)[q] *= alpha; }
      }
      BARRIER();
      KML_FOR(e, NR * k * V) {
        const int r = e / (k * V), q = e % (k * V);
        if (!SHI(r, 12)) continue;
        const KmWs w = WSR(r);
        const int j = q / V, am = SHI(r, 10);
        if (!(KM_WIC(w)[j] > 0) && j > am) { double *nx = NXT(w, r); nx[q] = nx[(long long)am * V + q % V]; }
      }
      BARRIER(); KM_T(6);
    }
    // ONE phase for every chain along the NEW centre rows: how far each centre moved and its squared norm (one walk of the row, a lane
    // per (restart, centre), from the BACK of the workgroup) and the dot products of the next iteration's centre-centre table (a lane per
    // (restart, pair), from the front: two kinds of code, on different wavefronts where the items allow it).  The dots wait in the
    // table's upper triangle — the E-step that read the old table is over — until the norms are there (next phase).
    {
      const int n_sn = n_live2 * k, n_dot = n_live2 * npairs, tid = MPRG_TID;
      for (int e = N_THREADS - 1 - tid; e < n_sn; e += N_THREADS) {
        const int q0 = dvK.div(e), r = live2_s[q0], j = e - q0 * k;
        const KmWs w = WSR(r);
        double nrm;
        csh_s[r * KM_KMAX + j] = kml_shift_norm16(NXT(w, r) + (long long)j * V, CROW(w, r, j), V, &nrm);
        csq_s[r * KM_KMAX + j] = nrm;
      }
      for (int e = tid; e < n_dot; e += N_THREADS) {
        KML_PAIR(e, q0, i, j);
        const int r = live2_s[q0];
        const double *nx = NXT(WSR(r), r);
        CHD(r)[i * k + j] = kml_syrk_dot16(nx + (long long)i * V, nx + (long long)j * V, V);
      }
    }
    BARRIER(); KM_T(7);
    KML_FOR(e, n_live2 * npairs) {        // the table of the new centres from the dots and the norms
      KML_PAIR(e, q0, i, j);
      const int r = live2_s[q0];
      double dd = -2 * CHD(r)[i * k + j]; dd += csq_s[r * KM_KMAX + i]; dd += csq_s[r * KM_KMAX + j];
      dd = dd > 0 ? dd : 0; dd = sqrt(dd);
      CHD(r)[i * k + j] = dd / 2; CHD(r)[j * k + i] = dd / 2;
    }
    KML_FOR(c, NR * k + 1) { cn_s[c] = 0; }                // (the next iteration's list)
    ONE_THREAD { ctl[1] = 0; ctl[2] = 0; }                 // (the M-step's flags: read before the barrier above)
    KML_FOR(e, n_live2 * D) {
      const int q0 = dvD.div(e), r = live2_s[q0], i = e - q0 * D;
      const double *cshift = csh_s + r * KM_KMAX;
      const int lab = lab_s[r * D + i];
      double *lrow = lb_s + r * Dk + i * k;
      double lbr[KM_KMAX], cs[KM_KMAX];
#pragma unroll
      for (int j = 0; j < KM_KMAX; j++) { lbr[j] = j < k ? lrow[j] : 0; cs[j] = j < k ? cshift[j] : 0; }
      ub_s[r * D + i] += cshift[lab];
#pragma unroll
      for (int j = 0; j < KM_KMAX; j++) if (j < k) { double l = lbr[j] - cs[j]; if (l < 0) l = 0; lrow[j] = l; }
      labo_s[r * D + i] = (uint8_t)lab;
    }
    if (wave_id() == 0) {                 // the stop test (a lane per restart) and, from its answers, the next iteration's lists of restarts
      const int r = MPRG_TID;               // (= the lane, as a fresh copy: what is derived from it is not kept across the iteration)
      int st = 3;
      if (r < NR) {
        st = SHI(r, 5);
        if (st == 2) st = 3;                               // that was the final E-step of this restart
        else if (st != 3) {
          const double *cshift = csh_s + r * KM_KMAX;
          const bool same = SHI(r, 11) == 0;                   // np.array_equal(labels, labels_old), _kmeans.py:575
          SHI(r, 11) = 0; SHI(r, 12) = 0;
          int stop = 0, strict = 0;
          if (same) { stop = 1; strict = 1; }
          else {
            double sq[KM_KMAX];
#pragma unroll
            for (int j = 0; j < KM_KMAX; j++) sq[j] = j < k ? cshift[j] * cshift[j] : 0.0;
            if (km_sum_small(sq, k) <= tol_s[0]) stop = 1;
          }
          SHI(r, 7) += 1;
          if (!stop && SHI(r, 7) >= 300) stop = 1;
          SHI(r, 6) = strict;
          st = stop ? (strict ? 3 : 2) : 0;        // 3: done, 2: one more E-step on the new centres, 0: iterate
          if (!(SHI(r, 14) && SHI(r, 13))) SHI(r, 8) ^= 1;     // the new centres become the current ones (none were formed: see above)
        }
        SHI(r, 5) = st; SHI(r, 14) = st == 0;
        if (st != 3) for (int j = 0; j < k; j++) cnt_s[r * KM_KMAX + j] = 0;          // (its next E-step counts the cluster sizes anew; a finished restart keeps its last)
      }
      const unsigned long long m_act = __ballot(r < NR && st != 3), m_live = __ballot(r < NR && st == 0);
      const unsigned long long below = (1ull << r) - 1ull;
      if (r < NR && st != 3) act_s[__popcll(m_act & below)] = r;
      if (r < NR && st == 0) live_s[__popcll(m_live & below)] = r;
      if (r == 0) { ctl[4] = __popcll(m_act); ctl[3] = __popcll(m_live); ctl[0] = m_act != 0; }
    }
    BARRIER(); KM_T(8);
    if (!ctl[0]) break;
  }
  // inertia (_k_means_common.pyx:95-125): per-sample squared distances (into the free distance rows), summed in sample order.  The
  // samples are walked sorted by cluster (the lists of the M-step, rebuilt for the final labels of every restart — cnt_s holds each
  // restart's sizes from its last E-step): lanes that follow each other read the same centre row.
  KML_FOR(e, NR * D) {
    const int r = dvD.div(e), i = e - r * D;
    const uint8_t *lr = lab_s + r * D;
    const int lab = lr[i];
    int pos = 0, before = 0;
    for (int j = 0; j < lab; j++) pos += cnt_s[r * KM_KMAX + j];
    for (int i2 = 0; i2 < i; i2++) before += lr[i2] == lab ? 1 : 0;
    ord_s[r * L.ordp + pos + before] = (uint8_t)i;
  }
  BARRIER();
  KML_FOR(e, NR * D) {
    const int r = dvD.div(e), i = ord_s[r * L.ordp + (e - r * D)];
    const KmWs w = WSR(r);
    const double *cl = CUR(w, r) + (long long)lab_s[r * D + i] * V;
    dist_s[r * Dk + i] = xl ? kml_euclid_xl16(xs + i * VP, mean_s, cl, V, true) : km_euclid(X + (long long)i * V, 1, cl, V, true);
  }
  BARRIER(); KM_T(9);
  KML_FOR(r, NR) {
    double inertia = 0;
    for (int i = 0; i < D; i++) inertia += dist_s[r * Dk + i] * 1.0;
    res_s[2 * r] = inertia; res_s[2 * r + 1] = (double)SHI(r, 7);
    if (SHI(r, 9)) ATOMIC_OR(km_status + fit, (int32_t)SHI(r, 9));
  }
#ifdef KML_DEBUG
  ONE_THREAD { for (int r = 0; r < 2; r++) { const KmWs w = WSR(r); printf("r %d parity %d lab", r, SHI(r, 8)); for (int i = 0; i < D; i++) printf(" %d", lab_s[r * D + i]); printf(" cA"); for (int j = 0; j < k * V; j++) printf(" %g", w.cA[j]); printf(" cB"); for (int j = 0; j < k * V; j++) printf(" %g", w.cB[j]); printf(" d"); for (int i = 0; i < D; i++) printf(" %g", dist_s[r * Dk + i]); printf("\n"); } }
  ONE_THREAD { for (int r = 0; r < NR; r++) { printf("r %d inertia %a iters %d flags %d cidx", r, res_s[2 * r], SHI(r, 7), SHI(r, 9)); for (int j = 0; j < k; j++) printf(" %d", cidx[r * KM_KMAX + j]); printf("\n"); } }
#endif
  ONE_THREAD { ctl[7] = 0; }
  BARRIER();
  // ---------------- best restart (KMeans.fit, _kmeans.py:1500-1531): restarts in order; a later one wins only with a strictly
  // smaller inertia AND a different partition (up to relabelling) than the current best (_is_same_clustering)
  ONE_THREAD {
    int best = -1; double best_inertia = 0;
    for (int r = 0; r < NR; r++) {
      const double inertia = res_s[2 * r];
      bool take = best < 0;
      if (!take && inertia < best_inertia) {
        unsigned long long map = ~0ull;                    // six bits per label: the label it maps to (63: none yet)
        bool same = true;
        const uint8_t *la = lab_s + r * D, *lbb = lab_s + best * D;
        for (int i = 0; i < D && same; i++) {
          const int a = la[i], b = lbb[i];
          const int cur = (int)((map >> (6 * a)) & 63u);
          if (cur == 63) map = (map & ~(63ull << (6 * a))) | ((unsigned long long)b << (6 * a));
          else if (cur != b) same = false;
        }
        take = !same;
      }
      if (take) { best = r; best_inertia = inertia; }
    }
    ctl[6] = best;
  }
  BARRIER();
  // ---------------- predict (_k_means_lloyd.pyx:168-218) with the best restart's centres, in LDS over the restarts' state
  const int rb = ctl[6];
  {
    const KmWs wb = WSR(rb);
    const double *fin = SHI(rb, 8) ? wb.cB : wb.cA;
    double *bestc = (double *)(pool + L.bestc), *pdist = (double *)(pool + L.pdist);
    const double *gmean = xl ? mean_s : G.mean;
    KML_FOR(e, k * V) { const int j = dvV.div(e); bestc[e] = fin[e] + gmean[e - j * V]; }
    BARRIER();
    KML_FOR(j, k) { csq_s[j] = km_einsum_sq(bestc + j * V, 1, V); }
    BARRIER();
    const double *Xraw = xcounts + P[8];
    KML_FOR(e, Dk) {                    // one dgemm element per thread
      const int j = dvD.div(e), i = e - j * D;
      // (D <= 64 < 256: the chunk of _k_means_lloyd is the whole matrix)
      pdist[i * k + j] = xl ? km_gemm_dot<uint8_t>(bestc + j * V, 1, xs + i * VP, 1, V, j, k, i, D, csq_s[j], -2.0)
                            : km_gemm_dot<double>(bestc + j * V, 1, Xraw + (long long)i * V, 1, V, j, k, i, D, csq_s[j], -2.0);
    }
    BARRIER();
    int32_t *labels = labels_all + KI[4] + P[10];
    KML_FOR(i, D) {
      int label = 0; double mind = 0;
      for (int j = 0; j < k; j++) {
        const double dd = pdist[i * k + j];
        if (j == 0 || dd < mind) { mind = dd; label = j; }
      }
      labels[i] = label;
      atomicOr(&ctl[7], 1 << label);          // which labels occur (the loop reverts the round if fewer than k do)
    }
    BARRIER();
    ONE_THREAD {
      double tot_iter = 0;
      for (int r = 0; r < NR; r++) tot_iter += res_s[2 * r + 1];
      double *info = km_info + 8 * (long long)fit;
      info[0] = res_s[2 * rb]; info[1] = res_s[2 * rb + 1]; info[2] = (double)rb; info[3] = (double)__popc((unsigned)ctl[7]); info[4] = tot_iter;
    }
  }
#undef SHI
#undef CHD
#undef CUR
#undef NXT
#undef CROW
#undef WSR
#undef KML_PAIR
}

// one workgroup (64 .. 1 024 threads: the host picks by class — 128 / 128 / 256 / 256 / 512 / 1 024, so that the classes of two and one
// workgroups per CU still keep 16 wavefronts on it) per fit of the launch's list; lds_bytes = the class's dynamic LDS
__attribute__((amdgpu_flat_work_group_size(64, 1024), amdgpu_waves_per_eu(KM_WAVES, KM_WAVES))) __global__ void k_kmeans_fit_lds(
    const int64_t *prob_all, const int32_t *kinfo, const int32_t *fit_list, int n_init, const double *uniforms_all,
    const double *xcounts, double *ws_all, int32_t *labels_all, double *km_info, int32_t *km_status, int lds_bytes) {
  HIP_DYNAMIC_SHARED(uint8_t, pool)
  const int fit = fit_list ? fit_list[BLOCK_ID] : BLOCK_ID;
  if (kinfo[5 * (long long)fit + 1] == 0) return;          // k = 0: the device-side loop control has retired this problem (k_kl_advance)
  kml_fit_body(fit, prob_all, kinfo, n_init, uniforms_all, xcounts, ws_all, labels_all, km_info, km_status, pool, lds_bytes);
}
