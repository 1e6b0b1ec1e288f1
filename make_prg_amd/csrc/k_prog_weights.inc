// ---------------------------------------------------------------------------------------------------------------
// K-W  the leaf weights of `from_msa --unaligned --progressive --seq-weights` (make_prg_amd/from_msa/star_align.py holds the spec,
//      "Sequence weights"; DESIGN.md §3b).  Integers only.  A kernel of its own: the tree kernels and every other kernel stay what
//      they were.
//
// k_prog_leaf_weights: one workgroup per locus, over the tables mprg_prog_distances or mprg_prog_identities left and a merge list as
//   the tree entry points write it.  UPGMA's table update is not replayed: every pair of leaves adds to exactly one node, its lowest
//   common ancestor.
//   (1) One thread replays the merges, O(L): per slot the node its cluster is now and the tail of the cluster's list of leaves; a
//       merge (u, v) hangs v's list behind u's and writes the merge's index t at the joint.  The list of the last cluster is the
//       dendrogram order; between positions p and p + 1 stands the index of the merge that joined them.  Merge indices rise towards
//       the root, so the lowest common ancestor of the leaves at positions p < q is the LARGEST index on the joints p .. q - 1.
//   (2) A thread takes the rows p and L - 1 - p of the order (L - 1 pairs together, whatever p) and walks q upwards with the running
//       maximum of the joints; m_a m_b D(a, b) goes into a register, flushed by one 64-bit integer atomic when the node changes.
//       D is computed on the fly from `shared` and `nw` as the tree kernels compute it.  Integer sums are exact in any order.
//   (3) A thread per node: H_t = N_t / (|U| |V|).  (4) A thread per leaf walks its parents for c_a.  (5) The workgroup's maximum, q.
//   The per-slot and per-node state lives in the locus's workspace, LW_WS_WORDS(m) = 6 m int64 words: N (m int64), then nine int32
//   arrays of m.  LDS: a long long per wavefront and a flag.
// ---------------------------------------------------------------------------------------------------------------
#define LW_MAX_LEAVES TR_MAX_WEIGHT            // the spec's PROG_MAX_LEAVES
#define LW_MAX_SUM TRW_MAX_WEIGHT              // the spec's PROG_MAX_RECORDS: the largest multiplicity sum of a locus
#define LW_UNIT 256                            // the spec's 256: a weight's scale, and the largest q
#define LW_WS_WORDS(m) (6 * (m))               // the workspace need of a locus of m records, int64 words
#define LW_DEAD (-2)                           // at[x]: x is no live cluster's key (no leaf, or merged into another)
#define LW_LEAF (-1)                           // at[x]: the cluster of key x is the leaf x; a parent: none

__global__ void __launch_bounds__(PG_THREADS) k_prog_leaf_weights(const uint32_t *shared, long long shared_words, const int64_t *nw,
                                                                  const int64_t *seqs, long long n_seqs, const int64_t *loci,
                                                                  const int32_t *weights, int64_t *ws, long long ws_words,
                                                                  const int32_t *merges, long long merges_words, int32_t *heights,
                                                                  int64_t *raw, int32_t *q, int32_t *status) {
  SHARED(long long, red, PG_WAVES);
  SHARED(int, flag, 1);
  const int64_t *Lc = loci + MPRG_PG_TREE_FIELDS * (long long)BLOCK_ID;
  const long long first = Lc[0], m = Lc[1], toff = Lc[2], woff = Lc[3], moff = Lc[4];
  const bool ok = first >= 0 && m >= 1 && m <= 0x7fffffffLL && first <= n_seqs - m && toff >= 0 && toff <= shared_words &&
                  m <= (shared_words - toff) / m && moff >= 0 && moff <= merges_words && (moff & 1) == 0;
  ONE_THREAD flag[0] = 0;
  // the leaves (22 bits), their multiplicity sum (30 bits) and the multiplicities out of range (above them) in one workgroup sum:
  // a thread's counts are clamped just above the limits, so 256 of them stay inside their fields
  long long part = 0;
  if (ok) {
    long long leaves = 0, sum = 0, low = 0;
    PAR_FOR(x, m) {
      if (seqs[2 * (first + x) + 1] <= 0) continue;
      const long long w = weights ? weights[first + x] : 1;
      ++leaves;
      if (w < 1 || w > LW_MAX_SUM) low = 1; else sum += w;
    }
    part = (leaves < LW_MAX_LEAVES + 1 ? leaves : LW_MAX_LEAVES + 1) | (sum < LW_MAX_SUM + 1 ? sum : LW_MAX_SUM + 1) << 22 | low << 52;
  }
#include "wg_sum.inc"
  WG_TOTAL(total, PG_WAVES);                                 // (every thread: st stays workgroup-uniform)
  const long long L = total & 0x3fffff, wsum = (total >> 22) & 0x3fffffff;
  int st = MPRG_PG_OK;
  if (!ok || total >> 52 || wsum > LW_MAX_SUM || L > LW_MAX_LEAVES || (L >= 2 && 2 * (L - 1) > merges_words - moff)) st = MPRG_PG_BAD_ITEM;
  else if (woff < 0 || woff > ws_words || LW_WS_WORDS(m) > ws_words - woff) st = MPRG_PG_NO_SPACE;
  if (st != MPRG_PG_OK) {                                    // (the whole workgroup)
    ONE_THREAD status[BLOCK_ID] = st;
    return;
  }
  long long *N = (long long *)(ws + woff);                   // per node: the sum of m_a m_b D(a, b) over its two sides
  int32_t *at = (int32_t *)(ws + woff + m);                  // per slot: the node its cluster is now
  int32_t *tail = at + m, *nxt = tail + m, *jt = nxt + m;    // per slot: its cluster's last leaf; the leaf behind it, the joint's merge
  int32_t *lpar = jt + m;                                    // per slot: the leaf's parent node
  int32_t *ord = lpar + m, *bnd = ord + m;                   // per position: its leaf; the joint between it and the next
  int32_t *par = bnd + m, *nsz = par + m, *usz = nsz + m;    // per node: its parent, its multiplicity sum, its first child's
  const uint32_t *tab = shared + toff;
  const int64_t *nwl = nw + first, *seql = seqs + 2 * first;
  const int32_t *wl = weights ? weights + first : nullptr, *mg = merges + moff;
  int32_t *hts = heights + moff / 2;
  PAR_FOR(x, m) {
    at[x] = seql[2 * x + 1] > 0 ? LW_LEAF : LW_DEAD;
    tail[x] = (int32_t)x; nxt[x] = -1; jt[x] = 0; lpar[x] = LW_LEAF; N[x] = 0;
  }
  BARRIER();
  // (1) the merges replayed by one thread
  ONE_THREAD {
    int bad = 0;
    for (long long t = 0; t < L - 1; ++t) {
      const long long u = mg[2 * t], v = mg[2 * t + 1];
      if (u < 0 || v >= m || u >= v || at[u] == LW_DEAD || at[v] == LW_DEAD) { bad = 1; break; }
      const int a = at[u], b = at[v];
      const int su = a < 0 ? (wl ? wl[u] : 1) : nsz[a], sv = b < 0 ? (wl ? wl[v] : 1) : nsz[b];
      if (a < 0) lpar[u] = (int32_t)t; else par[a] = (int32_t)t;
      if (b < 0) lpar[v] = (int32_t)t; else par[b] = (int32_t)t;
      nsz[t] = su + sv; usz[t] = su; par[t] = LW_LEAF;
      at[u] = (int32_t)t; at[v] = LW_DEAD;
      const int e = tail[u];
      jt[e] = (int32_t)t; nxt[e] = (int32_t)v; tail[u] = tail[v];
    }
    if (!bad && L >= 2) {                                    // the last cluster's list, from its key: the dendrogram order
      long long p = 0;
      for (int x = mg[2 * (L - 2)]; x >= 0 && p < L; x = nxt[x], ++p) { ord[p] = x; bnd[p] = jt[x]; }
      bad = p != L;
    }
    if (bad) flag[0] = 1;
  }
  BARRIER();
  if (flag[0]) {                                             // (the whole workgroup)
    ONE_THREAD status[BLOCK_ID] = MPRG_PG_BAD_ITEM;
    return;
  }
  // (2) every pair of leaves into its lowest common ancestor
  int bad = 0;
  if (L >= 2) PAR_FOR(i, (L + 1) / 2) {
    for (int side = 0; side < 2; ++side) {
      const long long p = side ? L - 1 - i : i;
      if (side && p == i) break;
      const long long a = ord[p], wa = wl ? wl[a] : 1, na = nwl[a];
      if (na < 0) bad = 1;
      long long acc = 0;
      int node = -1;
      for (long long r = p + 1; r < L; ++r) {
        const int t = bnd[r - 1];
        if (t > node) {
          if (acc) ATOMIC_ADD((unsigned long long *)(N + node), (unsigned long long)acc);
          acc = 0; node = t;
        }
        const long long b = ord[r], wb = wl ? wl[b] : 1, nb = nwl[b], mn = na < nb ? na : nb;
        const long long lo = a < b ? a : b, hi = a < b ? b : a, s = tab[lo * m + hi];
        if (mn < 0 || (mn > 0 && s > mn)) bad = 1;
        else acc += wa * wb * (mn > 0 ? TR_SCALE - (TR_SCALE * s) / mn : TR_SCALE);
      }
      if (acc) ATOMIC_ADD((unsigned long long *)(N + node), (unsigned long long)acc);
    }
  }
  if (bad) ATOMIC_OR(&flag[0], 1);
  BARRIER();
  if (flag[0]) {                                             // (the whole workgroup)
    ONE_THREAD status[BLOCK_ID] = MPRG_PG_BAD_ITEM;
    return;
  }
  // (3) the heights; N as the atomics left it (read where they added: an atomic of 0)
  PAR_FOR(t, L - 1) {
    const long long sum = (long long)ATOMIC_ADD((unsigned long long *)(N + t), 0ull);
    hts[t] = (int32_t)(sum / ((long long)usz[t] * (nsz[t] - usz[t])));
  }
  BARRIER();
  // (4) a leaf's share of the edges above it
  part = 0;                                                  // (here: this thread's largest c_a)
  PAR_FOR(x, m) {
    long long c = 0;
    if (seql[2 * x + 1] > 0) {
      const long long wx = wl ? wl[x] : 1;
      long long below = 0, n = wx;
      for (int t = lpar[x]; t >= 0; t = par[t]) {
        const long long h = hts[t], len = h > below ? h - below : 0;
        c += (LW_UNIT * len * wx) / n;
        below = h; n = nsz[t];
      }
    }
    raw[first + x] = c;
    part = c > part ? c : part;
  }
  // (5) the largest, and q
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(part, d); part = o > part ? o : part; }
  if (wave_lane() == 0) red[wave_id()] = part;               // (everybody read red's sums before the barriers above)
  BARRIER();
  long long M = 0;
  for (int w = 0; w < PG_WAVES; ++w) M = red[w] > M ? red[w] : M;
  PAR_FOR(x, m) {
    const long long c = raw[first + x];                      // (this thread's own store)
    q[first + x] = seql[2 * x + 1] > 0 ? (int32_t)(M ? 1 + ((LW_UNIT - 1) * c) / M : 1) : 0;
  }
  ONE_THREAD status[BLOCK_ID] = MPRG_PG_OK;
}
