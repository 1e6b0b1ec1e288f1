// ---------------------------------------------------------------------------------------------------------------
// K-T  the guide tree of `from_msa --unaligned --progressive --device-tree` (make_prg_amd/from_msa/star_align.py holds the spec,
//      "Progressive": Tree, and "Collapse": the weighted form; DESIGN.md §3b, "Device tree").  Integers only.  A kernel of its own:
//      every kernel of k_prog.inc, k_prog_band.inc and k_collapse.inc stays what it was.
//
// k_prog_tree: one workgroup per locus, exact UPGMA over the locus's leaves (its records of length > 0), a slot per RECORD (a
//   record that is no leaf, and a cluster merged into another, has size 0).  S, the m x m int64 sums of w_a w_b D(a, b) between
//   the clusters (symmetric, both halves kept so that a row is read coalesced), lives in the locus's workspace; per slot the
//   cluster's size (weight sum), the row's best partner among the LATER keys and that partner's sum live in LDS up to TR_LDS_M
//   records (8 KB) and behind S in the workspace above (the same code, instantiated for either address space).
//   A merge step: (1) every row marked for a rescan is scanned by one wavefront (lanes on consecutive later keys, a wave
//   reduction); (2) a block reduction over the rows' best pairs names (U, V); (3) row and column U of S take row V's sums, and
//   thread x decides in O(1) what the merge means for row x: its best partner was U or V: marked for a rescan; x < U: the new
//   cluster U against the row's best; U < x: nothing (a row only looks at later keys).  Three barriers per merge.
//   Averages are compared by cross-multiplication in int64 (below 2^60: sums <= 65 536 |U| |V|, |U| + |V| <= 4 096); equal
//   averages go to the smaller key, in the rescan (the partner's key) as in the reduction (the row's key): the pair the plain
//   statement's strict "smaller" keeps while it walks (key(U), key(V)) in ascending order.
//   All averages equal: row a's best is the next live key, one row is rescanned per merge: O(m^2) in all.
// ---------------------------------------------------------------------------------------------------------------
#define TR_LDS_M 512                           // records whose per-slot state is kept in LDS
#define TR_MAX_WEIGHT 4096                     // the spec's PROG_MAX_LEAVES: the largest weight sum of a locus
#define TR_SCALE 65536                         // the spec's PROG_SCALE
#define TR_NONE (-1)                           // best partner: no live later key
#define TR_RESCAN (-2)                         // best partner: to be found again

// the average num / den of the pair named by idx (the partner's key within a row, the row's key among rows); idx < 0: none
struct TrCand { long long num; int den, idx; };
// what the block reduction hands every thread: the winning row u, its partner v, their sizes
struct TrPick { long long num; int den, u, v, su, sv; };

MPRG_DEV bool tr_less(const TrCand a, const TrCand b) {
  if (a.idx < 0) return false;
  if (b.idx < 0) return true;
  const long long l = a.num * b.den, r = b.num * a.den;
  return l < r || (l == r && a.idx < b.idx);
}

// the smallest candidate of the wavefront, in every lane (all 64 lanes call it)
MPRG_DEV TrCand tr_wave_min(TrCand c) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    TrCand o;
    o.num = __shfl_xor(c.num, d); o.den = __shfl_xor(c.den, d); o.idx = __shfl_xor(c.idx, d);
    if (tr_less(o, c)) c = o;
  }
  return c;
}

// The merges of a locus of L >= 2 leaves whose ranges have been checked; size, best, bsum: m slots each, in LDS or in global
// memory.  Returns false (nothing of `out` written) when a table entry breaks the bound the arithmetic relies on.
MPRG_DEV bool tr_build(int32_t *size, int32_t *best, long long *bsum, long long *S, const uint32_t *tab, const int64_t *nwl,
                       const int64_t *seql, const int32_t *wl, long long m, int L, int32_t *out, TrPick *red, int *flag) {
  const int lane = wave_lane(), wv = wave_id();
  PAR_FOR(x, m) {
    const bool leaf = seql[2 * x + 1] > 0;
    size[x] = leaf ? (wl ? wl[x] : 1) : 0;
    best[x] = leaf ? TR_RESCAN : TR_NONE;
  }
  BARRIER();
  // S[a][b] = w_a w_b D(a, b), D(a, b) = 65 536 - floor(65 536 s / min(nw_a, nw_b)), 65 536 when the minimum is 0
  int bad = 0;
  PAR_FOR(i, m * m) {
    const long long a = i / m, b = i - a * m;
    const long long wa = size[a], wb = size[b];
    long long v = 0;
    if (a != b && wa > 0 && wb > 0) {
      const long long lo = a < b ? a : b, hi = a < b ? b : a;
      const long long s = tab[lo * m + hi], na = nwl[a], nb = nwl[b], mn = na < nb ? na : nb;
      if (mn < 0 || (mn > 0 && s > mn)) bad = 1;
      else v = wa * wb * (mn > 0 ? TR_SCALE - (TR_SCALE * s) / mn : TR_SCALE);
    }
    S[i] = v;
  }
  if (bad) ATOMIC_OR(flag, 1);
  BARRIER();
  if (*flag) return false;                                   // (the whole workgroup)
  for (int k = 0; k < L - 1; ++k) {
    // (1) the rows marked for a rescan, a wavefront each: the best partner among the live later keys
    for (long long r = wv; r < m; r += PG_WAVES) {
      if (best[r] != TR_RESCAN) continue;                    // (wave-uniform)
      const long long *row = S + r * m;
      TrCand c = {0, 1, TR_NONE};
      for (long long x = r + 1 + lane; x < m; x += WAVE) {
        const int sx = size[x];
        if (sx > 0) {
          const TrCand o = {row[x], sx, (int)x};
          if (tr_less(o, c)) c = o;
        }
      }
      c = tr_wave_min(c);
      if (lane == 0) { best[r] = c.idx; bsum[r] = c.num; }
    }
    BARRIER();
    // (2) the smallest average over the rows' best pairs; equal averages: the smallest row, whose partner is its smallest
    TrCand c = {0, 1, TR_NONE};
    PAR_FOR(r, m) {
      const int sr = size[r], p = sr > 0 ? best[r] : TR_NONE;
      if (p >= 0) {
        const TrCand o = {bsum[r], sr * size[p], (int)r};
        if (tr_less(o, c)) c = o;
      }
    }
    c = tr_wave_min(c);
    if (lane == 0) {
      TrPick w = {c.num, c.den, c.idx, TR_NONE, 0, 0};
      if (c.idx >= 0) { w.v = best[c.idx]; w.su = size[c.idx]; w.sv = size[w.v]; }
      red[wv] = w;
    }
    BARRIER();
    TrPick w = red[0];
#pragma unroll
    for (int q = 1; q < PG_WAVES; ++q) {
      const TrPick o = red[q];
      const TrCand oc = {o.num, o.den, o.u}, wc = {w.num, w.den, w.u};
      if (tr_less(oc, wc)) w = o;
    }
    const long long u = w.u, v = w.v;                        // (L - 1 - k live pairs at least: there is one)
    const int sn = w.su + w.sv;
    ONE_THREAD { out[2 * k] = (int32_t)u; out[2 * k + 1] = (int32_t)v; }
    if (k == L - 2) break;
    // (3) cluster u takes v's sums; what that means for row x.  Nobody reads size[u], size[v], best[u] here but their own threads.
    PAR_FOR(x, m) {
      if (x == u) { size[x] = sn; best[x] = TR_RESCAN; continue; }
      if (x == v) { size[x] = 0; continue; }
      if (size[x] <= 0) continue;
      const long long t = S[u * m + x] + S[v * m + x];
      S[u * m + x] = t;
      S[x * m + u] = t;
      if (x < v) {
        const int p = best[x];
        if (p == u || p == v) best[x] = TR_RESCAN;
        else if (x < u) {
          const TrCand nu = {t, sn, (int)u}, cur = {bsum[x], p >= 0 ? size[p] : 1, p};
          if (tr_less(nu, cur)) { best[x] = (int32_t)u; bsum[x] = t; }
        }
      }
    }
    BARRIER();
  }
  return true;
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_tree(const uint32_t *shared, long long shared_words, const int64_t *nw,
                                                          const int64_t *seqs, long long n_seqs, const int64_t *loci,
                                                          const int32_t *weights, int64_t *ws, long long ws_words, int32_t *merges,
                                                          long long merges_words, int32_t *status) {
  SHARED(int32_t, l_size, TR_LDS_M);
  SHARED(int32_t, l_best, TR_LDS_M);
  SHARED(long long, l_bsum, TR_LDS_M);
  SHARED(TrPick, red, PG_WAVES);
  SHARED(int, cnt, 3);                                       // leaves, their weight sum (both clamped above the limit), refused
  const int64_t *Lc = loci + MPRG_PG_TREE_FIELDS * (long long)BLOCK_ID;
  const long long first = Lc[0], m = Lc[1], toff = Lc[2], woff = Lc[3], moff = Lc[4];
  const bool ok = first >= 0 && m >= 1 && m <= 0x7fffffffLL && first <= n_seqs - m && toff >= 0 && toff <= shared_words &&
                  m <= (shared_words - toff) / m && moff >= 0 && moff <= merges_words;
  ONE_THREAD { cnt[0] = 0; cnt[1] = 0; cnt[2] = !ok; }
  BARRIER();
  if (ok) {
    long long leaves = 0, sum = 0;
    int low = 0;
    PAR_FOR(x, m) {
      if (seqs[2 * (first + x) + 1] <= 0) continue;
      const long long w = weights ? weights[first + x] : 1;
      ++leaves;
      if (w < 1 || w > TR_MAX_WEIGHT) low = 1; else sum += w;
    }
    if (leaves) ATOMIC_ADD(&cnt[0], (int)(leaves < TR_MAX_WEIGHT + 1 ? leaves : TR_MAX_WEIGHT + 1));
    if (sum) ATOMIC_ADD(&cnt[1], (int)(sum < TR_MAX_WEIGHT + 1 ? sum : TR_MAX_WEIGHT + 1));
    if (low) ATOMIC_OR(&cnt[2], 1);
  }
  BARRIER();
  const int L = cnt[0];
  int st = MPRG_PG_OK;
  if (cnt[2] || cnt[1] > TR_MAX_WEIGHT || L > TR_MAX_WEIGHT || (L >= 2 && 2LL * (L - 1) > merges_words - moff)) st = MPRG_PG_BAD_ITEM;
  else if (woff < 0 || woff > ws_words || m * (m + 2) > ws_words - woff) st = MPRG_PG_NO_SPACE;
  if (st != MPRG_PG_OK || L < 2) {                           // (the whole workgroup)
    ONE_THREAD status[BLOCK_ID] = st;
    return;
  }
  BARRIER();                                                 // cnt[2] is read above and written below
  long long *S = (long long *)(ws + woff);
  int32_t *out = merges + moff;
  const uint32_t *tab = shared + toff;
  const int64_t *nwl = nw + first, *seql = seqs + 2 * first;
  const int32_t *wl = weights ? weights + first : nullptr;
  bool built;
  if (m <= TR_LDS_M) built = tr_build(l_size, l_best, l_bsum, S, tab, nwl, seql, wl, m, L, out, red, &cnt[2]);
  else {
    int32_t *g = (int32_t *)(S + m * m);
    built = tr_build(g, g + m, S + m * m + m, S, tab, nwl, seql, wl, m, L, out, red, &cnt[2]);
  }
  ONE_THREAD status[BLOCK_ID] = built ? MPRG_PG_OK : MPRG_PG_BAD_ITEM;
}
