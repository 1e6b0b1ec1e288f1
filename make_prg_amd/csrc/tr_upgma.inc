// The exact UPGMA of a locus and the kernel around it, for k_prog_tree and k_prog_tree_wide.  Included as text (DESIGN.md §3a); the
// including file provides TR_CAND {num, den, idx} and TR_PICK {num, den, u, v, su, sv}, its candidate types (num long long, den in
// the type its denominators need), TR_LESS(a, b), its compare of two candidates' averages (ties to the smaller idx; idx < 0: none),
// TR_DEN(a, b), the product of two sizes in den's type, TR_WEIGHT_TOP and TR_LEAF_TOP, the largest weight sum and the most leaves it
// builds, and the names TR_WAVE_MIN, TR_BUILD and TR_KERNEL of what this text defines: the wavefront's smallest candidate, the
// merges of one locus, the kernel.

// the smallest candidate of the wavefront, in every lane (all 64 lanes call it)
MPRG_DEV TR_CAND TR_WAVE_MIN(TR_CAND c) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    TR_CAND o;
    o.num = __shfl_xor(c.num, d); o.den = __shfl_xor(c.den, d); o.idx = __shfl_xor(c.idx, d);
    if (TR_LESS(o, c)) c = o;
  }
  return c;
}

// The merges of a locus of L >= 2 leaves whose ranges have been checked; size, best, bsum: m slots each, in LDS or in global
// memory.  Returns false (nothing of `out` written) when a table entry breaks the bound the arithmetic relies on.
MPRG_DEV bool TR_BUILD(int32_t *size, int32_t *best, long long *bsum, long long *S, const uint32_t *tab, const int64_t *nwl,
                       const int64_t *seql, const int32_t *wl, long long m, int L, int32_t *out, TR_PICK *red, int *flag) {
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
      TR_CAND c = {0, 1, TR_NONE};
      for (long long x = r + 1 + lane; x < m; x += WAVE) {
        const int sx = size[x];
        if (sx > 0) {
          const TR_CAND o = {row[x], sx, (int)x};
          if (TR_LESS(o, c)) c = o;
        }
      }
      c = TR_WAVE_MIN(c);
      if (lane == 0) { best[r] = c.idx; bsum[r] = c.num; }
    }
    BARRIER();
    // (2) the smallest average over the rows' best pairs; equal averages: the smallest row, whose partner is its smallest
    TR_CAND c = {0, 1, TR_NONE};
    PAR_FOR(r, m) {
      const int sr = size[r], p = sr > 0 ? best[r] : TR_NONE;
      if (p >= 0) {
        const TR_CAND o = {bsum[r], TR_DEN(sr, size[p]), (int)r};
        if (TR_LESS(o, c)) c = o;
      }
    }
    c = TR_WAVE_MIN(c);
    if (lane == 0) {
      TR_PICK w = {c.num, c.den, c.idx, TR_NONE, 0, 0};
      if (c.idx >= 0) { w.v = best[c.idx]; w.su = size[c.idx]; w.sv = size[w.v]; }
      red[wv] = w;
    }
    BARRIER();
    TR_PICK w = red[0];
#pragma unroll
    for (int q = 1; q < PG_WAVES; ++q) {
      const TR_PICK o = red[q];
      const TR_CAND oc = {o.num, o.den, o.u}, wc = {w.num, w.den, w.u};
      if (TR_LESS(oc, wc)) w = o;
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
          const TR_CAND nu = {t, sn, (int)u}, cur = {bsum[x], p >= 0 ? size[p] : 1, p};
          if (TR_LESS(nu, cur)) { best[x] = (int32_t)u; bsum[x] = t; }
        }
      }
    }
    BARRIER();
  }
  return true;
}

__global__ void __launch_bounds__(PG_THREADS) TR_KERNEL(const uint32_t *shared, long long shared_words, const int64_t *nw,
                                                        const int64_t *seqs, long long n_seqs, const int64_t *loci,
                                                        const int32_t *weights, int64_t *ws, long long ws_words, int32_t *merges,
                                                        long long merges_words, int32_t *status) {
  SHARED(int32_t, l_size, TR_LDS_M);
  SHARED(int32_t, l_best, TR_LDS_M);
  SHARED(long long, l_bsum, TR_LDS_M);
  SHARED(TR_PICK, red, PG_WAVES);
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
      if (w < 1 || w > TR_WEIGHT_TOP) low = 1; else sum += w;
    }
    if (leaves) ATOMIC_ADD(&cnt[0], (int)(leaves < TR_LEAF_TOP + 1 ? leaves : TR_LEAF_TOP + 1));
    if (sum) ATOMIC_ADD(&cnt[1], (int)(sum < TR_WEIGHT_TOP + 1 ? sum : TR_WEIGHT_TOP + 1));
    if (low) ATOMIC_OR(&cnt[2], 1);
  }
  BARRIER();
  const int L = cnt[0];
  int st = MPRG_PG_OK;
  if (cnt[2] || cnt[1] > TR_WEIGHT_TOP || L > TR_LEAF_TOP || (L >= 2 && 2LL * (L - 1) > merges_words - moff)) st = MPRG_PG_BAD_ITEM;
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
  if (m <= TR_LDS_M) built = TR_BUILD(l_size, l_best, l_bsum, S, tab, nwl, seql, wl, m, L, out, red, &cnt[2]);
  else {
    int32_t *g = (int32_t *)(S + m * m);
    built = TR_BUILD(g, g + m, S + m * m + m, S, tab, nwl, seql, wl, m, L, out, red, &cnt[2]);
  }
  ONE_THREAD status[BLOCK_ID] = built ? MPRG_PG_OK : MPRG_PG_BAD_ITEM;
}
