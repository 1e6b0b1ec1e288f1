// ---------------------------------------------------------------------------------------------------------------
// K2  interval partition of one view per workgroup
//     reference from_msa/interval_partition.py:81-252 (IntervalPartitioner), utils/seq_utils.py:37-42
//
// Phases: (1) per-column longest all-gap run ending there over the view's rows (answers every
// has_empty_sequence(a,b) probe as maxrun[b] >= b-a+1); (2) thread 0 walks the consensus exactly as the reference's
// single left-to-right pass does (stacks of match / non-match intervals live in global scratch); (3) every non-match
// interval is tested for "fewer than two sequences" (enforce_multisequence_nonmatch_intervals) by comparing each
// row's ungapped content with the first N-free row, exactly (no hashing; 8 cells per load where the rows agree);
// (4) thread 0 emits the intervals sorted by start and checks that they tile the view
// (enforce_alignment_interval_bijection).  The level's triples are then packed by k_pack_scan / k_pack_copy.
// ---------------------------------------------------------------------------------------------------------------
MPRG_DEV bool col_is_nonmatch(const uint32_t *mask, int c) { return consensus_code(mask[c]) == 255; }

// K2a  longest all-gap run ending at each column over the view's rows (answers has_empty_sequence(a,b) as
//      maxrun[b] >= b-a+1; utils/seq_utils.py:37-42).  One (view, 256-row chunk, 512-column segment) per workgroup, thread = row
//      over the transposed copy (coalesced), atomicMax only where a gap run is alive; segments without any gap return at once.
//      A row's run at the start of a segment is counted backwards from there (a gap run is short next to a segment).
//      Work items: {view, segment * row chunks + row chunk}, gr_items() of them per view.
#define GR_ROWS 256
#ifndef GR_SEG
#define GR_SEG 512
#endif
#ifndef GR_BATCH
#define GR_BATCH 16                    // cells of its row a lane of k_gap_runs keeps in flight (8 cells per trip and 2 048-column segments: 256 round trips per lane)
#endif
MPRG_DEV long long gr_items(long long S, long long n) { return ((S + GR_ROWS - 1) / GR_ROWS) * ((n + GR_SEG - 1) / GR_SEG); }
KERNEL(k_gap_runs, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, const int32_t *work,
       const uint32_t *mask_all, uint32_t *maxrun_all, DsCount dc) {
  DS_GUARD(dc, 1);
  const int32_t *wk = work + 2 * (long long)BLOCK_ID;
  const ViewD d = load_view(views, wk[0]);
  const int n_chunks = (d.n_rows + GR_ROWS - 1) / GR_ROWS;
  const int r0 = (wk[1] % n_chunks) * GR_ROWS, cA = (wk[1] / n_chunks) * GR_SEG, cB = cA + GR_SEG < d.n_cols ? cA + GR_SEG : d.n_cols;
  const uint32_t *mask = mask_all + d.col_off;
  uint32_t *maxrun = maxrun_all + d.col_off;
  SHARED(int, has_gap, 1);
  ONE_THREAD { has_gap[0] = 0; }
  BARRIER();
  PAR_FOR(c, cB - cA) { if (mask[cA + c] & BIT_GAP) has_gap[0] = 1; }
  BARRIER();
  if (!has_gap[0]) return;
  PAR_FOR(t, GR_ROWS) {
    const int i = r0 + (int)t;
    if (i >= d.n_rows) continue;
    const int row = view_row(d, rowidx, i);
    uint32_t run = 0;
    for (int b = cA - 1; b >= 0 && cell_t(arena, d, row, b) == C_GAP; --b) ++run;       // the run that reaches into this segment
    int c = cA;
    for (; c + GR_BATCH <= cB; c += GR_BATCH) {          // GR_BATCH cells per round trip (the atomics would otherwise fence the loads)
      unsigned x[GR_BATCH];
#pragma unroll
      for (int q = 0; q < GR_BATCH; ++q) x[q] = cell_t(arena, d, row, c + q);
#pragma unroll
      for (int q = 0; q < GR_BATCH; ++q) { if (x[q] == C_GAP) { ++run; ATOMIC_MAX(maxrun + c + q, run); } else run = 0; }
    }
    for (; c < cB; ++c) {
      if (cell_t(arena, d, row, c) == C_GAP) { ++run; ATOMIC_MAX(maxrun + c, run); } else run = 0;
    }
  }
}

#define PT_STACK 512                  // LDS interval stacks: entries per stack
#define PT_COLS 16384                 // LDS: "is a non-match column" bytes + run lists (5 bytes per column); reused for the sorted triples
// Phases 2-4 of K2.  FAST: the stacks, the per-column non-match bytes, the retyping decisions and the emitted triples
// live in LDS, so the two serial stretches (scan, merge) never wait on global memory: a serial loop that mixes loads
// with global stores runs at one memory round trip per step.  !FAST (very wide views, tiny min_match_length): the
// same code on the global scratch.
// CL: the view's cells sit in LDS (cells_s[row position * cpitch + column], K2f) instead of the arena.
// first column in [i, n) whose non-match bit differs from `cur`, else n (bits: one per column, zero beyond n)
MPRG_DEV int pt_next_switch(const uint32_t *bits, int i, int n, bool cur) {
  while (i < n) {
    uint32_t w = bits[i >> 5];
    if (cur) w = ~w;
    w &= 0xffffffffu << (i & 31);
    if (w) { const int c = (i & ~31) + __ffs((int)w) - 1; return c < n ? c : n; }
    i = (i & ~31) + 32;
  }
  return n;
}
// The scan's closing rule (interval_partition.py _add_interval :143-185): close the run [cs, ce] of kind cur_non when the scan reaches
// column i (`end`: i is the view's width).  Stated once for the two scans that run it — the view's own (pt_phases, stacks in LDS /
// global scratch) and the hint scan of a non-match interval's columns (pt_scan_is_self, the stacks' tops in registers).  The user
// defines the stacks: nm / nn (entries), PUSH_M / PUSH_N (s, e), PT_POP_N (s, e out), PT_TOP_M_LEN, PT_DROP_M, PT_SHRINK_TOP_M (its
// end one column back), PT_GROW_TOP_N (its end x columns on), and PT_GAP_AT_CE: the longest all-gap row stretch ending at column ce.
#define PT_CLOSE_RUN()                                                                                                  \
        bool cont = false;                                                                                              \
        int ns = 0, ne = 0;                                                                                             \
        if (!cur_non) {                                                                                                 \
          if (ce - cs + 1 < L) {                       /* short match: absorbed by a non-match interval */              \
            if (nn > 0) { PT_POP_N(ns, ne); ne += (ce - cs + 1) + 1; }                                                  \
            else { ns = cs; ne = ce + 1; }                                                                              \
            if (end) { ne -= 1; PUSH_N(ns, ne); }                                                                       \
            cont = true;                                                                                                \
          } else PUSH_M(cs, ce);                                                                                        \
        } else {                                                                                                        \
          bool pushed = false;                                                                                          \
          if (nm > 0 && PT_GAP_AT_CE >= (uint32_t)(ce - cs + 1)) {   /* has_empty_sequence(alignment, (cs, ce)) */      \
            const int lm = PT_TOP_M_LEN();                                                                              \
            if (lm - 1 < L) {                                                                                           \
              PT_DROP_M(); cs -= lm;                                                                                    \
              if (nn > 0) { PT_GROW_TOP_N(ce - cs + 1); pushed = true; }                                                \
            } else { PT_SHRINK_TOP_M(); cs -= 1; }                                                                      \
          }                                                                                                             \
          if (!pushed) PUSH_N(cs, ce);                                                                                  \
        }
// MPRG_IV_SELF: would columns s..e of this view, taken as a view of their own with the same rows, partition into exactly themselves —
// no match interval, one non-match interval (0, e - s)?  The scan of those columns is RUN (same closing rule, same n < L branch):
// their consensus is this view's (nmz: non-match bytes of this view's columns), and has_empty_sequence(a, b) asks for a row that is
// all gaps from a to b, which does not depend on where a view starts (maxrun[b] >= b - a + 1, maxrun this view's).  Only the top
// PT_SELF_STACK entries of either stack are kept, in registers; a push beyond them answers "no".  (That "no" is the scan's answer
// too: a non-match run always starts where the top match interval ends, and a match interval that has stayed after the probe of the
// run behind it stays for good — a later probe spans that run as well, or, after PT_SHRINK_TOP_M, a match column, where no row holds
// a gap — and two non-match intervals on the stack have such a match interval between them: a third entry on either stack means a
// match interval is in the result.)
// The walk goes from switch to switch of the consensus.  run_start / run_gap (may be null): the view's run lists (pt_phases, by_runs)
// — the next switch and the gap stretch at a run's end are then one LDS read each instead of a walk over the run's columns and a
// read of global memory: a root view's longest non-match interval spans hundreds of columns, and its lane holds up the workgroup.
#define PT_SELF_STACK 2
struct PtTops { int s0, e0, s1, e1; };
MPRG_DEV bool pt_scan_is_self(const uint8_t *nmz, const uint32_t *maxrun, int s, int e, int L, const uint16_t *run_start,
                              const uint16_t *run_gap, int R, int n) {
  if (e < s) return false;
  if (e - s + 1 < L) {                                // (every column goes to one interval: non-match if any column is)
    bool any = false;
    for (int c = s; c <= e; ++c) any = any || nmz[c] != 0;
    return any;
  }
  int r = 0;                                          // by runs: the run that holds column `at`
  if (run_start) {
    int hi = R;                                       // (run_start[0] == 0 <= s)
    while (hi - r > 1) { const int mid = (r + hi) >> 1; if ((int)run_start[mid] <= s) r = mid; else hi = mid; }
  }
  PtTops Ms = {0, 0, 0, 0}, Ns = {0, 0, 0, 0};
  int nm = 0, nn = 0;
#define PT_SELF_PUSH(T, cnt, s_, e_) do { if (cnt >= PT_SELF_STACK) return false; T.s1 = T.s0; T.e1 = T.e0; T.s0 = (s_); T.e0 = (e_); ++cnt; } while (0)
#define PT_SELF_POP(T, cnt) do { T.s0 = T.s1; T.e0 = T.e1; --cnt; } while (0)
#define PUSH_M(s_, e_) PT_SELF_PUSH(Ms, nm, s_, e_)
#define PUSH_N(s_, e_) PT_SELF_PUSH(Ns, nn, s_, e_)
#define PT_POP_N(s_, e_) do { (s_) = Ns.s0; (e_) = Ns.e0; PT_SELF_POP(Ns, nn); } while (0)
#define PT_TOP_M_LEN() (Ms.e0 - Ms.s0 + 1)
#define PT_DROP_M() PT_SELF_POP(Ms, nm)
#define PT_SHRINK_TOP_M() (Ms.e0 -= 1)
#define PT_GROW_TOP_N(x_) (Ns.e0 += (x_))
#define PT_GAP_AT_CE (whole_run ? (uint32_t)run_gap[r] : maxrun[ce])
  int cs = s, at = s;                                 // the open run starts at cs; `at`: a column of the consensus run it ends with
  bool cur_non = nmz[s] != 0;
  for (;;) {
    int i;                                            // the next switch: first column of the next consensus run
    if (run_start) i = r + 1 < R ? (int)run_start[r + 1] : n;
    else { i = at + 1; while (i <= e && (nmz[i] != 0) == cur_non) ++i; }
    const bool whole_run = run_start != nullptr && i <= e + 1;      // (the columns end inside a consensus run: its gap stretch is not the list's)
    if (i > e + 1) i = e + 1;
    const int ce = i - 1;
    const bool end = (i == e + 1);
    PT_CLOSE_RUN()
    if (end) break;
    cs = cont ? ns : i;                               // (cont: the short match run and the non-match run behind it go on as one open run)
    cur_non = !cur_non; at = i; ++r;
  }
#undef PT_SELF_PUSH
#undef PT_SELF_POP
#undef PUSH_M
#undef PUSH_N
#undef PT_POP_N
#undef PT_TOP_M_LEN
#undef PT_DROP_M
#undef PT_SHRINK_TOP_M
#undef PT_GROW_TOP_N
#undef PT_GAP_AT_CE
  return nm == 0 && nn == 1 && Ns.s0 == s && Ns.e0 == e;
}
// WV: the phases run by ONE wavefront on its own (k_partition_wave: several small views per workgroup): the loops stride the 64
// lanes, what the workgroup forms settle with a barrier is a wavefront-scope fence (WAVE_SYNC), "one thread" is lane 0.
template <bool FAST, bool CL, bool WV = false>
MPRG_DEV void pt_phases(const uint8_t *arena, const ViewD &d, const int32_t *rowidx, const uint32_t *mask, int L,
                        const uint32_t *maxrun, int32_t *gstack, int32_t *flag_multi, int32_t *ref_row, int32_t *iv,
                        int32_t *stk_s, int stack_cap, uint8_t *nmz_s, int nmz_cap, int32_t *ntype_s, int *sh,
                        const uint8_t *cells_s, int cpitch KM_TPARAM) {
#define P_FOR(i_, n_) for (long long i_ = WV ? wave_lane() : MPRG_TID; i_ < (long long)(n_); i_ += WV ? WAVE : (int)blockDim.x)
#define P_BAR() do { if (WV) WAVE_SYNC(); else BARRIER(); } while (0)
#define P_ONE if ((WV ? wave_lane() : MPRG_TID) == 0)
  const int n = d.n_cols;
  int32_t *Ms = FAST ? stk_s : gstack;                                  // match stack: (s,e) pairs
  int32_t *Ns = FAST ? stk_s + 2 * stack_cap : gstack + 2 * (long long)n; // non-match stack
  // !CL: the row-major copy — the tasks below run along a row's columns (interval by interval), so neighbouring lanes and
  // consecutive steps stay inside one row's bytes, and 8 cells come with one (unaligned) 64-bit load
#define PCELL(i_, row_, c_) (CL ? (unsigned)cells_s[(i_) * cpitch + (c_)] \
                                : (unsigned)arena[d.rm + (long long)(row_) * d.pitchC + d.col0 + (c_)])
#define PCELL8(i_, row_, c_, out_) do { if (CL) __builtin_memcpy(&(out_), cells_s + (i_) * cpitch + (c_), 8); \
                                        else __builtin_memcpy(&(out_), arena + d.rm + (long long)(row_) * d.pitchC + d.col0 + (c_), 8); } while (0)
  int32_t *ivw = FAST ? (int32_t *)nmz_s : iv;                           // FAST: triples staged in LDS, copied out below
#define NONMATCH(c) (FAST ? nmz_s[c] != 0 : col_is_nonmatch(mask, c))
  // ---- phase 2: the reference's scan (interval_partition.py:88-110, _add_interval :143-185).  The scan only acts where
  //      the consensus switches between match and non-match columns, so (FAST, 3n <= nmz_cap) all threads first list the
  //      run starts in order and the serial walk visits runs, not columns (a 2000-column root view has ~100 runs).
  const bool by_runs = !WV && FAST && n >= L && 5LL * n + 8 <= nmz_cap && n < 65535;
  uint16_t *run_start = (uint16_t *)(nmz_s + ((n + 1) & ~1));      // [n] column where run r starts
  uint16_t *run_gap = run_start + n;                               // [n] longest all-gap row stretch ending with run r
  if (by_runs) {
    // run starts in column order: every thread counts the starts of its chunk of columns, a workgroup prefix sum places them
    const int chunk = (n + N_THREADS - 1) / N_THREADS;
    const int c_lo = (int)threadIdx.x * chunk, c_hi = c_lo + chunk < n ? c_lo + chunk : n;
    int k = 0;
    for (int c = c_lo; c < c_hi; ++c) k += (c == 0 || nmz_s[c] != nmz_s[c - 1]) ? 1 : 0;
    int total;
    int o = block_scan_excl(k, (int *)stk_s, &total);    // the stacks are not in use yet
    P_ONE { sh[6] = total; }
    for (int c = c_lo; c < c_hi; ++c)
      if (c == 0 || nmz_s[c] != nmz_s[c - 1]) run_start[o++] = (uint16_t)c;
    P_BAR();
    P_FOR(r, sh[6]) {                                 // has_empty_sequence() is only ever asked at the end of a run
      const int e = (r + 1 < sh[6] ? (int)run_start[r + 1] : n) - 1;
      const uint32_t g = maxrun[e];
      run_gap[r] = (uint16_t)(g > 65535u ? 65535u : g);
    }
    P_BAR();
  }
  // !FAST (a view wider than the LDS column bytes, or one whose worst case overruns the LDS stacks): the non-match flags as a
  // BIT array in LDS — the serial walk then jumps from switch to switch, a word of 32 columns per step, instead of fetching
  // every column's mask from global memory (4 ms for the 20 000 columns of BASELINE config D)
  const bool wide_bits = !FAST && n >= L && (long long)n + 32 <= 8LL * nmz_cap;
  if (wide_bits) {
    uint32_t *bits = (uint32_t *)nmz_s;
    P_FOR(w, (n + 31) >> 5) {
      uint32_t b = 0;
      for (int q = 0; q < 32; ++q) { const int c = 32 * (int)w + q; if (c < n && col_is_nonmatch(mask, c)) b |= 1u << q; }
      bits[w] = b;
    }
    P_BAR();
  }
  P_ONE {
    int nm = 0, nn = 0;
#define PUSH_M(s, e) do { Ms[2 * nm] = (s); Ms[2 * nm + 1] = (e); ++nm; } while (0)
#define PUSH_N(s, e) do { Ns[2 * nn] = (s); Ns[2 * nn + 1] = (e); ++nn; } while (0)
    // (PT_CLOSE_RUN's stacks: the arrays Ms / Ns)
#define PT_POP_N(s_, e_) do { --nn; (s_) = Ns[2 * nn]; (e_) = Ns[2 * nn + 1]; } while (0)
#define PT_TOP_M_LEN() (Ms[2 * (nm - 1) + 1] - Ms[2 * (nm - 1)] + 1)
#define PT_DROP_M() (--nm)
#define PT_SHRINK_TOP_M() (Ms[2 * (nm - 1) + 1] -= 1)
#define PT_GROW_TOP_N(x_) (Ns[2 * (nn - 1) + 1] += (x_))
    if (n < L) {
      if (n > 0) {
        bool any = false;
        for (int c = 0; c < n; ++c) any = any || NONMATCH(c);
        if (any) PUSH_N(0, n - 1); else PUSH_M(0, n - 1);
      }
    } else if (by_runs) {
      const int R = sh[6];
      int cs = 0, ce = (R > 1 ? (int)run_start[1] : n) - 1;
      bool cur_non = NONMATCH(0);
      for (int r = 1; r <= R; ++r) {                   // boundary r: run r starts at column i (r == R: the end)
        const bool end = (r == R);
        const int i = end ? n : (int)run_start[r];
        const bool tt = end ? false : NONMATCH(i);
#define PT_GAP_AT_CE ((uint32_t)run_gap[r - 1])        /* ce is the last column of run r - 1 */
        PT_CLOSE_RUN()
#undef PT_GAP_AT_CE
        if (end) break;
        if (cont) { cs = ns; ce = ne; cur_non = true; }
        else { cs = i; ce = i; cur_non = tt; }
        ce += (r + 1 < R ? (int)run_start[r + 1] : n) - 1 - i;   // the rest of run r: every column extends the open run
      }
    } else if (wide_bits) {                            // !FAST: the same walk, from switch to switch over the bit array
      const uint32_t *bits = (const uint32_t *)nmz_s;
      int cs = 0, ce = 0;
      bool cur_non = (bits[0] & 1u) != 0;
      for (int i = 1; i <= n; ++i) {
        i = pt_next_switch(bits, i, n, cur_non);       // (the open run always ends at the column before the switch)
        ce = i - 1;
        const bool end = (i == n);
#define PT_GAP_AT_CE maxrun[ce]
        PT_CLOSE_RUN()
#undef PT_GAP_AT_CE
        if (end) break;
        if (cont) { cs = ns; cur_non = true; }
        else { cs = i; cur_non = !cur_non; }
      }
    } else {
      int cs = 0, ce = 0;
      bool cur_non = NONMATCH(0);
      for (int i = 1; i <= n; ++i) {
        const bool end = (i == n);
        bool t = false;
        if (!end) {
          t = NONMATCH(i);
          if (t == cur_non) { ++ce; continue; }
        }
#define PT_GAP_AT_CE maxrun[ce]
        PT_CLOSE_RUN()
#undef PT_GAP_AT_CE
        if (end) break;
        if (cont) { cs = ns; ce = ne; cur_non = true; }
        else { cs = i; ce = i; cur_non = t; }
      }
    }
#undef PT_POP_N
#undef PT_TOP_M_LEN
#undef PT_DROP_M
#undef PT_SHRINK_TOP_M
#undef PT_GROW_TOP_N
    sh[1] = nm; sh[2] = nn;
  }
  P_BAR();
  P_FOR(j, sh[2]) { flag_multi[j] = 0; ref_row[j] = (sh[4] || d.n_rows == 0) ? 0x7fffffff : 0; }
  P_BAR(); KM_T(17);
  // ---- phase 3: non-match intervals with fewer than two (expanded) sequences become match intervals
  //      (interval_partition.py:187-217; SequenceExpander utils/seq_utils.py:116-158)
  const int nn = sh[2];
  const long long tasks = (long long)nn * d.n_rows;
  const bool scan_n = sh[4] != 0, scan_amb = sh[4] != 0 || sh[5] != 0;   // the masks say whether N / IUPAC occur at all
  P_FOR(tk, scan_n ? tasks : 0) {                   // pass A: rows containing N are left out; first N-free row
    const int j = (int)(tk / d.n_rows), i = (int)(tk % d.n_rows);
    const int row = view_row(d, rowidx, i);
    bool hasN = false;
    for (int c = Ns[2 * j]; c <= Ns[2 * j + 1] && c < n; ++c) hasN = hasN || (PCELL(i, row, c) == C_N);
    if (!hasN) ATOMIC_MIN(ref_row + j, i);
  }
  P_BAR(); KM_T(18);
  // pass B: does some N-free row differ from the reference row once gaps are removed?  One (interval, row) task per
  // thread, exact two-pointer comparison.  Most rows EQUAL the reference row and would walk the whole interval, yet one
  // differing row settles the question: FAST keeps a per-interval "settled" word in LDS that every walk polls.
  int32_t *settled = ntype_s;                        // free until phase 4 writes the retyping decisions
  if (FAST) { P_FOR(j, nn) { settled[j] = 0; } P_BAR(); }
  P_FOR(tk, tasks) {
    // interval index fastest: the rows of an interval are spread over the rounds, so once an early row has settled the
    // interval the later rounds skip their walks (a root view has ~60 intervals x 100 rows)
    const int j = (int)((unsigned)tk % (unsigned)nn), i = (int)((unsigned)tk / (unsigned)nn);
    const int ref = scan_n ? ref_row[j] : 0;          // without N in the view every row qualifies: the first one
    if (ref == 0x7fffffff) continue;
    const int a = Ns[2 * j], b = (Ns[2 * j + 1] < n) ? Ns[2 * j + 1] : n - 1;
    const int row = view_row(d, rowidx, i), rrow = view_row(d, rowidx, ref);
    bool hasN = false, iupac = false;
    if (scan_amb) for (int c = a; c <= b; ++c) {
      const unsigned x = PCELL(i, row, c);
      hasN = hasN || x == C_N;
      iupac = iupac || (x >= 5 && x <= 10);
    }
    if (hasN) continue;
    int f = iupac ? 2 : 0;
    // (!FAST — a view too wide for the LDS column bytes — polls the interval's flag word itself: it only ever gains bits, and a walk
    //  only ever adds bit 0; the 10 000 rows of BASELINE config D each walked to their first difference from row 0: 0.45 ms of one
    //  workgroup's round trips)
    if (i != ref && !(FAST ? settled[j] != 0 : ((*(volatile int32_t *)(flag_multi + j)) & 1) != 0)) {          // two-pointer walk over the non-gap characters
      int p = a, q = a;
      bool differ = false;
      for (;;) {
        if (p == q) {                                 // aligned pointers: equal cells (same symbol or both gaps) move both
          while (p + 8 <= b + 1) {                    // pointers by one each, so equal stretches are skipped 8 at a time
            uint64_t x8, y8;
            PCELL8(i, row, p, x8); PCELL8(ref, rrow, p, y8);
            if (x8 != y8 || (FAST && settled[j])) break;
            p += 8;
          }
          q = p;
        }
        if (FAST && settled[j]) break;                // another row already differs: this walk cannot change the flag
        while (p <= b && PCELL(i, row, p) == C_GAP) ++p;
        while (q <= b && PCELL(ref, rrow, q) == C_GAP) ++q;
        if (p > b || q > b) { differ = (p <= b) != (q <= b); break; }
        if (PCELL(i, row, p) != PCELL(ref, rrow, q)) { differ = true; break; }
        ++p; ++q;
      }
      if (differ) { f |= 1; if (FAST) settled[j] = 1; }
    }
    if (f) ATOMIC_OR(flag_multi + j, f);
  }
  P_BAR();
  KM_T(19);
  // ---- phase 4: emit the intervals sorted by start (both stacks are sorted: a two-way merge), retype, and check that
  //      they tile the view (enforce_alignment_interval_bijection, interval_partition.py:219-252)
  // retyping decision per non-match interval: 0 match (one distinct sequence without ambiguity codes), 1 non-match,
  // 3 non-match and every row of the slice contained N; an alignment without rows skips the test (:201-202)
#define NTYPE(j) (d.n_rows > 0 ? (ref_row[j] == 0x7fffffff ? 3 : (flag_multi[j] == 0 ? 0 : 1)) : 1)
  // FAST, a thread per non-match interval: + MPRG_IV_SELF where the interval stays a non-match interval of a view with rows and
  // without N / ambiguity codes (what `pure` asks below) and the scan of its own columns gives the interval back (the non-match
  // bytes are still in nmz_s: the triples overwrite them only below).  The child node then needs no partition (k_forest.inc S1).
  if (FAST) {
    const bool hint = !(sh[4] || sh[5]) && d.n_rows > 0;
    P_FOR(j, nn) {
      int ty = NTYPE(j);
      if (hint && ty == 1 && Ns[2 * j] >= 0 && Ns[2 * j + 1] < n && pt_scan_is_self(nmz_s, maxrun, Ns[2 * j], Ns[2 * j + 1], L, by_runs ? run_start : nullptr, run_gap, by_runs ? sh[6] : 0, n)) ty |= MPRG_IV_SELF;
      ntype_s[j] = ty;
    }
    P_BAR();
  }
  P_ONE {
    const int nm = sh[1];
    int status = 0, cnt = 0, expect = 0, im = 0, in = 0;
    // bit 1 of the type word: a match interval straight from the scan in a view without N / ambiguity codes — every
    // column is one plain base for these rows, so the child node is a one-allele leaf whatever else (MPRG_IV_PURE)
    const int pure = (sh[4] || sh[5]) ? 0 : 2;
    while (im < nm || in < nn) {
      const bool takeM = in >= nn || (im < nm && Ms[2 * im] <= Ns[2 * in]);
      int s, e, type;
      if (takeM) { s = Ms[2 * im]; e = Ms[2 * im + 1]; type = pure; ++im; }
      else {
        s = Ns[2 * in]; e = Ns[2 * in + 1];
        const int ty = FAST ? ntype_s[in] : NTYPE(in);
        if ((ty & 3) == 3) status |= 2;
        type = ty & (1 | MPRG_IV_SELF);
        ++in;
      }
      if (s != expect || e < s || e >= n) { status |= 1; break; }
      ivw[3 * cnt] = s; ivw[3 * cnt + 1] = e; ivw[3 * cnt + 2] = type;
      ++cnt;
      expect = e + 1;
    }
    if (expect != n || cnt != nm + nn) status |= 1;
    sh[6] = cnt; sh[3] = status; sh[7] = cnt > 0 ? (ivw[2] & 1) : 0;
  }
  P_BAR(); KM_T(20);
#undef PUSH_M
#undef PUSH_N
#undef NONMATCH
#undef NTYPE
#undef PCELL
#undef PCELL8
#undef P_FOR
#undef P_BAR
#undef P_ONE
}

// what the host's control step needs of the view, in one record; the sorted triples (still in LDS on the fast paths) go to
// the view's slots.  The packed list (sum(n_iv) triples for the host instead of one slot per column) is filled afterwards
// by k_pack_scan / k_pack_copy: one returning atomic per view on a single counter serialised the views of a level
// (28 % of the partition kernels' cycles, profiles/r02/kmeans_phase_cycles.txt).
template <bool WV = false>
MPRG_DEV void pt_outputs(int v, int *sh, bool fast, const uint8_t *nmz_s, int32_t *iv, int32_t *n_iv_out, int32_t *status_out,
                         int32_t *view_out KM_TPARAM) {
  if ((WV ? wave_lane() : MPRG_TID) == 0) {
    const int cnt = sh[6], status = sh[3];
    n_iv_out[v] = cnt;
    status_out[v] = status;
    if (view_out) {
      int32_t *o = view_out + 8 * (long long)v;
      o[0] = cnt; o[1] = status; o[2] = sh[7];
      o[3] = (sh[0] ? 1 : 0) | ((sh[4] || sh[5]) ? 2 : 0) | (sh[4] ? 4 : 0);       // (N is no part of a column's consensus: its own bit)
      o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;       // o[4]: first packed triple (k_pack_scan)
    }
  }
  KM_T(22);
  if (fast) {
    const int32_t *src = (const int32_t *)nmz_s;
    for (int e = WV ? wave_lane() : MPRG_TID; e < 3 * sh[6]; e += WV ? WAVE : (int)blockDim.x) iv[e] = src[e];
  }
}
// packed list of the level's triples: exclusive prefix sum of the views' interval counts, then a wavefront per view copies its
// triples to its place.  The scan by MANY workgroups, PK_VIEWS consecutive views each: a workgroup first sums the counts of all
// EARLIER views itself (coalesced loads of a few hundred KB that stay in L2: no partial sums pass between workgroups, so there is no
// scratch and no second launch), then scans its own views, PK_SCAN_PER_THREAD consecutive ones per thread.  The workgroup that holds
// the last view writes the total.  (Until round 7 ONE workgroup walked a level's 10^5 - 3 x 10^5 views in serial batches of 32 768:
// 0.3 ms for the largest level, 0.9 ms per pass of 7 500 alignments; this form: 0.065 ms and 0.23 ms.)
#define PK_SCAN_THREADS 1024
#define PK_SCAN_PER_THREAD 8
#define PK_VIEWS (PK_SCAN_THREADS * PK_SCAN_PER_THREAD)
KERNEL(k_pack_scan, int n_views_cap, const int32_t *n_iv, int32_t *view_out, int32_t *iv_count, DsCount dc) {
  const int n_views = (int)ds_n(dc, n_views_cap);
  const int v0 = BLOCK_ID * PK_VIEWS;
  if (BLOCK_ID > 0 && v0 >= n_views) return;
  SHARED(int, scratch, 17);
  int part = 0;
  for (int u = (int)threadIdx.x; u < v0; u += PK_SCAN_THREADS) part += n_iv[u];
  int base;
  block_scan_excl(part, scratch, &base);
  const int v = v0 + (int)threadIdx.x * PK_SCAN_PER_THREAD;
  int c[PK_SCAN_PER_THREAD], sum = 0;
#pragma unroll
  for (int q = 0; q < PK_SCAN_PER_THREAD; ++q) { c[q] = v + q < n_views ? n_iv[v + q] : 0; sum += c[q]; }
  int tot;
  int run = base + block_scan_excl(sum, scratch, &tot);
#pragma unroll
  for (int q = 0; q < PK_SCAN_PER_THREAD; ++q) { if (v + q < n_views) view_out[8 * (long long)(v + q) + 4] = run; run += c[q]; }
  if (v0 + PK_VIEWS >= n_views) ONE_THREAD { iv_count[0] = base + tot; }
}
#define PK_THREADS 256
KERNEL(k_pack_copy, int n_views, const int64_t *views, const int32_t *iv_all, const int32_t *view_out, int32_t *iv_packed, DsCount dc) {
  const int v = BLOCK_ID * (PK_THREADS / WAVE) + wave_id();
  if (v >= ds_n(dc, n_views)) return;
  const int32_t *o = view_out + 8 * (long long)v;
  const int32_t *src = iv_all + 3 * views[(long long)v * VF + 8];      // the view's slots: 3 ints per column (MPRG_V_COL_OFF)
  int32_t *dst = iv_packed + 3 * (long long)o[4];
  for (int e = wave_lane(); e < 3 * o[0]; e += WAVE) dst[e] = src[e];
}

// view_list (may be null): the views this launch handles; null = view BLOCK_ID
KERNEL(k_partition, const int32_t *view_list, const uint8_t *arena, const int64_t *views, const int32_t *rowidx,
       const uint32_t *mask_all, int L, uint32_t *maxrun_all, int32_t *stack_all, int32_t *ivflag_all, int32_t *iv_all,
       int32_t *n_iv_out, int32_t *status_out, int32_t *view_out, DsCount dc) {
  DS_GUARD(dc, 1);
  KM_T0();
  const int v = view_list ? view_list[BLOCK_ID] : BLOCK_ID;
  const ViewD d = load_view(views, v);
  const int n = d.n_cols;
  const uint32_t *mask = mask_all + d.col_off;
  uint32_t *maxrun = maxrun_all + d.col_off;
  // Both stacks alternate along the view and a match interval is at least L-1 wide once pushed, so a few hundred
  // entries hold any pan-genome view.
  SHARED(int32_t, stk_s, 4 * PT_STACK);
  __shared__ __attribute__((aligned(16))) uint8_t nmz_s[PT_COLS];
  SHARED(int32_t, ntype_s, PT_STACK);
  const bool fast = n / (L > 1 ? L - 1 : 1) + 4 <= PT_STACK && n <= PT_COLS;
  int32_t *flag_multi = ivflag_all + 2 * d.col_off; // per non-match interval: bit0 = >= 2 distinct, bit1 = has IUPAC
  int32_t *ref_row = flag_multi + n;                // per non-match interval: first row position without N
  int32_t *iv = iv_all + 3 * d.col_off;
  SHARED(int, sh, 8);       // 0: a column is not one plain base, 1: n_match, 2: n_non, 3: status, 4: has_N, 5: has_iupac,
                            // 6: intervals emitted, 7: type of the first interval, then first packed triple
  ONE_THREAD { sh[0] = 0; sh[1] = 0; sh[2] = 0; sh[3] = 0; sh[4] = 0; sh[5] = 0; sh[6] = 0; sh[7] = 0; }
  BARRIER();
  // ---- phase 1 (gap runs) is k_gap_runs; here only: does the view hold N / ambiguity codes at all?
  PAR_FOR(c, n) {
    const uint32_t m = mask[c];
    if (m & BIT_N) sh[4] = 1;
    if (m & BITS_IUPAC) sh[5] = 1;
    const uint32_t mm = m & ~BIT_N;                   // N never counts towards the consensus (seq_utils.py:73-84)
    const bool star = !(mm != 0 && (mm & (mm - 1)) == 0 && (mm & BITS_IUPAC) == 0 && mm != BIT_GAP);
    if (star) sh[0] = 1;
    if (fast) nmz_s[c] = star ? 1 : 0;               // == col_is_nonmatch(mask, c)
  }
  BARRIER(); KM_T(16);
  if (fast) pt_phases<true, false>(arena, d, rowidx, mask, L, maxrun, stack_all + 4 * d.col_off, flag_multi, ref_row, iv, stk_s,
                                   PT_STACK, nmz_s, PT_COLS, ntype_s, sh, nullptr, 0 KM_TARG);
  else pt_phases<false, false>(arena, d, rowidx, mask, L, maxrun, stack_all + 4 * d.col_off, flag_multi, ref_row, iv, stk_s,
                               PT_STACK, nmz_s, PT_COLS, ntype_s, sh, nullptr, 0 KM_TARG);
  pt_outputs(v, sh, fast, nmz_s, iv, n_iv_out, status_out, view_out KM_TARG);
  KM_T(21);
}

// K2f  masks + gap runs + partition of a SMALL view in one workgroup, the view's cells in LDS (one coalesced read of
//      the row-major copy instead of three kernels that each walk it through global memory): S <= PF_ROWS rows,
//      n <= PF_COLS columns, S * pitch <= PF_CELLS bytes, n / max(L-1, 1) + 4 <= PF_STACK (the host checks; the entry
//      point documents it).  No global scratch: masks, gap runs, stacks and per-interval flags are LDS.
#define PF_ROWS 512
#define PF_COLS 1024
#define PF_CELLS 8192
#define PF_STACK 128
#define PF_ITEMS 8                    // 4-byte pieces a thread keeps in flight while a small view is loaded
MPRG_DEV int pf_pitch(int n) { int p = (n + 3) & ~3; if (((p >> 2) & 1) == 0) p += 4; return p; }   // odd number of LDS words per row
// K2w  the same for a SMALL view by ONE wavefront, PW_WAVES views per workgroup (the rule from the second recursion level on: a
//      level of 7 500 alignments holds ~300 000 views of a few hundred cells; one workgroup per view costs ~16 us of launch,
//      barriers and one thread's walk whatever the view holds, with six views resident per CU): n <= 64 columns (a lane per
//      column), the cells in PW_CELLS bytes of LDS, no workgroup barrier anywhere — a wavefront's LDS accesses are ordered by
//      WAVE_SYNC, the serial walks are lane 0's.  Same phases, same code (pt_phases<.., WV>), same answers.
#define PW_WAVES 4
#define PW_CELLS 4096
#define PW_ROWS 256
#define PW_STACK 32
MPRG_DEV bool pw_is_small(long long S, long long n, int L) {
  return S >= 1 && n >= 1 && n <= WAVE && S <= PW_ROWS && S * pf_pitch((int)n) <= PW_CELLS && n / (L > 1 ? L - 1 : 1) + 4 <= PW_STACK;
}
KERNEL(k_partition_fused, const int32_t *view_list, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, int L,
       int32_t *iv_all, int32_t *n_iv_out, int32_t *status_out, int32_t *view_out, int wave_form, DsCount dc) {
  DS_GUARD(dc, 1);
  KM_T0();
  const int v = view_list[BLOCK_ID];
  const ViewD d = load_view(views, v);
  const int n = d.n_cols, S = d.n_rows, cpitch = pf_pitch(n);
  if (wave_form && pw_is_small(S, n, L)) return;          // k_partition_wave's (same list, launched beside this kernel)
  // the launch shape's preconditions (include/mprg.h), checked here too: a view that breaks them would run over the LDS arrays
  if (S > PF_ROWS || n > PF_COLS || n < 1 || S < 1 || (long long)S * cpitch > PF_CELLS || n / (L > 1 ? L - 1 : 1) + 4 > PF_STACK) {
    ONE_THREAD {
      n_iv_out[v] = 0; status_out[v] = MPRG_ST_BAD_LAUNCH;
      if (view_out) { int32_t *o = view_out + 8 * (long long)v; o[0] = 0; o[1] = MPRG_ST_BAD_LAUNCH; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0; }
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) uint8_t cells_s[PF_CELLS];
  SHARED(uint32_t, mask_s, PF_COLS);
  SHARED(uint32_t, maxrun_s, PF_COLS);
  SHARED(int32_t, stk_s, 4 * PF_STACK);
  SHARED(uint8_t, nmz_s, 24 * PF_STACK);            // n <= PF_COLS <= 24 * PF_STACK bytes; later 2 * PF_STACK triples
  SHARED(int32_t, ntype_s, PF_STACK);
  SHARED(int32_t, flagm_s, PF_STACK);
  SHARED(int32_t, refrow_s, PF_STACK);
  SHARED(int, sh, 8);
  ONE_THREAD { sh[0] = 0; sh[1] = 0; sh[2] = 0; sh[3] = 0; sh[4] = 0; sh[5] = 0; sh[6] = 0; sh[7] = 0; }
  PAR_FOR(c, n) { mask_s[c] = 0; maxrun_s[c] = 0; }
  // the view's cells into LDS.  A small view is a handful of KB: what this costs is ROUND TRIPS, not bytes — so the row
  // indices come in first (one coalesced read), and then every thread fetches its 4-byte pieces (item = row x 4 columns)
  // with all its loads in flight at once (PF_ITEMS independent items per thread and pass)
  __shared__ int32_t rows_s[PF_ROWS];
  PAR_FOR(i, S) { rows_s[i] = view_row(d, rowidx, i); }
  BARRIER(); KM_T(23);
  {
    const int cpr = (n + 3) >> 2;                     // 4-byte pieces per row
    const int items = S * cpr;
    const uint8_t *src0 = arena + d.rm + d.col0;
    for (int e0 = (int)threadIdx.x; e0 < items; e0 += PF_ITEMS * N_THREADS) {
      uint32_t w[PF_ITEMS];
      int at[PF_ITEMS];
#pragma unroll
      for (int q = 0; q < PF_ITEMS; ++q) {
        const int e = e0 + q * N_THREADS;
        at[q] = -1;
        w[q] = 0;
        if (e < items) {
          const int i = (int)((unsigned)e / (unsigned)cpr), c4 = ((int)((unsigned)e % (unsigned)cpr)) << 2;
          __builtin_memcpy(&w[q], src0 + (long long)rows_s[i] * d.pitchC + c4, 4);   // the arena is padded: reading past n is harmless
          at[q] = i * cpitch + c4;
        }
      }
#pragma unroll
      for (int q = 0; q < PF_ITEMS; ++q) if (at[q] >= 0) *(uint32_t *)(cells_s + at[q]) = w[q];      // cpitch % 4 == 0
    }
  }
  BARRIER(); KM_T(24);
  {                                                 // K1: presence masks; item = (4 adjacent columns, row slice): small views
    const int cpr = (n + 3) >> 2;                   // are a few dozen columns wide, so columns alone would idle most lanes
    int slices = N_THREADS / cpr;
    slices = slices < 1 ? 1 : (slices > S ? (S > 0 ? S : 1) : slices);
    for (int e = (int)threadIdx.x; e < cpr * slices; e += N_THREADS) {
      const int g = (int)((unsigned)e % (unsigned)cpr), sl = (int)((unsigned)e / (unsigned)cpr);
      uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
      for (int i = sl; i < S; i += slices) {
        const uint32_t w = *(const uint32_t *)(cells_s + i * cpitch + 4 * g);
        m0 |= 1u << (w & 31u); m1 |= 1u << ((w >> 8) & 31u); m2 |= 1u << ((w >> 16) & 31u); m3 |= 1u << ((w >> 24) & 31u);
      }
      const int c = 4 * g;
      atomicOr(&mask_s[c], m0);
      if (c + 1 < n) atomicOr(&mask_s[c + 1], m1);
      if (c + 2 < n) atomicOr(&mask_s[c + 2], m2);
      if (c + 3 < n) atomicOr(&mask_s[c + 3], m3);
    }
  }
  BARRIER();
  PAR_FOR(c, n) {
    const uint32_t m = mask_s[c];
    if (m & BIT_N) sh[4] = 1;
    if (m & BITS_IUPAC) sh[5] = 1;
    const uint32_t mm = m & ~BIT_N;
    const bool star = !(mm != 0 && (mm & (mm - 1)) == 0 && (mm & BITS_IUPAC) == 0 && mm != BIT_GAP);
    if (star) sh[0] = 1;
    nmz_s[c] = star ? 1 : 0;
    if (m & BIT_GAP) sh[1] = 1;                     // (sh[1] is reset by the scan below)
  }
  BARRIER(); KM_T(25);
  if (sh[1]) {                                      // K2a: longest all-gap run ending at each column
    PAR_FOR(i, S) {
      uint32_t run = 0;
      for (int c = 0; c < n; ++c) {
        if (cells_s[i * cpitch + c] == C_GAP) { ++run; ATOMIC_MAX(maxrun_s + c, run); } else run = 0;
      }
    }
  }
  BARRIER(); KM_T(16);
  int32_t *iv = iv_all + 3 * d.col_off;
  pt_phases<true, true>(arena, d, rowidx, mask_s, L, maxrun_s, nullptr, flagm_s, refrow_s, iv, stk_s, PF_STACK, nmz_s,
                        24 * PF_STACK, ntype_s, sh, cells_s, cpitch KM_TARG);
  pt_outputs(v, sh, true, nmz_s, iv, n_iv_out, status_out, view_out KM_TARG);
  KM_T(21);
}

struct PwLds {
  __attribute__((aligned(16))) uint8_t cells[PW_CELLS];
  union {
    int32_t rows[PW_ROWS];             // the view's MSA rows: only while the cells come in
    struct { uint32_t maxrun[WAVE]; int32_t stk[4 * PW_STACK]; int32_t ntype[PW_STACK]; int32_t flagm[PW_STACK]; int32_t refrow[PW_STACK]; } t;
  } u;
  __attribute__((aligned(4))) uint8_t nmz[24 * PW_STACK];      // non-match bytes of the columns; later up to 2 * PW_STACK triples
  int sh[8];
};
KERNEL(k_partition_wave, const int32_t *view_list, const uint8_t *arena, const int64_t *views, const int32_t *rowidx, int L,
       int32_t *iv_all, int32_t *n_iv_out, int32_t *status_out, int32_t *view_out, int n_list, DsCount dc) {
  KM_T0();
  __shared__ PwLds lds_all[PW_WAVES];
  const long long slot = (long long)BLOCK_ID * PW_WAVES + wave_id();
  if (slot >= ds_n(dc, n_list)) return;               // (per wavefront: nothing below waits for the workgroup)
  const int v = view_list[slot];
  const ViewD d = load_view(views, v);
  const int n = d.n_cols, S = d.n_rows, cpitch = pf_pitch(n);
  if (!pw_is_small(S, n, L)) return;                  // k_partition_fused's
  PwLds &ld = lds_all[wave_id()];
  const int lane = wave_lane();
  int *sh = ld.sh;
  if (lane < 8) sh[lane] = 0;
  for (int i = lane; i < S; i += WAVE) ld.u.rows[i] = view_row(d, rowidx, i);
  WAVE_SYNC();
  {                                                   // the cells: item = (row, 4 columns), PF_ITEMS loads in flight per lane
    const int cpr = (n + 3) >> 2, items = S * cpr;
    const uint8_t *src0 = arena + d.rm + d.col0;
    for (int e0 = lane; e0 < items; e0 += PF_ITEMS * WAVE) {
      uint32_t w[PF_ITEMS];
      int at[PF_ITEMS];
#pragma unroll
      for (int q = 0; q < PF_ITEMS; ++q) {
        const int e = e0 + q * WAVE;
        at[q] = -1; w[q] = 0;
        if (e < items) {
          const int i = (int)((unsigned)e / (unsigned)cpr), c4 = ((int)((unsigned)e % (unsigned)cpr)) << 2;
          __builtin_memcpy(&w[q], src0 + (long long)ld.u.rows[i] * d.pitchC + c4, 4);      // the arena is padded: reading past n is harmless
          at[q] = i * cpitch + c4;
        }
      }
#pragma unroll
      for (int q = 0; q < PF_ITEMS; ++q) if (at[q] >= 0) *(uint32_t *)(ld.cells + at[q]) = w[q];
    }
  }
  WAVE_SYNC();                                        // (the rows are done with: their place is the tables' from here on)
  // lane = (column c, row slice sl): p2 = columns rounded up to a power of two, 64 / p2 slices of rows side by side
  int lg = 0;
  while ((1 << lg) < n) ++lg;
  const int p2 = 1 << lg, slices = WAVE >> lg, c = lane & (p2 - 1), sl = lane >> lg;
  const bool col = c < n;
  uint32_t m = 0;
  if (col) for (int i = sl; i < S; i += slices) m |= 1u << (ld.cells[i * cpitch + c] & 31u);
  for (int off = p2; off < WAVE; off <<= 1) m |= (uint32_t)__shfl_xor((int)m, off);
  const uint32_t mm = m & ~BIT_N;
  const bool star = col && !(mm != 0 && (mm & (mm - 1)) == 0 && (mm & BITS_IUPAC) == 0 && mm != BIT_GAP);
  const bool first = col && sl == 0;
  const bool any_star = __ballot(first && star) != 0, any_n = __ballot(first && (m & BIT_N)) != 0;
  const bool any_iupac = __ballot(first && (m & BITS_IUPAC)) != 0, any_gap = __ballot(first && (m & BIT_GAP)) != 0;
  if (first) ld.nmz[c] = star ? 1 : 0;
  // K2a: longest all-gap run ending at each column: a row's gap cells as bits of a ballot, the run ending at column c = the
  // distance to the nearest bit below c that is not set
  uint32_t mr = 0;
  if (any_gap) {
    const unsigned long long seg_mask = p2 == WAVE ? ~0ull : ((1ull << p2) - 1ull);
    for (int i0 = 0; i0 < S; i0 += slices) {           // uniform trip count: every lane votes
      const int i = i0 + sl;
      const bool gap = col && i < S && ld.cells[i * cpitch + c] == C_GAP;
      const unsigned long long g = (__ballot(gap) >> (sl * p2)) & seg_mask;
      if (gap) {
        const unsigned long long z = ~g & ((c == WAVE - 1) ? ~0ull : ((2ull << c) - 1ull));      // no-gap columns at or below c
        const uint32_t run = z ? (uint32_t)(c - (63 - __clzll((long long)z))) : (uint32_t)(c + 1);
        mr = run > mr ? run : mr;
      }
    }
    for (int off = p2; off < WAVE; off <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)mr, off); mr = o > mr ? o : mr; }
  }
  if (first) ld.u.t.maxrun[c] = mr;
  if (lane == 0) { sh[0] = any_star; sh[4] = any_n; sh[5] = any_iupac; }
  WAVE_SYNC(); KM_T(16);
  int32_t *iv = iv_all + 3 * d.col_off;
  pt_phases<true, true, true>(arena, d, rowidx, nullptr, L, ld.u.t.maxrun, nullptr, ld.u.t.flagm, ld.u.t.refrow, iv, ld.u.t.stk, PW_STACK,
                              ld.nmz, 24 * PW_STACK, ld.u.t.ntype, sh, ld.cells, cpitch KM_TARG);
  pt_outputs<true>(v, sh, true, ld.nmz, iv, n_iv_out, status_out, view_out KM_TARG);
}
