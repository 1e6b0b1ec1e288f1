// The body of the two centre kernels, below their LDS declarations (tot, hist, red, bad).  Included as text (DESIGN.md §3a); the
// kernel provides its parameters and ST_BIN(k), the bin a window of index k counts in: k itself, or st_canonical(k).
  const int64_t *L = loci + MPRG_ST_LOCUS_FIELDS * (long long)BLOCK_ID;
  const long long first = L[0], m = L[1];
  ONE_THREAD {
#define ST_ALSO_BAD false
#include "st_seqs_serial.inc"
#undef ST_ALSO_BAD
    bad[0] = b;
    if (b) centre[BLOCK_ID] = MPRG_ST_CENTRE_BAD;
  }
  BARRIER();
  if (bad[0]) return;                                        // (the whole workgroup)
  PAR_FOR(b, ST_BINS) tot[b] = 0;
  BARRIER();
  for (long long a = 0; a < m; ++a) {
    const long long off = seqs[2 * (first + a)], n = seqs[2 * (first + a) + 1];
    PAR_FOR(w, n - (ST_K - 1)) {
#include "st_window.inc"
      if (valid) ATOMIC_ADD(&tot[ST_BIN(k)], 1u);
    }
  }
  BARRIER();
  long long best = 0;
  int best_a = -1;
  for (long long a = 0; a < m; ++a) {
    const long long off = seqs[2 * (first + a)], n = seqs[2 * (first + a) + 1];
    PAR_FOR(b, ST_BINS) hist[b] = 0;
    BARRIER();
    PAR_FOR(w, n - (ST_K - 1)) {
#include "st_window.inc"
      if (valid) ATOMIC_ADD(&hist[ST_BIN(k)], 1u);
    }
    BARRIER();
    long long part = 0;
    PAR_FOR(w, n - (ST_K - 1)) {
#include "st_window.inc"
      if (valid) { const unsigned b = ST_BIN(k); part += (long long)tot[b] - (long long)hist[b]; }
    }
#include "wg_sum.inc"
    ONE_THREAD {
      WG_TOTAL(s, ST_WAVES);
      if (n > 0 && (best_a < 0 || s > best)) { best = s; best_a = (int)a; }
    }
    BARRIER();                                               // (hist and red are rewritten for the next sequence)
  }
  ONE_THREAD centre[BLOCK_ID] = best_a;                     // -1: every sequence is empty
