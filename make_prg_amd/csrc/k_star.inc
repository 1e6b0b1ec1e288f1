// ---------------------------------------------------------------------------------------------------------------
// K-S  centre-star MSAs of `from_msa --unaligned` (make_prg_amd/from_msa/star_align.py holds the spec; DESIGN.md §3b).
//      The pairs themselves are k_align_pairs' (K-A): the centre is a 1-row leaf, every other sequence a new sequence.
//
// k_star_kmer_centre: one workgroup per locus.  T (the locus's 6-mer counts over ACGT, 4096 bins) is built in LDS from every
//   window of every sequence; then, sequence by sequence, its own histogram c_a in a second 16 KB of LDS and
//   score(a) = <c_a, T> - <c_a, c_a> = sum over a's windows w of (T[k_w] - c_a[k_w]) in int64, a block reduction, and the
//   argmax with the lowest-index tie rule over the non-empty sequences.  Integers only.
// k_star_kmer_centre_canonical (`--adjust-direction`): the same body with every window counted in the bin min(k, rc6(k)), so the
//   centre it picks does not change when any subset of the locus's sequences is reverse-complemented.
// k_star_strand: one workgroup per locus.  The forward 6-mer histogram h of the locus's centre sequence (as stored) is built once
//   in 16 KB of LDS and then only read: the wavefronts take the locus's sequences round-robin, the lanes stride over a sequence's
//   windows, a valid window adds h[k] to fwd, h[rc6(k)] to rev and 1 to nw; a wave reduction, lane 0 writes the three int64.
//   The reference orientation of the spec may be the centre's reverse complement: h_rc(s)[k] = h_s[rc6(k)], so the HOST swaps
//   fwd and rev for such a locus instead of the kernel reading a reversed centre.
// k_star_revcomp: one wavefront per job: the reverse complement of a sequence written elsewhere in the same code buffer (the
//   buffer's tail), consecutive lanes on consecutive bytes of both.
// k_star_merge_widths: one wavefront per row of a locus that came out of the pair kernel.  The row's ops (stored reversed) are
//   read forward in 64-op chunks; wave scans give each op its boundary / column (non-I ops before it), its residue index (non-D
//   ops before it) and, for an I, its rank in the run of I's at that boundary; atomicMax(width[boundary], rank + 1).
// k_star_merge_columns: one wavefront per locus: start[j] = sum over j' < j of (width[j'] + 1), the output width W.
// k_star_merge_rows: one wavefront per row: every byte of the output row is written exactly once (no fill pass to order
//   against): a column op writes its column and the '-' padding of the boundary before it, an I its residue at its rank,
//   the trailing boundary's padding after the walk.  Centre and empty rows (ops count -1) place residue i at column i.
// ---------------------------------------------------------------------------------------------------------------
#define ST_THREADS 256
#define ST_WAVES (ST_THREADS / 64)
#define ST_K 6
#define ST_BINS 4096

// reverse complement of a 6-mer index: complement (4095 - k), then the six 2-bit groups in reverse order
MPRG_DEV unsigned st_rc6(unsigned k) {
  k = ~k & (ST_BINS - 1);
  unsigned r = 0;
#pragma unroll
  for (int q = 0; q < ST_K; ++q) r = (r << 2) | ((k >> (2 * q)) & 3u);
  return r;
}
KERNEL(k_star_kmer_centre, const uint8_t *codes, long long codes_bytes, const int64_t *seqs, long long n_seqs, const int64_t *loci,
       int32_t *centre) {
  SHARED(uint32_t, tot, ST_BINS);
  SHARED(uint32_t, hist, ST_BINS);
  SHARED(long long, red, ST_WAVES);
  SHARED(int, bad, 1);
#define ST_BIN(k) (k)
#include "st_centre.inc"
#undef ST_BIN
}

// the strand-blind bin of a window: the smaller of its index and its reverse complement's
MPRG_DEV unsigned st_canonical(unsigned k) {
  const unsigned r = st_rc6(k);
  return r < k ? r : k;
}

// k_star_kmer_centre with canonical bins.  A kernel of its own whose body is the same text (st_centre.inc), not a shared function:
// an inlined common body compiles k_star_kmer_centre differently, the included text leaves both kernels the instructions they had
// (DESIGN.md §3a), so a run without --adjust-direction launches what it always did.
KERNEL(k_star_kmer_centre_canonical, const uint8_t *codes, long long codes_bytes, const int64_t *seqs, long long n_seqs,
       const int64_t *loci, int32_t *centre) {
  SHARED(uint32_t, tot, ST_BINS);
  SHARED(uint32_t, hist, ST_BINS);
  SHARED(long long, red, ST_WAVES);
  SHARED(int, bad, 1);
#define ST_BIN(k) st_canonical(k)
#include "st_centre.inc"
#undef ST_BIN
}

KERNEL(k_star_strand, const uint8_t *codes, long long codes_bytes, const int64_t *seqs, long long n_seqs, const int64_t *loci,
       const int32_t *centre, int64_t *evidence, int32_t *status) {
  SHARED(uint32_t, href, ST_BINS);
  SHARED(int, bad, 1);
  const int64_t *L = loci + MPRG_ST_LOCUS_FIELDS * (long long)BLOCK_ID;
  const long long first = L[0], m = L[1], c = centre[BLOCK_ID];
  ONE_THREAD {
#define ST_ALSO_BAD c < 0 || c >= m
#include "st_seqs_serial.inc"
#undef ST_ALSO_BAD
    bad[0] = b;
    status[BLOCK_ID] = b ? MPRG_ST_CENTRE_BAD : MPRG_ST_OK;
  }
  PAR_FOR(b, ST_BINS) href[b] = 0;
  BARRIER();
  if (bad[0]) return;                                        // (the whole workgroup; no triple written)
  {
    const long long off = seqs[2 * (first + c)], n = seqs[2 * (first + c) + 1];
    PAR_FOR(w, n - (ST_K - 1)) {
#include "st_window.inc"
      if (valid) ATOMIC_ADD(&href[k], 1u);
    }
  }
  BARRIER();                                                 // href is read-only from here on: no barrier, no LDS write below
  for (long long a = wave_id(); a < m; a += ST_WAVES) {
    const long long off = seqs[2 * (first + a)], n = seqs[2 * (first + a) + 1];
    long long fwd = 0, rev = 0, nw = 0;
    for (long long w = wave_lane(); w < n - (ST_K - 1); w += WAVE) {
#include "st_window.inc"
      if (valid) { fwd += href[k]; rev += href[st_rc6(k)]; ++nw; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { fwd += __shfl_xor(fwd, d); rev += __shfl_xor(rev, d); nw += __shfl_xor(nw, d); }
    if (wave_lane() == 0) {
      int64_t *e = evidence + 3 * (first + a);
      e[0] = fwd; e[1] = rev; e[2] = nw;
    }
  }
}

// a wavefront per job {source offset, n, destination offset}: dst[i] = complement of src[n - 1 - i], both inside `codes`
__global__ void __launch_bounds__(ST_THREADS) k_star_revcomp(uint8_t *codes, long long codes_bytes, const int64_t *jobs, int n_jobs,
                                                             int32_t *status) {
  const long long j = (long long)BLOCK_ID * ST_WAVES + wave_id();
  if (j >= n_jobs) return;                                   // (a whole wavefront)
  const long long src = jobs[3 * j], n = jobs[3 * j + 1], dst = jobs[3 * j + 2];
  const bool ok = src >= 0 && n >= 0 && dst >= 0 && src + n <= codes_bytes && dst + n <= codes_bytes && (dst >= src + n || dst + n <= src);
  if (wave_lane() == 0) status[j] = ok ? MPRG_ST_OK : MPRG_ST_BAD_ROW;
  if (!ok) return;
  // ACGT-RYKMSWN: A<->T, C<->G, R<->Y, K<->M; '-', S, W, N and anything else stay
  for (long long i = wave_lane(); i < n; i += WAVE) {
    const unsigned x = codes[src + n - 1 - i];
    codes[dst + i] = (uint8_t)(x < 4u ? 3u - x : x == 5u || x == 7u ? x + 1u : x == 6u || x == 8u ? x - 1u : x);
  }
}

// inclusive max-scan over the lanes of a wave (all 64 lanes call it)
MPRG_DEV long long st_wave_max_incl(long long v) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) { const long long y = __shfl_up(v, d); if (wave_lane() >= d && y > v) v = y; }
  return v;
}

// One forward op of a row, as a wave-wide chunk step: the op at forward index q (q < k), its boundary / column `col`, residue
// index `res`, and `rank`: the I's immediately before it (for an I, its place in its run; for a column op, the I's of the boundary
// before its column).  The carries (columns, residues, index of the last non-I op) advance by the chunk.
struct StOp { unsigned op; long long col, res, rank; };
MPRG_DEV StOp st_op_step(const uint8_t *ops, long long ops_off, long long k, long long q0, long long &c_col, long long &c_res,
                         long long &c_last) {
  const long long q = q0 + wave_lane();
  const bool valid = q < k;
  const unsigned op = valid ? (unsigned)ops[ops_off + k - 1 - q] : (unsigned)'M';
  const int inc_c = valid && op != 'I', inc_r = valid && op != 'D';
  const int sc = wave_scan_incl(inc_c), sr = wave_scan_incl(inc_r);
  const long long last_incl = st_wave_max_incl(inc_c ? q : -1);
  long long prev = __shfl_up(last_incl, 1);
  if (wave_lane() == 0) prev = -1;
  const long long last_excl = prev > c_last ? prev : c_last;
  StOp r;
  r.op = op;
  r.col = c_col + sc - inc_c;
  r.res = c_res + sr - inc_r;
  r.rank = q - last_excl - 1;
  c_col += __shfl(sc, 63);
  c_res += __shfl(sr, 63);
  const long long l63 = __shfl(last_incl, 63);
  if (l63 > c_last) c_last = l63;
  return r;
}

// a row's fields against the buffers: locus in range, its width / start range inside n_width, the sequence inside the codes,
// the ops inside the ops buffer and their count possible for n residues against C columns (k = n + C - #M); k < 0: n <= C
MPRG_DEV bool st_row_ok(const int64_t *R, const int64_t *loci, int n_loci, long long n_width, long long codes_bytes,
                        long long ops_bytes, long long &C, long long &woff) {
  const long long l = R[0], soff = R[1], n = R[2], ops_off = R[3], k = R[4];
  if (l < 0 || l >= n_loci) return false;
  C = loci[MPRG_ST_LOCUS_FIELDS * l + 2];
  woff = loci[MPRG_ST_LOCUS_FIELDS * l + 3];
  if (C < 1 || woff < 0 || woff + C + 1 > n_width || n < 0 || soff < 0 || soff + n > codes_bytes) return false;
  if (k < 0) return n <= C;
  return ops_off >= 0 && ops_off + k <= ops_bytes && k >= (n > C ? n : C) && k <= n + C;
}

__global__ void __launch_bounds__(ST_THREADS) k_star_merge_widths(const uint8_t *ops, long long ops_bytes, const int64_t *rows,
                                                                  int n_rows, const int64_t *loci, int n_loci, int32_t *width,
                                                                  long long n_width, long long codes_bytes, int32_t *status) {
  const long long r = (long long)BLOCK_ID * ST_WAVES + wave_id();
  if (r >= n_rows) return;                                   // (a whole wavefront)
  const int64_t *R = rows + MPRG_ST_ROW_FIELDS * r;
  long long C = 0, woff = 0;
  if (!st_row_ok(R, loci, n_loci, n_width, codes_bytes, ops_bytes, C, woff)) {
    if (wave_lane() == 0) status[r] = MPRG_ST_BAD_ROW;
    return;
  }
  const long long n = R[2], ops_off = R[3], k = R[4];
  long long c_col = 0, c_res = 0, c_last = -1;
  bool bad = false;
  if (k > 0) {
    for (long long q0 = 0; q0 < k; q0 += WAVE) {
      const StOp o = st_op_step(ops, ops_off, k, q0, c_col, c_res, c_last);
      if (q0 + wave_lane() >= k) continue;
      if (o.op == 'I') {
        if (o.col > C || o.res >= n) bad = true;
        else ATOMIC_MAX(&width[woff + o.col], (int32_t)(o.rank + 1));
      } else if (o.op == 'M' || o.op == 'D') {
        if (o.col >= C || (o.op == 'M' && o.res >= n)) bad = true;
      } else bad = true;
    }
    if (c_col != C || c_res != n) bad = true;
  }
  bad = __ballot(bad) != 0ull;
  if (wave_lane() == 0) status[r] = bad ? MPRG_ST_BAD_ROW : MPRG_ST_OK;
}

__global__ void __launch_bounds__(ST_THREADS) k_star_merge_columns(const int64_t *loci, int n_loci, const int32_t *width,
                                                                   int64_t *start, long long n_width, int64_t *out_width) {
  const long long l = (long long)BLOCK_ID * ST_WAVES + wave_id();
  if (l >= n_loci) return;
  const long long C = loci[MPRG_ST_LOCUS_FIELDS * l + 2], woff = loci[MPRG_ST_LOCUS_FIELDS * l + 3];
  if (C < 1 || woff < 0 || woff + C + 1 > n_width) { if (wave_lane() == 0) out_width[l] = -1; return; }
  long long carry = 0;
  for (long long j0 = 0; j0 <= C; j0 += WAVE) {
    const long long j = j0 + wave_lane();
    const long long v = j <= C ? (long long)width[woff + j] + 1 : 0;
    const long long incl = wave_scan_incl_ll(v);
    if (j <= C) start[woff + j] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (wave_lane() == 0) out_width[l] = carry - 1;              // C + sum of the widths (boundary C has no column after it)
}

__global__ void __launch_bounds__(ST_THREADS) k_star_merge_rows(const uint8_t *codes, long long codes_bytes, const uint8_t *ops,
                                                                long long ops_bytes, const int64_t *rows, int n_rows,
                                                                const int64_t *loci, int n_loci, const int32_t *width,
                                                                const int64_t *start, long long n_width, const int64_t *out_width,
                                                                uint8_t *out, long long out_bytes, int32_t *status) {
  const long long r = (long long)BLOCK_ID * ST_WAVES + wave_id();
  if (r >= n_rows) return;
  const int64_t *R = rows + MPRG_ST_ROW_FIELDS * r;
  long long C = 0, woff = 0;
  if (!st_row_ok(R, loci, n_loci, n_width, codes_bytes, ops_bytes, C, woff)) {
    if (wave_lane() == 0) status[r] = MPRG_ST_BAD_ROW;
    return;
  }
  const long long soff = R[1], n = R[2], ops_off = R[3], k = R[4], ooff = R[5], W = out_width[R[0]];
  if (ooff < 0 || W < C || ooff + W > out_bytes) { if (wave_lane() == 0) status[r] = MPRG_ST_NO_SPACE; return; }
  const char *abc = "ACGT-RYKMSWN";
  const int32_t *wd = width + woff;
  const int64_t *st = start + woff;
  uint8_t *o = out + ooff;
  bool bad = false;
  auto pad = [&](long long j, long long from) {             // boundary j's slots from `from` on: '-'
    const long long w = wd[j];
    if (from > w) { bad = true; return; }
    for (long long x = from; x < w; ++x) o[st[j] + x] = '-';
  };
  if (k < 0) {
    for (long long c = wave_lane(); c <= C; c += WAVE) {
      pad(c, 0);
      if (c < C) o[st[c] + wd[c]] = c < n ? (uint8_t)abc[codes[soff + c] < 12 ? codes[soff + c] : 4] : (uint8_t)'-';
    }
  } else {
    long long c_col = 0, c_res = 0, c_last = -1;
    for (long long q0 = 0; q0 < k; q0 += WAVE) {
      const StOp p = st_op_step(ops, ops_off, k, q0, c_col, c_res, c_last);
      if (q0 + wave_lane() >= k) continue;
      if ((p.op != 'M' && p.op != 'I' && p.op != 'D') || p.col > C || (p.op != 'D' && p.res >= n)) { bad = true; continue; }
      const uint8_t ch = p.op == 'D' ? (uint8_t)'-' : (uint8_t)abc[codes[soff + p.res] < 12 ? codes[soff + p.res] : 4];
      if (p.op == 'I') {
        if (p.rank >= wd[p.col]) bad = true;
        else o[st[p.col] + p.rank] = ch;
      } else if (p.col >= C) bad = true;
      else { pad(p.col, p.rank); o[st[p.col] + wd[p.col]] = ch; }
    }
    if (c_col != C || c_res != n) bad = true;                // (as k_star_merge_widths: a column or a residue too few)
    if (wave_lane() == 0 && !bad) pad(C, k - 1 - c_last);    // the I's after the last column op
  }
  bad = __ballot(bad) != 0ull;
  if (wave_lane() == 0) status[r] = bad ? MPRG_ST_BAD_ROW : MPRG_ST_OK;
}
