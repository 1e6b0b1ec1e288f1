// A locus's sequence table against the code buffer, by the whole workgroup.  Included as text (DESIGN.md §3a); the kernel provides
// first, m, seqs, codes_bytes, the LDS word bad[0] and ok, its own checks of the locus's fields (workgroup-uniform; the sequences
// are only read when it holds).  Behind the closing barrier bad[0] is non-zero when !ok or a sequence leaves the code buffer.
  ONE_THREAD bad[0] = !ok;
  BARRIER();
  if (ok) {
    int b = 0;
    PAR_FOR(x, m) {
      const long long off = seqs[2 * (first + x)], n = seqs[2 * (first + x) + 1];
      b |= off < 0 || n < 0 || off > codes_bytes || n > codes_bytes - off;
    }
    if (b) ATOMIC_OR(&bad[0], 1);
  }
  BARRIER();
