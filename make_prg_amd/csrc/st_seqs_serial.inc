// A locus's sequence table against the code buffer, by one thread.  Included as text (DESIGN.md §3a); the kernel provides first,
// m, seqs, n_seqs, codes_bytes and ST_ALSO_BAD, its own further refusals: the end of the || chain below, so clauses joined by ||
// and no brackets around them (false: none).  Defines b: non-zero when the locus's range leaves the table, a sequence leaves the
// code buffer, or ST_ALSO_BAD.
    int b = first < 0 || m < 0 || first + m > n_seqs || ST_ALSO_BAD;
    for (long long a = 0; !b && a < m; ++a) b = seqs[2 * (first + a)] < 0 || seqs[2 * (first + a) + 1] < 0 ||
                                               seqs[2 * (first + a)] + seqs[2 * (first + a) + 1] > codes_bytes;
