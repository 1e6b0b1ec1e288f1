// One 6-mer window, what the centre rule, the strand evidence and the tree distances all mean by it.  Included as text inside the
// loop over a sequence's windows (DESIGN.md §3a); the kernel provides codes, off, w.  Defines k, the index of the window
// codes[off + w .. off + w + 5] (2 bits per code, the first code highest), and valid: all six codes are A, C, G or T.
      unsigned k = 0;
      bool valid = true;
#pragma unroll
      for (int q = 0; q < ST_K; ++q) { const unsigned code = codes[off + w + q]; valid = valid && code < 4u; k = (k << 2) | (code & 3u); }
