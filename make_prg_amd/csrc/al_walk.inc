// Lane 0's walk back through the traceback from (n, C) in state H, the ops (reversed) and the {status, score, count} triple: written
// once, included as text at the end of each of the four sweep kernels.  The kernel provides kBand (the strips of a banded kernel
// start at column sc = max(0, i0 + dlo), and t counts steps from there), dlo (0 where not kBand), tb, nst8, ops, opoff, o, score, ni, Ci.
  if (lane == 0) {
    uint8_t *op = ops + opoff;
    long long k = 0;
    int i = ni, j = Ci, st = 0;                              // st: 0 H, 1 D, 2 I
    while (i > 0 && j > 0) {
      const int rr = i - 1, l = rr & 63, sc = kBand && (rr & ~63) + dlo > 0 ? (rr & ~63) + dlo : 0, t = j - 1 - sc + l;
      const unsigned cell = (tb[((long long)(rr >> 6) * nst8 + (t >> 3)) * 64 + l] >> (4 * (t & 7))) & 15u;
      if (st == 0) {
        if ((cell & 3u) == 0) { op[k++] = 'M'; --i; --j; }
        else st = (int)(cell & 3u);
      } else if (st == 1) { op[k++] = 'D'; --j; st = (cell & 4u) ? 1 : 0; }
      else { op[k++] = 'I'; --i; st = (cell & 8u) ? 2 : 0; }
    }
    for (; j > 0; --j) op[k++] = 'D';                        // row 0: only Y's columns alone lead back to (0, 0); column 0: only X's
    for (; i > 0; --i) op[k++] = 'I';
    o[0] = MPRG_AL_OK; o[1] = score; o[2] = (int32_t)k;
  }
