// The five counts A C G T '-' of one column of a text of cell codes, rows walked in order.  Included as text (DESIGN.md §3a); the
// kernel provides R, the text's rows (r walks them in R's own type, int or long long), AL_CELL(r), the column's cell in row r,
// and AL_WEIGHT(r), the times row r counts (1: a plain text).  Defines cnt[5], and in long long acgt = cnt[0] + .. + cnt[3] and
// gap = cnt[4].
    int cnt[5] = {0, 0, 0, 0, 0};
    for (decltype(+R) r = 0; r < R; ++r) {
      const unsigned code = AL_CELL(r);
      const int w = AL_WEIGHT(r);
#pragma unroll
      for (int q = 0; q < 5; ++q) cnt[q] += code == (unsigned)q ? w : 0;
    }
    const long long acgt = (long long)cnt[0] + cnt[1] + cnt[2] + cnt[3], gap = cnt[4];
