// The planes of one column, from its counts: what the DP kernels read, the truncation toward zero of a negative numerator
// included.  Included as text (DESIGN.md §3a); the kernel provides cnt[0 .. 4] (A C G T '-'), acgt and gap (long long), pl_rows,
// the divisor (the rows counted), and pl_stride, the words between two planes (both int or long long, as the kernel holds them), o,
// the column's word of plane 0, and kind.  Kind 0 writes Y's six planes: the scores of A C G T, of an ambiguity code and of a gap in X against the column.
// Kind 2 writes those six and Oc, what a run that starts by skipping the column pays (star_align.py, "Position gaps").
// Kind 1 writes X's seven: the counts of A C G T, of the ambiguity codes, of '-', and Ic, the cost of the column alone.
    if (kind != 1) {
#pragma unroll
      for (int x = 0; x < 4; ++x) o[(long long)x * pl_stride] = (int32_t)(64 * (20 * cnt[x] - 9 * (acgt - cnt[x]) - 10 * gap) / pl_rows);
      o[4LL * pl_stride] = (int32_t)(64 * (-10 * gap) / pl_rows);
      o[5LL * pl_stride] = (int32_t)(64 * (-10 * (pl_rows - gap)) / pl_rows);
      if (kind == 2) o[6LL * pl_stride] = (int32_t)(64 * (-11 * (pl_rows - gap)) / pl_rows);
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x) o[(long long)x * pl_stride] = (int32_t)cnt[x];
      o[4LL * pl_stride] = (int32_t)(pl_rows - acgt - gap);
      o[5LL * pl_stride] = (int32_t)gap;
      o[6LL * pl_stride] = (int32_t)(64 * (-10 * (pl_rows - gap)) / pl_rows);
    }
