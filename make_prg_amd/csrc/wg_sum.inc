// The workgroup's sum of a long long per thread, up to the barrier.  Included as text (DESIGN.md §3a); the kernel provides part,
// this thread's term, and red, LDS of a long long per wavefront.  Behind the closing barrier red[w] is wavefront w's sum; the
// threads that need the total declare it with WG_TOTAL(s, waves).
#ifndef WG_TOTAL
#define WG_TOTAL(s, waves) long long s = 0; for (int w = 0; w < (waves); ++w) s += red[w]
#endif
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
    if (wave_lane() == 0) red[wave_id()] = part;
    BARRIER();
