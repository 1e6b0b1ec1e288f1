// The three-state recurrence of one DP cell, its tie order and its 4-bit traceback cell: the bit-exactness contract of the whole
// `--unaligned` family, written once.  Included as text (not called) inside the in-band branch of each of the sweep kernels,
// so that every kernel compiles to the instructions it had (DESIGN.md §3a); the kernel provides diag (H of the diagonal
// predecessor + the cell's score), dc (Y's column alone), xcost (X's element alone), h_left, d_left, h_up, i_up, and the sweep's
// cell, h_out, i_out, score, r, c, ni, Ci; and the two open terms: AL_OPEN_D, what a run of D ops that starts with this column
// pays on top of H (open and column), AL_OPEN_I likewise for a run of I ops that starts with X's element.  The kernels with the
// fixed open define them as AL_OPEN + dc and AL_OPEN + xcost (no brackets: the tokens they had); the position-gap kernels
// (pg_pairs.inc, pg_pairs_band.inc) as one LDS word and one register.
        const int d_ext = d_left + dc, d_open = h_left + AL_OPEN_D;
        const int i_ext = i_up + xcost, i_open = h_up + AL_OPEN_I;
        const int dd = d_ext >= d_open ? d_ext : d_open, ii = i_ext >= i_open ? i_ext : i_open;
        int h = diag;
        unsigned src = 0;
        if (dd > h) { h = dd; src = 1; }
        if (ii > h) { h = ii; src = 2; }
        cell = src | (d_ext >= d_open ? 4u : 0u) | (i_ext >= i_open ? 8u : 0u);
        h_left = h; d_left = dd; h_out = h; i_out = ii;
        if (r == ni - 1 && c == Ci - 1) score = h;
