// The body of one tile of K21 / K25 (ctc_align_long.hip has the picture).  Included, not called:
// once as the body of K21's tile kernel, and once as the body of the device function K25's tile
// kernel calls.  K21's kernel has to stay the code it was, instruction for instruction: routed
// through an inlined function - the same statements - its code came out with scalar operands
// and two registers swapped and ran 0.7 % longer at the hour shape.
//
// In scope where it is included: the arguments of the tile kernel (labels, T, C, blank, L,
// tile_frames, diag, i_lo, ctrl, table, rowb, halo, bp) and two constants:
//   WILD  a label may be CTCASR_ALIGN_WILDCARD (K25);
//   FILL  (WILD only) some thread of this tile holds one, so fill[t] is needed.
    __shared__ float s_lp[ALONG_STAGE_FRAMES * ALONG_MAX_C];
    __shared__ double s_hin[ALONG_STAGE_FRAMES];
    __shared__ double s_xch[2][ALONG_WAVES];
    __shared__ float s_fill[FILL ? ALONG_STAGE_FRAMES : 1];

    if (ctrl[LC_STATUS] != 0) return;
    const AlongGeom g(T, C, L, tile_frames);
    const long long i = i_lo + blockIdx.x, j = diag - i;
    if (!g.live(i, j)) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s0 = j * ALONG_TILE_STATES + (long long)tid * ALONG_PER_THREAD;
    const long long t_first = i * g.tf;
    const long long t_end = t_first + g.tf < T ? t_first + g.tf : T;

    // states s0 .. s0+3: blank, label k0, blank, label k0 + 1 (where they exist)
    const long long k0 = s0 >> 1;
    const bool has_a = k0 < L, has_b = k0 + 1 < L;
    const int lab_a = has_a ? labels[k0] : blank;
    const int lab_b = has_b ? labels[k0 + 1] : blank;
    const bool skip_a = has_a && k0 >= 1 && labels[k0 - 1] != lab_a;   // s0 - 1 -> s0 + 1
    const bool skip_b = has_b && lab_b != lab_a;                       // s0 + 1 -> s0 + 3
    const bool has_below = s0 >= 1;
    // WILD: the wildcard may be this thread's lab_a or its lab_b (never both: refused in prep);
    // its emission is fill[t], and the table is read at the blank's column in its place
    const bool wild_a = WILD && has_a && lab_a == CTCASR_ALIGN_WILDCARD;
    const bool wild_b = WILD && has_b && lab_b == CTCASR_ALIGN_WILDCARD;
    const int col_a = wild_a ? blank : lab_a, col_b = wild_b ? blank : lab_b;

    const double ninf = -(double)INFINITY;
    double v0 = ninf, v1 = ninf, v2 = ninf, v3 = ninf;
    if (i > 0 && g.live(i - 1, j)) {
        const double *src = rowb + (size_t)(i - 1) * g.s_pad + s0;
        v0 = src[0]; v1 = src[1]; v2 = src[2]; v3 = src[3];
    }
    const bool left_live = g.live(i, j - 1);          // writer of the halo at frames >= t_first
    const bool diag_live = g.live(i - 1, j - 1);      // ... and at frame t_first - 1

    for (long long tc = t_first; tc < t_end; tc += ALONG_STAGE_FRAMES) {
        const int nf = (int)(t_end - tc < ALONG_STAGE_FRAMES ? t_end - tc : ALONG_STAGE_FRAMES);
        __syncthreads();          // the frames before are done with the stage
        for (int e = tid; e < nf * C; e += ALONG_THREADS) s_lp[e] = table[(size_t)tc * C + e];
        if (tid < nf) {
            const long long tp = tc + tid - 1;        // the frame the halo value belongs to
            double h = ninf;
            if (j > 0 && tp >= 0 && (tp >= t_first ? left_live : diag_live))
                h = halo[(size_t)(j - 1) * T + tp];
            s_hin[tid] = h;
        }
        __syncthreads();
        if (FILL) {
            // fill of staged frame f: 4 threads take the columns q, q + 4, ... of its row (the
            // maximum of finite values does not depend on the order it is taken in)
            const int f = tid >> 2, q = tid & 3;
            float mx = s_lp[f < nf ? f * C : 0];
            if (f < nf)
                for (int c = q; c < C; c += 4) mx = fmaxf(mx, s_lp[f * C + c]);
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            if (f < nf && q == 0) s_fill[f] = mx;
            __syncthreads();
        }
        for (int f = 0; f < nf; ++f) {
            const long long t = tc + f;
            const float *lp = s_lp + f * C;
            const double e_blank = (double)lp[blank];
            double e_a = (double)lp[col_a], e_b = (double)lp[col_b];
            if (FILL) {
                const double e_fill = (double)s_fill[f];
                e_a = wild_a ? e_fill : e_a;
                e_b = wild_b ? e_fill : e_b;
            }
            if (t == 0) {          // (uniform: the first frame of tile row 0)
                v0 = s0 == 0 ? e_blank : ninf;
                v1 = (s0 == 0 && has_a) ? e_a : ninf;
                v2 = ninf;
                v3 = ninf;
            } else {
                const int par = (int)(t & 1);
                if (lane == 63) s_xch[par][wave] = v3;
                __syncthreads();
                double below = __shfl_up(v3, 1, 64);
                if (lane == 0) below = wave == 0 ? s_hin[f] : s_xch[par][wave - 1];
                // tie rule: strict > in the order s, s - 1, s - 2
                double b0 = v0, b1 = v1, b2 = v2, b3 = v3;
                int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
                if (has_below && below > b0) { b0 = below; m0 = 1; }
                if (v0 > b1) { b1 = v0; m1 = 1; }
                if (skip_a && below > b1) { b1 = below; m1 = 2; }
                if (v1 > b2) { b2 = v1; m2 = 1; }
                if (v2 > b3) { b3 = v2; m3 = 1; }
                if (skip_b && v1 > b3) { b3 = v1; m3 = 2; }
                v0 = b0 + e_blank;
                v1 = has_a ? b1 + e_a : ninf;
                v2 = has_a ? b2 + e_blank : ninf;     // state s0 + 2 exists iff label k0 does
                v3 = has_b ? b3 + e_b : ninf;
                if (s0 >= g.S) v0 = ninf;
                bp[((size_t)j * T + t) * ALONG_THREADS + tid] =
                    (unsigned char)(m0 | (m1 << 2) | (m2 << 4) | (m3 << 6));
            }
            if (tid == ALONG_THREADS - 1) halo[(size_t)j * T + t] = v3;
        }
    }
    double *dst = rowb + (size_t)i * g.s_pad + s0;
    dst[0] = v0; dst[1] = v1; dst[2] = v2; dst[3] = v3;
