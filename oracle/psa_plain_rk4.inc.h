/* psa_plain_rk4.inc.h -- TEST INFRASTRUCTURE.  The one text of the plain classic RK4, included once per precision by
 * psa_plain_rk4.c with
 *     T        the type of the state and of every operation            (long double | double | float)
 *     PH       the type z and the phase rate * z are formed in         (long double | double | double)
 *     SFX      the suffix of the instantiation's names                 (_ld | _f64 | _f32)
 *     COS_T, SIN_T   cos / sin of a T                                  (cosl, sinl | cos, sin | cosf, sinf)
 *     REDUCE_PHASE   defined for float alone: the phase, formed in PH = double, is brought to [-pi, pi] there before it
 *                    is rounded to T (what tests/truth_cases._expi32 does)
 *
 * The scheme is tests/truth_ld.py's: k1..k4 on the grid z_i = i h, h = z_max / n, the phase cos / sin of the product at
 * every stage, nothing carried from one step to the next but the state, nothing regrouped, complex products written out as
 * (ar br - ai bi, ar bi + ai br).  The right-hand sides are written from the equations of truth_ld's docstring. */

#define PR_CAT_(a, b) a##b
#define PR_CAT(a, b) PR_CAT_(a, b)
#define FN(name) PR_CAT(name, SFX)
#define CX FN(cx)

typedef struct { T re, im; } CX;

static inline CX FN(mul)(CX a, CX b) { CX r = { a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re }; return r; }
static inline CX FN(cj)(CX a) { CX r = { a.re, -a.im }; return r; }
static inline CX FN(add)(CX a, CX b) { CX r = { a.re + b.re, a.im + b.im }; return r; }
static inline CX FN(scale)(T s, CX a) { CX r = { s * a.re, s * a.im }; return r; }
static inline CX FN(times_i)(CX a) { CX r = { -a.im, a.re }; return r; }

/* exp(i rate z) for every phase rate of the point */
static void FN(phases)(int nc, const double *rate, PH z, CX *e)
{
    for (int c = 0; c < nc; ++c) {
        PH th = (PH)rate[c] * z;
#ifdef REDUCE_PHASE
        th = th - (PH)PR_TWO_PI * rint(th / (PH)PR_TWO_PI);
#endif
        e[c].re = COS_T((T)th);
        e[c].im = SIN_T((T)th);
    }
}

/* two pumps and K pairs [p1, p2, s_1, i_1, ..., s_K, i_K]:
 *   dA_j/dz = -alpha/2 A_j + i gamma (2S - P_j) A_j + 2 i gamma M_j,    S = sum_k P_k  (= P_j + 2 sum_{k != j} P_k)
 *   M_p1 = conj(A_p2) sum_c A_sc A_ic e^{+i th_c}    M_sc = conj(A_ic) A_p1 A_p2 e^{-i th_c}    (p2, ic: partners swapped) */
static void FN(rhs_pairs)(int nw, const CX *e, const CX *a, T g, T al, CX *out)
{
    T P[PR_MAX_WAVES], total = 0;
    CX M[PR_MAX_WAVES], mix = { 0, 0 };
    const int K = (nw - 2) / 2;
    for (int j = 0; j < nw; ++j) {
        P[j] = a[j].re * a[j].re + a[j].im * a[j].im;
        total += P[j];
    }
    for (int c = 0; c < K; ++c)
        mix = FN(add)(mix, FN(mul)(FN(mul)(a[2 + 2 * c], a[3 + 2 * c]), e[c]));
    const CX p12 = FN(mul)(a[0], a[1]);
    M[0] = FN(mul)(FN(cj)(a[1]), mix);
    M[1] = FN(mul)(FN(cj)(a[0]), mix);
    for (int c = 0; c < K; ++c) {
        const CX down = FN(mul)(p12, FN(cj)(e[c]));
        M[2 + 2 * c] = FN(mul)(FN(cj)(a[3 + 2 * c]), down);
        M[3 + 2 * c] = FN(mul)(FN(cj)(a[2 + 2 * c]), down);
    }
    for (int j = 0; j < nw; ++j) {
        const T kerr = (T)2 * total - P[j];
        out[j] = FN(add)(FN(add)(FN(scale)(-(al / (T)2), a[j]), FN(times_i)(FN(scale)(g * kerr, a[j]))),
                         FN(times_i)(FN(scale)((T)2 * g, M[j])));
    }
}

/* single pump [p, s, i], S = sum_j P_j:
 *   dA_p/dz = (-alpha/2 + i gamma (2S - P_p)) A_p + 2 i gamma conj(A_p) A_s A_i e^{+i th}
 *   dA_s/dz = (-alpha/2 + i gamma (2S - P_s)) A_s +   i gamma conj(A_i) A_p^2 e^{-i th}         (i: s <-> i) */
static void FN(rhs_single_pump)(const CX *e, const CX *a, T g, T al, CX *out)
{
    T P[3], S = 0;
    CX M[3];
    for (int j = 0; j < 3; ++j) {
        P[j] = a[j].re * a[j].re + a[j].im * a[j].im;
        S += P[j];
    }
    const CX pp = FN(mul)(FN(mul)(a[0], a[0]), FN(cj)(e[0]));
    M[0] = FN(scale)((T)2, FN(mul)(FN(mul)(FN(mul)(FN(cj)(a[0]), a[1]), a[2]), e[0]));
    M[1] = FN(mul)(FN(cj)(a[2]), pp);
    M[2] = FN(mul)(FN(cj)(a[1]), pp);
    for (int j = 0; j < 3; ++j) {
        const T kerr = (T)2 * S - P[j];
        out[j] = FN(add)(FN(add)(FN(scale)(-(al / (T)2), a[j]), FN(times_i)(FN(scale)(g * kerr, a[j]))),
                         FN(times_i)(FN(scale)(g, M[j])));
    }
}

/* M-line comb, B_m = A_m e^{i kappa_m z}:
 *   dA_m/dz = -alpha/2 A_m + i gamma e^{-i kappa_m z} sum_{k + l - n = m} B_k B_l conj(B_n)
 * every product once for k <= l (twice where k < l: (k, l, n) and (l, k, n) are one product), in ascending (k, l, n) per line */
static void FN(rhs_comb)(int nw, const CX *u, const CX *a, T g, T al, CX *out)
{
    CX B[PR_MAX_LINES], BB[PR_MAX_LINES][PR_MAX_LINES];
    for (int m = 0; m < nw; ++m)
        B[m] = FN(mul)(a[m], u[m]);
    for (int k = 0; k < nw; ++k)
        for (int l = k; l < nw; ++l)
            BB[k][l] = FN(scale)(k < l ? (T)2 : (T)1, FN(mul)(B[k], B[l]));
    for (int m = 0; m < nw; ++m) {
        CX S = { 0, 0 };
        for (int k = 0; k < nw; ++k)
            for (int l = k; l < nw; ++l) {
                const int n = k + l - m;
                if (n >= 0 && n < nw)
                    S = FN(add)(S, FN(mul)(BB[k][l], FN(cj)(B[n])));
            }
        out[m] = FN(add)(FN(scale)(-(al / (T)2), a[m]), FN(times_i)(FN(scale)(g, FN(mul)(FN(cj)(u[m]), S))));
    }
}

static void FN(rhs)(int model, int nw, const CX *e, const CX *a, T g, T al, CX *out)
{
    if (model == PR_MODEL_PAIRS)
        FN(rhs_pairs)(nw, e, a, g, al, out);
    else if (model == PR_MODEL_SINGLE_PUMP)
        FN(rhs_single_pump)(e, a, g, al, out);
    else
        FN(rhs_comb)(nw, e, a, g, al, out);
}

/* One point.  update: how y_{i+1} = y_i + (h/6)(k1 + 2 k2 + 2 k3 + k4) is stored.
 *   PR_UPDATE_PLAIN        y += increment
 *   PR_UPDATE_KAHAN        per component, with the running residue c: t = inc - c; s = y + t; c = (s - y) - t; y = s
 *   PR_UPDATE_BASE_OFFSET  the state is base + offset: y = fl(yb + dl) is formed for the stage inputs, the increment joins
 *                          dl, and every PR_FOLD_EVERY steps dl is folded into yb with its rounding residue kept in dl
 *                          (Fast2Sum: s = yb + dl; dl = dl - (s - yb); yb = s)
 *   PR_UPDATE_BASE_OFFSET_NO_RESIDUE   the same with the fold's residue thrown away (dl = 0): a planted defect
 * drift != 0 (PR_UPDATE_PLAIN only) plants ONE defect into the otherwise plain run: after every step the waves behind the two
 * pumps are scaled by 1 + drift -- what a rotation by a rounded r = exp(i dbeta h/2), |r| = 1 + drift, does to the sidebands'
 * moduli in a kernel that applies one per step.  The tests use it to evaluate such a kernel's stated drift budget.
 * rows: (n / save_every + 1, nw) or NULL.  Row 0 at z = 0, a row after every step with (i + 1) % save_every == 0. */
static void FN(point)(int model, int nw, int nc, int update, double drift, double z_max, int64_t n, int64_t save_every,
                      const double *rate, double gamma, double alpha, const double *a0, CX *rows, CX *a_end, T *p_end, T *p_max)
{
    const PH hp = (PH)z_max / (PH)n;
    const T g = (T)gamma, al = (T)alpha;
    CX y[PR_MAX_WAVES], yb[PR_MAX_WAVES], dl[PR_MAX_WAVES], s[PR_MAX_WAVES];
    CX k1[PR_MAX_WAVES], k2[PR_MAX_WAVES], k3[PR_MAX_WAVES], k4[PR_MAX_WAVES];
    CX e0[PR_MAX_WAVES], em[PR_MAX_WAVES], e1[PR_MAX_WAVES];
    int64_t row = 0;
    for (int j = 0; j < nw; ++j) {
        y[j].re = (T)a0[2 * j];
        y[j].im = (T)a0[2 * j + 1];
        yb[j] = y[j];
        dl[j].re = dl[j].im = 0;            /* the offset of the base + offset forms, the residue of Kahan's */
        a_end[j] = y[j];
        p_end[j] = p_max[j] = y[j].re * y[j].re + y[j].im * y[j].im;
        if (rows)
            rows[j] = y[j];
    }
    for (int64_t i = 0; i < n; ++i) {
        /* the grid is z_i = i h, its last point z_max, and the step from z_i is the difference of its two grid points, as
         * integrate_fixed_step and every NumPy twin take it (np.linspace, h = z[i + 1] - z[i]): in exact arithmetic h, in
         * double off it by the rounding of the two points.  One rounded h for every step is another rounding path: the
         * double instantiation then sat 1.44x off pairs_np's median on one input set (tests/test_truth_long_host.py). */
        const PH z = (PH)i * hp, z_next = i + 1 == n ? (PH)z_max : (PH)(i + 1) * hp, hz = z_next - z;
        const T h = (T)hz, half = (T)(hz / (PH)2), sixth = (T)(hz / (PH)6);
        FN(phases)(nc, rate, z, e0);
        FN(phases)(nc, rate, z + hz / (PH)2, em);
        FN(phases)(nc, rate, z + hz, e1);
        FN(rhs)(model, nw, e0, y, g, al, k1);
        for (int j = 0; j < nw; ++j)
            s[j] = FN(add)(y[j], FN(scale)(half, k1[j]));
        FN(rhs)(model, nw, em, s, g, al, k2);
        for (int j = 0; j < nw; ++j)
            s[j] = FN(add)(y[j], FN(scale)(half, k2[j]));
        FN(rhs)(model, nw, em, s, g, al, k3);
        for (int j = 0; j < nw; ++j)
            s[j] = FN(add)(y[j], FN(scale)(h, k3[j]));
        FN(rhs)(model, nw, e1, s, g, al, k4);
        for (int j = 0; j < nw; ++j) {
            const CX inc = FN(scale)(sixth, FN(add)(FN(add)(FN(add)(k1[j], FN(scale)((T)2, k2[j])), FN(scale)((T)2, k3[j])), k4[j]));
            T *yy = &y[j].re, *bb = &yb[j].re, *dd = &dl[j].re;
            const T ii[2] = { inc.re, inc.im };
            for (int c = 0; c < 2; ++c) {
                if (update == PR_UPDATE_PLAIN) {
                    yy[c] = yy[c] + ii[c];
                } else if (update == PR_UPDATE_KAHAN) {
                    const T t = ii[c] - dd[c];
                    const T sum = yy[c] + t;
                    dd[c] = (sum - yy[c]) - t;
                    yy[c] = sum;
                } else {
                    dd[c] = dd[c] + ii[c];
                    if ((i + 1) % PR_FOLD_EVERY == 0) {
                        const T sum = bb[c] + dd[c];
                        dd[c] = update == PR_UPDATE_BASE_OFFSET ? dd[c] - (sum - bb[c]) : (T)0;
                        bb[c] = sum;
                    }
                    yy[c] = bb[c] + dd[c];
                }
            }
        }
        if (drift != 0.0)                   /* planted: every wave but the two pumps scaled by 1 + drift after the step */
            for (int j = 2; j < nw; ++j)
                y[j] = FN(scale)((T)1 + (T)drift, y[j]);
        if ((i + 1) % save_every == 0) {
            ++row;
            for (int j = 0; j < nw; ++j) {
                const T p = y[j].re * y[j].re + y[j].im * y[j].im;
                a_end[j] = y[j];            /* a_end, p_wave_end: the last saved row */
                p_end[j] = p;
                if (p > p_max[j])
                    p_max[j] = p;
                if (rows)
                    rows[row * nw + j] = y[j];
            }
        }
    }
}

/* N points, OpenMP over the points with the runtime's default thread count.  rate (N, nc), gamma / alpha (N,), a0 (N, nw)
 * complex as pairs of doubles; rows (N, n / save_every + 1, nw) or NULL, a_end (N, nw), p_wave_end / p_wave_max (N, nw): all
 * in T, as the instantiation computed them.  -> 0, or -1 for arguments outside the text's limits. */
int FN(psa_plain_rk4)(int model, int nw, int update, double drift, int64_t n_points, double z_max, int64_t n, int64_t save_every,
                      const double *rate, const double *gamma, const double *alpha, const double *a0, void *rows, void *a_end,
                      void *p_wave_end, void *p_wave_max)
{
    const int nc = model == PR_MODEL_PAIRS ? (nw - 2) / 2 : model == PR_MODEL_SINGLE_PUMP ? 1 : nw;
    if (nw < 1 || nw > PR_MAX_WAVES || n < 1 || save_every < 1 || update < 0 || update > PR_UPDATE_BASE_OFFSET_NO_RESIDUE
        || (model == PR_MODEL_PAIRS && (nw < 4 || nw % 2)) || (model == PR_MODEL_SINGLE_PUMP && nw != 3)
        || (model == PR_MODEL_COMB && nw > PR_MAX_LINES) || (drift != 0.0 && (update != PR_UPDATE_PLAIN || model != PR_MODEL_PAIRS))
        || (model != PR_MODEL_PAIRS && model != PR_MODEL_SINGLE_PUMP && model != PR_MODEL_COMB))
        return -1;
    const int64_t n_rows = n / save_every + 1;
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t p = 0; p < n_points; ++p)
        FN(point)(model, nw, nc, update, drift, z_max, n, save_every, rate + p * nc, gamma[p], alpha[p], a0 + p * 2 * nw,
                  rows ? (CX *)rows + p * n_rows * nw : NULL, (CX *)a_end + p * nw, (T *)p_wave_end + p * nw,
                  (T *)p_wave_max + p * nw);
    return 0;
}

#undef CX
#undef FN
#undef PR_CAT
#undef PR_CAT_
