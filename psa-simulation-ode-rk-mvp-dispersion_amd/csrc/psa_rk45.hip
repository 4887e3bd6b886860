// psa_rk45.hip -- the adaptive sweep kernel for gfx950: embedded Dormand-Prince 5(4) with per-point step-size control.
//
// One sweep point per lane, the whole z-loop inside the kernel, state and all seven stage vectors in VGPRs.  The
// algorithm is scipy.integrate.RK45 (scipy 1.15, _ivp/rk.py RungeKutta._step_impl + rk_step, _ivp/common.py
// select_initial_step / norm) applied to the complex state A[NW], step for step:
//   * stages at z + c_i*h, FSAL (stage 7 = f(z + h, y_new) is the next step's stage 1), z_new = min(z + h, z_max);
//   * error norm: RMS over the NW complex components of err_j / (atol + rtol * max(|y_j|, |y_new_j|));
//   * controller: SAFETY 0.9, factor in [0.2, 10], exponent -1/5, factor <= 1 after a rejection in the same step,
//     h clamped to [10 * ulp(z), h_max] at the start of every step; a NaN error norm is a rejection by 0.2, so a
//     non-finite state ends with status 1 (step below the minimum) exactly as scipy's solver fails;
//   * the RHS is yaman_stage<double, NW, false, LOSS> (psa_rk4_stage.inc.h) with 2*gamma*exp(i dbeta z) from an exact
//     sincos at every stage's own z (5 per attempt and pair: stage 7 shares stage 6's z).
// Lanes run independent step counts.  The loop body is the same for an accepted and a rejected attempt: y, z, the FSAL
// vector and the step are chosen with selects, and only the dense-output row stores and the loop exit diverge.  An
// attempt costs 6 RHS evaluations (64 DP instructions each for 4 waves), the stage combinations, 5 sincos per pair and
// the error norm; DESIGN.md has the count.  max_steps (accepted + rejected attempts) bounds every lane's loop.
#include "psa_launch.inc.h"
#include "psa_rk4_stage.inc.h"

namespace psa {
namespace {

// Dormand-Prince 5(4) as scipy's RK45 spells it (each entry the correctly rounded quotient, as Python's `a/b`)
constexpr double C2 = 1.0 / 5, C3 = 3.0 / 10, C4 = 4.0 / 5, C5 = 8.0 / 9;
constexpr double A21 = 1.0 / 5;
constexpr double A31 = 3.0 / 40, A32 = 9.0 / 40;
constexpr double A41 = 44.0 / 45, A42 = -56.0 / 15, A43 = 32.0 / 9;
constexpr double A51 = 19372.0 / 6561, A52 = -25360.0 / 2187, A53 = 64448.0 / 6561, A54 = -212.0 / 729;
constexpr double A61 = 9017.0 / 3168, A62 = -355.0 / 33, A63 = 46732.0 / 5247, A64 = 49.0 / 176, A65 = -5103.0 / 18656;
constexpr double B1 = 35.0 / 384, B3 = 500.0 / 1113, B4 = 125.0 / 192, B5 = -2187.0 / 6784, B6 = 11.0 / 84;
constexpr double E1 = -71.0 / 57600, E3 = 71.0 / 16695, E4 = -71.0 / 1920, E5 = 17253.0 / 339200, E6 = -22.0 / 525,
                 E7 = 1.0 / 40;
// dense output (scipy's P; row 2 is zero): y(z + x h) = y + h * sum_j (sum_s K_s P[s][j]) x^(j+1)
constexpr double P[7][4] = {
    {1.0, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0.0, 0.0, 0.0, 0.0},
    {0.0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0.0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0.0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
    {0.0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0.0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};

constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0, ERR_EXP = -1.0 / 5;

// 10 * (nextafter(z, +inf) - z) for finite z >= 0: the next double up is one unit of the bit pattern away
__device__ __forceinline__ double min_step_at(double z) {
    return 10.0 * (__longlong_as_double(__double_as_longlong(z) + 1) - z);
}

template <int NW>
struct Rk45Lane {
    static constexpr int NC = 2 * NW, NP = (NW - 2) / 2;
    double db[NP];
    double g, tg, ha;

    // E_p = 2*gamma*exp(i dbeta_p z) at one z, for every pair
    __device__ __forceinline__ void phase(double z, double (&Er)[NP], double (&Ei)[NP]) const {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            double s, c;
            sincos(db[p] * z, &s, &c);
            Er[p] = tg * c;
            Ei[p] = tg * s;
        }
    }
    template <bool LOSS>
    __device__ __forceinline__ void rhs(const double (&Er)[NP], const double (&Ei)[NP], const double (&a)[NC],
                                        double (&out)[NC]) const {
        yaman_stage<double, NW, false, LOSS>(a, a, Er, Ei, g, tg, ha, out);
    }
    template <bool LOSS>
    __device__ __forceinline__ void rhs_at(double z, const double (&a)[NC], double (&out)[NC]) const {
        double Er[NP], Ei[NP];
        phase(z, Er, Ei);
        rhs<LOSS>(Er, Ei, a, out);
    }
};

// common.norm(v / scale): sqrt(sum Re^2 + sum Im^2) / sqrt(NW), as np.linalg.norm of a complex vector
template <int NW>
__device__ __forceinline__ double rms_scaled(const double (&v)[2 * NW], const double (&scale)[NW]) {
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const double xr = v[2 * j] / scale[j], xi = v[2 * j + 1] / scale[j];
        sr = fma_(xr, xr, sr);
        si = fma_(xi, xi, si);
    }
    return sqrt(sr + si) / sqrt((double)NW);
}

__device__ __forceinline__ double cabs_(double re, double im) { return hypot(re, im); }

template <int NW, bool LOSS, bool ROWS>
__global__ void __launch_bounds__(256) rk45_sweep_kernel(const AdaptiveArgs<double> A) {
    constexpr int NC = 2 * NW, NP = (NW - 2) / 2;
    using Pair = PairOf<double>::type;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long N = A.n_points;
    if (idx >= N) return;

    Rk45Lane<NW> L;
    L.g = A.gamma[idx * A.gamma_stride];
    L.tg = L.g + L.g;
    L.ha = -0.5 * A.alpha[idx * A.alpha_stride];
    L.db[0] = A.dbeta[idx];
    if constexpr (NP == 2) L.db[1] = A.dbeta2[idx];

    double y[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = A.a0[(long long)c * A.a0_ld + idx * A.a0_stride];

    const double z_max = A.z_max, rtol = A.rtol, atol = A.atol, h_max = A.h_max;
    const long long n_out = A.n_out, LD = A.traj_ld;
    auto store_row = [&](long long r, const double (&v)[NC]) {
        double *row = A.traj + (r * NW * LD + idx) * 2;
#pragma unroll
        for (int j = 0; j < NW; ++j) *reinterpret_cast<Pair *>(row + (long long)j * LD * 2) = Pair{v[2 * j], v[2 * j + 1]};
    };
    // t_eval = np.linspace(0, z_max, n_out + 1): k * (z_max / n_out), the last one z_max itself
    const double dz_out = ROWS && n_out > 0 ? z_max / (double)n_out : 0.0;
    auto z_row = [&](long long k) { return k == n_out ? z_max : (double)k * dz_out; };
    if constexpr (ROWS) store_row(0, y);

    double z = 0.0;
    double pm = fma_(y[4], y[4], y[5] * y[5]);  // |A_sig|^2 over z = 0 and every accepted step end
    long long n_acc = 0, n_rej = 0, next_row = 1;
    int status = 1;

    if (!any_nonfinite<double, NC>(y)) {
        double K0[NC];   // f(z, y): stage 1 of the next attempt (FSAL)
        L.template rhs_at<LOSS>(0.0, y, K0);
        double h_abs;
        if (A.first_step > 0.0) {
            // scipy rejects first_step > z_max; here the first step's end is clamped onto z_max below, which is scipy
            // with first_step = z_max (h_abs becomes the clamped step before the controller scales it)
            h_abs = A.first_step;
        } else {   // common.select_initial_step (order 4): one more RHS evaluation
            double scale[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) scale[j] = atol + cabs_(y[2 * j], y[2 * j + 1]) * rtol;
            const double d0 = rms_scaled<NW>(y, scale), d1 = rms_scaled<NW>(K0, scale);
            double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
            h0 = h0 < z_max ? h0 : z_max;
            double y1[NC], f1[NC], df[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) y1[c] = y[c] + h0 * K0[c];
            L.template rhs_at<LOSS>(h0, y1, f1);
#pragma unroll
            for (int c = 0; c < NC; ++c) df[c] = f1[c] - K0[c];
            const double d2 = rms_scaled<NW>(df, scale) / h0;
            double h1;
            if (d1 <= 1e-15 && d2 <= 1e-15) h1 = (1e-6 > h0 * 1e-3) ? 1e-6 : h0 * 1e-3;
            else h1 = pow(0.01 / (d1 > d2 ? d1 : d2), 1.0 / 5);
            h_abs = 100.0 * h0;
            h_abs = h1 < h_abs ? h1 : h_abs;
            h_abs = z_max < h_abs ? z_max : h_abs;
            h_abs = h_max < h_abs ? h_max : h_abs;
        }
        double min_step = min_step_at(z);
        h_abs = h_abs > h_max ? h_max : (h_abs < min_step ? min_step : h_abs);
        bool rejected = false;   // a rejection earlier in the current step

        for (;;) {
            if (h_abs < min_step) { status = 1; break; }
            if (n_acc + n_rej >= A.max_steps) { status = 2; break; }
            double t_new = z + h_abs;
            t_new = t_new > z_max ? z_max : t_new;
            const double h = t_new - z;
            h_abs = fabs(h);

            double K1[NC], K2[NC], K3[NC], K4[NC], K5[NC], K6[NC], ys[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) ys[c] = fma_(K0[c] * A21, h, y[c]);
            L.template rhs_at<LOSS>(z + C2 * h, ys, K1);
#pragma unroll
            for (int c = 0; c < NC; ++c) ys[c] = fma_(fma_(K1[c], A32, K0[c] * A31), h, y[c]);
            L.template rhs_at<LOSS>(z + C3 * h, ys, K2);
#pragma unroll
            for (int c = 0; c < NC; ++c) ys[c] = fma_(fma_(K2[c], A43, fma_(K1[c], A42, K0[c] * A41)), h, y[c]);
            L.template rhs_at<LOSS>(z + C4 * h, ys, K3);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                ys[c] = fma_(fma_(K3[c], A54, fma_(K2[c], A53, fma_(K1[c], A52, K0[c] * A51))), h, y[c]);
            L.template rhs_at<LOSS>(z + C5 * h, ys, K4);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                ys[c] = fma_(fma_(K4[c], A65, fma_(K3[c], A64, fma_(K2[c], A63, fma_(K1[c], A62, K0[c] * A61)))), h, y[c]);
            double Er[NP], Ei[NP];
            L.phase(z + h, Er, Ei);   // c_6 = 1: stage 6 and the FSAL stage share z + h
            L.template rhs<LOSS>(Er, Ei, ys, K5);
            double yn[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c)
                yn[c] = fma_(fma_(K5[c], B6, fma_(K4[c], B5, fma_(K3[c], B4, fma_(K2[c], B3, K0[c] * B1)))), h, y[c]);
            L.template rhs<LOSS>(Er, Ei, yn, K6);

            // error norm over the NW complex components
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                double e[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int c = 2 * j + q;
                    e[q] = fma_(K6[c], E7, fma_(K5[c], E6, fma_(K4[c], E5, fma_(K3[c], E4, fma_(K2[c], E3, K0[c] * E1))))) * h;
                }
                const double ay = cabs_(y[2 * j], y[2 * j + 1]), an = cabs_(yn[2 * j], yn[2 * j + 1]);
                const double m = (ay > an || ay != ay) ? ay : an;   // np.maximum propagates NaN
                const double sc = atol + m * rtol;
                const double xr = e[0] / sc, xi = e[1] / sc;
                sr = fma_(xr, xr, sr);
                si = fma_(xi, xi, si);
            }
            const double en = sqrt(sr + si) / sqrt((double)NW);
            const bool acc = en < 1.0;
            const double f = SAFETY * pow(en, ERR_EXP);   // NaN for a NaN norm
            double fac_acc = en == 0.0 ? MAX_FACTOR : (f < MAX_FACTOR ? f : MAX_FACTOR);
            fac_acc = (rejected && !(fac_acc < 1.0)) ? 1.0 : fac_acc;
            const double fac_rej = f > MIN_FACTOR ? f : MIN_FACTOR;   // Python's max(0.2, NaN) is 0.2
            h_abs *= acc ? fac_acc : fac_rej;

            if constexpr (ROWS) {   // rows with z_k in (z, t_new]: scipy's RkDenseOutput of this step
                if (acc) {
                    while (next_row <= n_out && z_row(next_row) <= t_new) {
                        const double x = (z_row(next_row) - z) / h;
                        const double x2 = x * x, x3 = x2 * x, x4 = x3 * x;
                        double v[NC];
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            const double k[7] = {K0[c], K1[c], K2[c], K3[c], K4[c], K5[c], K6[c]};
                            double q[4];
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                double s = k[0] * P[0][jj];
#pragma unroll
                                for (int st = 2; st < 7; ++st) s = fma_(k[st], P[st][jj], s);
                                q[jj] = s;
                            }
                            v[c] = fma_(h, fma_(q[3], x4, fma_(q[2], x3, fma_(q[1], x2, q[0] * x))), y[c]);
                        }
                        store_row(next_row, v);
                        ++next_row;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                y[c] = acc ? yn[c] : y[c];
                K0[c] = acc ? K6[c] : K0[c];
            }
            z = acc ? t_new : z;
            n_acc += acc ? 1 : 0;
            n_rej += acc ? 0 : 1;
            rejected = !acc;
            const double ps = fma_(y[4], y[4], y[5] * y[5]);
            pm = (acc && (ps > pm || ps != ps)) ? ps : pm;   // NaN-propagating, accepted step ends only
            if (acc && z >= z_max) { status = 0; break; }
            min_step = min_step_at(z);
            const double hc = h_abs > h_max ? h_max : (h_abs < min_step ? min_step : h_abs);
            h_abs = acc ? hc : h_abs;   // the clamp at the start of every step
        }
    }

    if constexpr (ROWS) {   // rows past the point where the integration ended
        double nan_row[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) nan_row[c] = __builtin_nan("");
        for (long long r = next_row; r <= n_out; ++r) store_row(r, nan_row);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) A.a_end[(long long)c * N + idx] = y[c];
    A.p_end[idx] = fma_(y[4], y[4], y[5] * y[5]);
    A.p_max[idx] = pm;
    A.status[idx] = status;
    A.z_end[idx] = z;
    A.n_accepted[idx] = n_acc;
    A.n_rejected[idx] = n_rej;
}

}  // namespace

// Its own: no flag but LOSSLESS is read, so the workgroup size is the shared rule without BLOCK64; the kernel takes either size
hipError_t launch_rk45_sweep_f64(hipStream_t s, int n_waves, uint32_t flags, const AdaptiveArgs<double> &a) {
    const int block = workgroup_size(0, a.n_points, simd_count(s));
    return with_int<4, 6>(n_waves, [&](auto nw) {
    return with_bool((flags & PSA_OPT_LOSSLESS) != 0, [&](auto ll) {
    return with_bool(a.traj != nullptr, [&](auto rw) {
        return launch_lanes(reinterpret_cast<const void *>(rk45_sweep_kernel<nw, !ll, rw>), a.n_points, block, 0, a, s);
    }); }); });
}

}  // namespace psa
