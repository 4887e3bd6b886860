// psa_rk4_single_pump_kernel.inc.h -- float64 RK4 sweep of the SINGLE-PUMP (degenerate) three-wave model (gfx950): one pump,
// a signal at w_s and an idler at w_i = 2 w_p - w_s.  Build-defined, no reference counterpart.
//
//     waves [p, s, i],  P_j = |A_j|^2,  S = P_p + P_s + P_i,  E(z) = 2*gamma*exp(i*dbeta*z),  dbeta = b(w_s) + b(w_i) - 2 b(w_p)
//     dA_p/dz = (-alpha/2 + i*gamma*(2S - P_p)) A_p + i*conj(A_p) * E * A_s A_i
//     dA_s/dz = (-alpha/2 + i*gamma*(2S - P_s)) A_s + i*conj(A_i) * (conj(E)/2) * A_p^2            (i: s <-> i)
//
// Sign and phase conventions are yaman_stage's (the pump reads e^{+i dbeta z}).  This is NOT the 4-wave system with A1 == A2:
// with a = A1 = A2 and A_p = sqrt(2) a the sideband equations coincide, but the pump's self-phase term there is
// 3*gamma*|a|^2 = 1.5*gamma*|A_p|^2 instead of gamma*|A_p|^2.
//
// Layout: one sweep point per lane, the whole z-loop in the kernel, the six state components in VGPRs, the fused regrouped
// stage (stage coefficient folded into g, tg, ha and the carried phase factor).  The step, the re-seeds on the absolute
// RESYNC grid, the event-driven loop, the save / NaN semantics and the replay that finds the exact first_bad_step are the
// shared ones of psa_rk4_carried.inc.h (see that file); every stride, save_every == 1 included, goes through its event loop.
// Wave-uniform control flow only: every branch is on a kernel argument, the loop counters or a ballot.
//
// What is carried is H = E/2, not E.  The sidebands need conj(E)/2 * A_p^2 and Im(A_p^2) = fma(x, y, y*x) = 2*RN(x*y) for every
// input (tests/test_fold_identity.py; DESIGN.md 3.1 item 8, history), so with m = RN(x*y)
//     Re (conj(E)/2 * A_p^2) = H_r*Re(A_p^2) + H_i*(2m) = H_r*Re(A_p^2) + E_i*m        E = H + H: an exact doubling
//     Im (conj(E)/2 * A_p^2) = H_r*(2m) - H_i*Re(A_p^2) = E_r*m - H_i*Re(A_p^2)
// are the same real products, hence the same rounded numbers, and Im(A_p^2) is never formed.  The pump reads E, the sidebands
// H and E; every value is the result of an explicit fma, of a bare product that feeds one, or of an add of such results, so
// -ffp-contract=fast has nothing left to fuse and the result is bit-defined whatever the instantiation.  The one edge is the
// overflow of E = H + H, |2 d gamma| >= 2^1023, where the cubic terms of step 0 overflow all the same.
//
// Per stage 50 DP instructions (|A_j|^2: 6, S and g_j: 6, A_s A_i: 4, E * A_s A_i: 4, Re(A_p^2) and m: 2 -- the y*y of |A_p|^2
// is shared --, conj(H) A_p^2: 4, six 4-deep chains: 24; 44 without the loss links), per step 4 * 50 + 18 (t) + 6 (update) +
// 8 (two rotations of H) + 6 (three doublings: E at z + h/2, 2E for stage 3, E at z + h) = 238 against 298 for four waves;
// 239 as built (215 without the loss links), see the table in DESIGN.md 3.3c.
//
// Out of scope: lane-pair / lane-quad layouts, RK45, chains, LDS staging, a mirrored variant, a dedicated
// save_every == 1 trajectory loop (every stride goes through the event loop).  Float32 is
// psa_rk4_single_pump_pk_kernel.inc.h.
#pragma once
#include "psa_launch.inc.h"
#include "psa_rk4_carried.inc.h"

namespace psa {

// out = base + c * dA/dz of a = [Re p, Im p, Re s, Im s, Re i, Im i]; c is folded into g = c*gamma, tg = 2*c*gamma,
// ha = -c*alpha/2, (Hr, Hi) = c*gamma*exp(i*dbeta*z) and (Er, Ei) = twice that.
template <bool LOSS>
__device__ __forceinline__ void single_pump_stage(const double (&a)[6], const double (&base)[6], const double Hr, const double Hi,
                                                  const double Er, const double Ei, const double g, const double tg,
                                                  const double ha, double (&out)[6]) {
    const double xp = a[0], yp = a[1], xs = a[2], ys = a[3], xi = a[4], yi = a[5];
    const double ypyp = yp * yp;   // shared by |A_p|^2 and Re A_p^2
    const double p[3] = {fma_(xp, xp, ypyp), fma_(xs, xs, ys * ys), fma_(xi, xi, yi * yi)};
    const double s = (p[0] + p[1]) + p[2];
    const double gs = tg * s;   // c*gamma * 2S
    double gj[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) gj[j] = fma_(-g, p[j], gs);   // c*gamma * (2S - P_j)

    auto link = [&](const double gsig, const double v, const int c) -> double {
        if constexpr (LOSS) return fma_(gsig, v, fma_(ha, a[c], base[c]));
        else return fma_(gsig, v, base[c]);
    };
    const double qr = fma_(xs, xi, -(ys * yi)), qi = fma_(xs, yi, ys * xi);   // A_s A_i
    const double Fpr = fma_(Er, qr, -(Ei * qi)), Fpi = fma_(Er, qi, Ei * qr);  // E A_s A_i: drives the pump
    const double ppr = fma_(xp, xp, -ypyp);                                   // Re A_p^2
    const double m = yp * xp;                                                 // Im A_p^2 = 2m
    const double Fsr = fma_(Hr, ppr, Ei * m), Fsi = fma_(Er, m, -(Hi * ppr));  // conj(E)/2 A_p^2: drives signal and idler
    // pump: (ha + i g_p) A_p + i conj(A_p) Fp
    out[0] = fma_(yp, Fpr, fma_(-xp, Fpi, link(-gj[0], yp, 0)));
    out[1] = fma_(xp, Fpr, fma_(yp, Fpi, link(gj[0], xp, 1)));
    // signal: (ha + i g_s) A_s + i conj(A_i) Fs ;  idler: (ha + i g_i) A_i + i conj(A_s) Fs
    out[2] = fma_(yi, Fsr, fma_(-xi, Fsi, link(-gj[1], ys, 2)));
    out[3] = fma_(xi, Fsr, fma_(yi, Fsi, link(gj[1], xs, 3)));
    out[4] = fma_(ys, Fsr, fma_(-xs, Fsi, link(-gj[2], yi, 4)));
    out[5] = fma_(xs, Fsr, fma_(ys, Fsi, link(gj[2], xi, 5)));
}

template <int CHECK, bool TRAJ, int BLOCK, bool LOSS>
__global__ void __launch_bounds__(BLOCK) rk4_sweep_single_pump_kernel(const SinglePumpArgs<double> A) {
    const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long N = A.n_points;
    if (idx >= N) return;

    double a[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) a[c] = A.a0[(long long)c * A.a0_ld + idx * A.a0_stride];
    const double g = A.gamma[idx * A.gamma_stride];
    const double ha = -0.5 * A.alpha[idx * A.alpha_stride];
    const double dbd = A.dbeta[idx];
    const CarriedConsts K = carried_consts(g, ha, dbd, A.z_max, A.n_steps);
    const double h_amp = K.g_d;   // modulus of the carried H = E/2 = d*gamma*exp(i*dbeta*z)
    double Hr = h_amp, Hi = 0.0;

    double pm[3];   // np.max of |A_j|^2 over saved rows (z = 0 is one)
#pragma unroll
    for (int j = 0; j < 3; ++j) pm[j] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
    auto store_a_end = [&]() {   // the last saved row and |A_j|^2 there
#pragma unroll
        for (int c = 0; c < 6; ++c) A.a_end[(long long)c * N + idx] = a[c];
#pragma unroll
        for (int j = 0; j < 3; ++j) A.p_wave_end[(long long)j * N + idx] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
    };
    // trajectory rows [row][wave][ld][2]: a wave-uniform (row, wave) base and the lane's 32-bit byte offset, as in
    // rk4_sweep_kernel; the C-ABI keeps ld * 16 below 2^32 for trajectory launches
    using Pair = typename PairOf<double>::type;
    const long long LD = A.traj_ld;
    const unsigned lane_off = (unsigned)idx * (unsigned)sizeof(Pair);
    auto store_traj_row = [&](const int r) {
        const char *rowb = reinterpret_cast<const char *>(A.traj) + (long long)r * 3 * LD * (long long)sizeof(Pair);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            store_pair_nt(rowb + (long long)j * LD * (long long)sizeof(Pair), lane_off, Pair{a[2 * j], a[2 * j + 1]});
    };
    if constexpr (TRAJ) store_traj_row(0);
    if (A.n_steps / A.save_every == 0) store_a_end();   // no saved row after z = 0

    // the adapter forms E = H + H from the factor it is handed; stage 3 is handed 2H, stage 2's E
    auto stage = [&](auto full, const double (&y)[6], const double (&base)[6], const double hr, const double hi, double (&out)[6]) {
        if constexpr (decltype(full)::value) single_pump_stage<LOSS>(y, base, hr, hi, hr + hr, hi + hi, K.g_h, K.tg_h, K.ha_h, out);
        else single_pump_stage<LOSS>(y, base, hr, hi, hr + hr, hi + hi, K.g_d, K.tg_d, K.ha_d, out);
    };
    auto step_on = [&](double (&y)[6], double &hr, double &hi) { carried_step<6>(y, hr, hi, K.rc, K.rs, stage); };
    auto seed_on = [&](const int step, double &hr, double &hi) { carried_seed(h_amp, dbd, K.hd, step, hr, hi); };
    auto nonfinite_on = [&](const double (&y)[6]) -> bool { return any_nonfinite<double, 6>(y); };
    auto summarise = [&]() {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const double pw = fma_(a[2 * w], a[2 * w], a[2 * w + 1] * a[2 * w + 1]);
            pm[w] = (pw > pm[w] || pw != pw) ? pw : pm[w];   // np.max propagates NaN
        }
    };
    auto save_row = [&](const int row, const bool last) {
        if constexpr (TRAJ) store_traj_row(row);
        if (last) store_a_end();
    };
    const long long bad = carried_event_loop<CHECK, 2>(a, Hr, Hi, A.n_steps, A.save_every, step_on, seed_on, nonfinite_on, summarise, save_row);
#pragma unroll
    for (int j = 0; j < 3; ++j) A.p_wave_max[(long long)j * N + idx] = pm[j];
    A.first_bad[idx] = bad;
}

}  // namespace psa
