// psa_rk4_split_kernel.inc.h -- float64 RK4 sweep with TWO LANES PER SWEEP POINT (gfx950).
//
// Why: the sweep is FP64-issue bound and the z-loop is sequential, so a sweep smaller than the chip
// (N <= 32 768 points = 512 waves for 1 024 SIMDs: BASELINE config 5's per-GPU shard; config 1's single point)
// leaves SIMDs idle that no amount of occupancy can use.  Here a point's waves are divided between an even
// lane and its odd neighbour, which halves the dependent instruction stream per lane:
//
//   4 waves   even lane: (u, v) = (A_p1, A_p2)            odd lane: (u, v) = (A_s, A_i)
//             dA_u/dz = (-alpha/2 + i*gamma*f_u) A_u + i*conj(A_v) * F,    F = E_lane * Q
//             Q = (A_u A_v) of the PARTNER lane,  E_lane = 2*gamma*exp(+i*dbeta*z) (even) | its conjugate (odd)
//             -- the pumps are driven by E*(A_s A_i), the sidebands by conj(E)*(A_p1 A_p2)  (yaman_model.py:174-181),
//             so both lanes run the SAME instruction stream with a lane-dependent sign of dbeta.
//   6 waves   even lane: (w, u, v) = (A_p1, A_s1, A_i1), dbeta_1      odd lane: (A_p2, A_s2, A_i2), dbeta_2
//             dA_w/dz = (...) A_w + i*conj(W) * (t + T),   t = E_own * (A_u A_v),  W, T = the partner's A_w, t
//             dA_u/dz = (...) A_u + i*conj(A_v) * conj(E_own) * (A_w W)            (same for v with u)
//   f_j = 2*S - |A_j|^2 with S = own partial sum + the partner's.
//
// Values cross between the two lanes with DPP quad_perm:[1,0,3,2] moves (two v_mov_b32_dpp per double: gfx950's
// DP ALU accepts no quad_perm, so the exchange cannot be folded into the consuming v_fma_f64).  Per RHS evaluation:
// 4 waves 39 instructions (6 of them moves) instead of 64; 6 waves 65 (10 moves) instead of 100.
// The regrouped RK4 step, the phase recurrence, both z-loops and the save / NaN semantics (exact index by replay) are the
// shared ones of psa_rk4_carried.inc.h -- see that file.
// 4 waves: a wave whose points all start mirrored (A2 == A1, A4 == A3) does not run this stage at all but the mirrored z-loop of
// rk4_sweep_kernel on its even lanes (see the kernel below).
#pragma once
#include "psa_rk4_carried.inc.h"
#include "psa_rk4_kernel.inc.h"

namespace psa {

// the value the neighbouring lane (lane ^ 1) holds
__device__ __forceinline__ double from_partner(const double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true);  // quad_perm:[1,0,3,2]
    hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// (A/B, DESIGN.md 5.2: routing the exchanges that have slack -- the other pump, the other pair's driving term -- through
// the LDS crossbar with ds_swizzle_b32 frees 32 VALU slots per step but its latency is exposed with one wave per SIMD:
// 12.50 ms instead of 11.73 ms on the config-5 shard shape.  All exchanges stay DPP moves.)

// out = base + c * dA/dz(a) for the lane's own waves (stage coefficient folded into g, tg, ha, E as in yaman_stage).
// NL = waves per lane (2 | 3); a = [Re, Im] x NL in the lane's order given above.
template <int NL, bool LOSS>
__device__ __forceinline__ void split_stage(const double (&a)[2 * NL], const double (&base)[2 * NL], const double Er,
                                            const double Ei, const double g, const double tg, const double ha,
                                            double (&out)[2 * NL]) {
    double p[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) p[j] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
    double sl = p[0] + p[1];
    if constexpr (NL == 3) sl += p[2];
    const double s = sl + from_partner(sl);
    const double gs = tg * s;
    double gj[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) gj[j] = fma_(-g, p[j], gs);
    auto link = [&](const double gsig, const double v, const int c) -> double {
        if constexpr (LOSS) return fma_(gsig, v, fma_(ha, a[c], base[c]));
        else return fma_(gsig, v, base[c]);
    };
    // the last two waves of the lane are a pair (u, v) coupled through one driving term F
    constexpr int U = 2 * (NL - 2);
    const double xu = a[U], yu = a[U + 1], xv = a[U + 2], yv = a[U + 3];
    const double qr = fma_(xu, xv, -(yu * yv)), qi = fma_(xu, yv, yu * xv);  // A_u * A_v
    double Fr, Fi;
    if constexpr (NL == 2) {
        const double Qr = from_partner(qr), Qi = from_partner(qi);
        Fr = fma_(Er, Qr, -(Ei * Qi));
        Fi = fma_(Er, Qi, Ei * Qr);
    } else {
        const double xw = a[0], yw = a[1];
        const double Xw = from_partner(xw), Yw = from_partner(yw);  // the other pump
        const double tr = fma_(Er, qr, -(Ei * qi)), ti = fma_(Er, qi, Ei * qr);  // E_own * (A_u A_v)
        const double Fpr = tr + from_partner(tr), Fpi = ti + from_partner(ti);  // sum over both pairs
        const double q12r = fma_(xw, Xw, -(yw * Yw)), q12i = fma_(xw, Yw, yw * Xw);  // A_p1 * A_p2
        Fr = fma_(Er, q12r, Ei * q12i);  // conj(E_own) * (A_p1 A_p2)
        Fi = fma_(Er, q12i, -(Ei * q12r));
        // pump: (ha + i g_w) A_w + i conj(W) Fp
        out[0] = fma_(Yw, Fpr, fma_(-Xw, Fpi, link(-gj[0], yw, 0)));
        out[1] = fma_(Xw, Fpr, fma_(Yw, Fpi, link(gj[0], xw, 1)));
    }
    const double gu = gj[NL - 2], gv = gj[NL - 1];
    out[U] = fma_(yv, Fr, fma_(-xv, Fi, link(-gu, yu, U)));
    out[U + 1] = fma_(xv, Fr, fma_(yv, Fi, link(gu, xu, U + 1)));
    out[U + 2] = fma_(yu, Fr, fma_(-xu, Fi, link(-gv, yv, U + 2)));
    out[U + 3] = fma_(xu, Fr, fma_(yu, Fi, link(gv, xv, U + 3)));
}

// WSUM: the per-wave summary (see rk4_sweep_kernel); each lane keeps the running maxima of its own NL waves and writes their rows
template <int NW, int CHECK, bool TRAJ, int BLOCK, bool LOSS, bool WSUM = false>
__global__ void __launch_bounds__(BLOCK) rk4_sweep_split_kernel(const SweepArgs<double> A) {
    static_assert(!WSUM || !TRAJ, "the per-wave summary exists for launches without trajectory");
    constexpr int NL = NW / 2;    // waves per lane
    constexpr int NC = 2 * NL;    // real components per lane
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long idx = gid >> 1;   // sweep point: lanes 2k and 2k+1 of a wave share one
    const int role = (int)(gid & 1);
    const long long N = A.n_points;
    if (idx >= N) return;             // both lanes of a pair leave together

    // which global wave each of the lane's waves is
    int wave_of[NL];
    if constexpr (NL == 2) {
        wave_of[0] = 2 * role;
        wave_of[1] = 2 * role + 1;
    } else {
        wave_of[0] = role;
        wave_of[1] = 2 + 2 * role;
        wave_of[2] = 3 + 2 * role;
    }
    const bool owns_signal = (NL == 2) ? (role == 1) : (role == 0);   // wave index 2, the gain summary's wave
    constexpr int SIG = (NL == 2) ? 0 : 2;                            // its component offset in the owning lane

    double y[NC];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        y[2 * j] = A.a0[(long long)(2 * wave_of[j]) * A.a0_ld + idx * A.a0_stride];
        y[2 * j + 1] = A.a0[(long long)(2 * wave_of[j] + 1) * A.a0_ld + idx * A.a0_stride];
    }
    // 4 waves: a wave whose live points all start mirrored (A2 == A1 and A4 == A3 bit for bit, all finite: each lane tests its
    // own two waves, one ballot) takes the mirrored z-loop of rk4_sweep_kernel -- sweep_point<..., MIRROR> on the even lane
    // of each point, the odd lane leaves.  The z-loop is issue-bound, so what counts is the wave's instruction stream, not
    // how many of its lanes work: 144 instructions per step instead of this kernel's 183.6.  And the record is then the
    // one-lane kernel's in every bit, whatever layout a sweep's size selects (the stage below pairs the products as
    // A_u * A_v per lane, the one-lane kernel crosswise: on other points the two layouts agree to rounding).  With the
    // run-time row loop (ROW = 0) at every stride: the fixed-row form is the one-lane launch's, and moves no bit.
    if constexpr (NL == 2) {
        const bool same = __builtin_bit_cast(long long, y[0]) == __builtin_bit_cast(long long, y[2]) &&
                          __builtin_bit_cast(long long, y[1]) == __builtin_bit_cast(long long, y[3]);
        const bool objects = !same || any_nonfinite<double, NC>(y);
        if (__builtin_amdgcn_ballot_w64(objects) == 0) {
            if (role) return;
            long long idx_m = idx;            // A1 and A3 loaded again through an opaque index, as in rk4_sweep_kernel
            asm volatile("" : "+v"(idx_m));
            double ym[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) ym[c] = A.a0[(long long)(c < 2 ? c : c + 2) * A.a0_ld + idx_m * A.a0_stride];
            sweep_point<double, 4, CHECK, TRAJ, BLOCK, false, LOSS, WSUM, true>(A, idx_m, ym);
            return;
        }
    }
    const double g = A.gamma[idx * A.gamma_stride];
    const double ha = -0.5 * A.alpha[idx * A.alpha_stride];
    // the lane's phase rate: 4 waves +dbeta (pumps) | -dbeta (sidebands: conj(E)); 6 waves the own pair's dbeta_k
    double dbd;
    if constexpr (NL == 2) dbd = role ? -A.dbeta[idx] : A.dbeta[idx];
    else dbd = role ? A.dbeta2[idx] : A.dbeta[idx];

    const CarriedConsts K = carried_consts(g, ha, dbd, A.z_max, A.n_steps);
    const double e_amp = K.tg_d;
    double Er = e_amp, Ei = 0.0;

    double pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
    double pm = pe;
    double pwm[WSUM ? NL : 1];     // WSUM: np.max of |A|^2 over saved rows, for each of the lane's waves
    if constexpr (WSUM) {
#pragma unroll
        for (int j = 0; j < NL; ++j) pwm[j] = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
    }
    // any component of the POINT non-finite (own lane's or the partner's)
    auto nonfinite_on = [&](const double (&v)[NC]) -> bool {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) t = fma_(v[c], 0.0, t);
        t += from_partner(t);
        return t != t;
    };

    // trajectory rows [row][wave][N][2]: the lane writes its own waves' (re, im) pairs.  wave_of[j] = U_j + role * R_j, so the
    // address splits into a wave-uniform part (row, U_j: an SGPR pair) and a per-lane constant 32-bit byte offset
    // (role * R_j * N + idx) * 16 -- the global_store saddr form of rk4_sweep_kernel, no vector instruction spent on
    // addressing inside the z-loop.  (The C-ABI keeps NW * N * 16 B < 2^32 for two-lane trajectory launches.)
    using Pair = typename PairOf<double>::type;
    const long long LD = A.traj_ld;   // points per (row, wave) region (psa_traj_ld)
    unsigned lane_off[NL];
    int wave_u[NL];
    if constexpr (NL == 2) {
        wave_u[0] = 0;
        wave_u[1] = 1;
        lane_off[0] = lane_off[1] = (unsigned)((unsigned long long)(role * 2 * LD + idx) * sizeof(Pair));
    } else {
        wave_u[0] = 0;
        wave_u[1] = 2;
        wave_u[2] = 3;
        lane_off[0] = (unsigned)((unsigned long long)(role * LD + idx) * sizeof(Pair));
        lane_off[1] = lane_off[2] = (unsigned)((unsigned long long)(role * 2 * LD + idx) * sizeof(Pair));
    }
    auto store_traj_row = [&](const int r) {
        const char *rowb = reinterpret_cast<const char *>(A.traj) + (long long)r * NW * LD * (long long)sizeof(Pair);
#pragma unroll
        for (int j = 0; j < NL; ++j)
            store_pair_nt(rowb + (long long)wave_u[j] * LD * (long long)sizeof(Pair), lane_off[j], Pair{y[2 * j], y[2 * j + 1]});
    };
    auto store_a_end = [&]() {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            A.a_end[(long long)(2 * wave_of[j]) * N + idx] = y[2 * j];
            A.a_end[(long long)(2 * wave_of[j] + 1) * N + idx] = y[2 * j + 1];
            if constexpr (WSUM) A.p_wave_end[(long long)wave_of[j] * N + idx] = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
        }
    };
    if constexpr (TRAJ) store_traj_row(0);
    if (A.n_steps / A.save_every == 0) store_a_end();   // no saved row after z = 0

    auto stage = [&](auto full, const double (&a)[NC], const double (&base)[NC], const double er, const double ei, double (&out)[NC]) {
        if constexpr (decltype(full)::value) split_stage<NL, LOSS>(a, base, er, ei, K.g_h, K.tg_h, K.ha_h, out);
        else split_stage<NL, LOSS>(a, base, er, ei, K.g_d, K.tg_d, K.ha_d, out);
    };
    auto step_on = [&](double (&a)[NC], double &er, double &ei) { carried_step<NC>(a, er, ei, K.rc, K.rs, stage); };
    auto seed_on = [&](const int step, double &er, double &ei) { carried_seed(e_amp, dbd, K.hd, step, er, ei); };
    auto write_summary = [&](const long long bad) {
        if (owns_signal) {
            A.p_end[idx] = pe;
            A.p_max[idx] = pm;
        }
        if (role == 0) A.first_bad[idx] = bad;
        if constexpr (WSUM) {
#pragma unroll
            for (int j = 0; j < NL; ++j) A.p_wave_max[(long long)wave_of[j] * N + idx] = pwm[j];
        }
    };

    // ---- save_every == 1 with a trajectory: every step is a saved row (per row: |A_sig|^2, running maximum, finite test, the
    // lane's NL streaming stores).  (A/B, profiles/r03_split_traj_ab.log: issuing the stores of the previous row one per stage
    // instead of as a burst after the step measured SLOWER, 1.71 vs 1.62 ms for 4 waves at 32 768 points, as did default
    // instead of non-temporal stores: with one wave per SIMD a store that finds the queue full stalls the only wave.)
    if constexpr (TRAJ) {
        if (A.save_every == 1) {
            auto summarise = [&]() {
                pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
                pm = pe > pm ? pe : pm;               // NaN is made to propagate after the loop (it is sticky in y)
            };
            const long long bad = carried_every_step_loop<CHECK>(y, Er, Ei, A.n_steps, step_on, seed_on, nonfinite_on, summarise, store_traj_row);
            if (pe != pe) pm = pe;
            store_a_end();
            write_summary(bad);
            return;
        }
    }

    // ---- z-loop, event driven.  Four steps per trip, then two, then one: with one wave per SIMD a taken back-edge is ~32
    // exposed cycles (tools/issue_probe.hip); four against two measured -0.5 % (config-5 shard) ... -1.2 % (4 096 points, four lanes)
    auto summarise = [&]() {
        pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
        pm = (pe > pm || pe != pe) ? pe : pm;   // np.max propagates NaN
        if constexpr (WSUM) {
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const double pj = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
                pwm[j] = (pj > pwm[j] || pj != pj) ? pj : pwm[j];
            }
        }
    };
    auto save_row = [&](const int row, const bool last) {
        if constexpr (TRAJ) store_traj_row(row);
        if (last) store_a_end();
    };
    write_summary(carried_event_loop<CHECK, 4>(y, Er, Ei, A.n_steps, A.save_every, step_on, seed_on, nonfinite_on, summarise, save_row));
}

// Two lanes per point: register layout only; the per-wave summary without trajectory.
struct SplitLanes {
    static long long lanes(long long n_points) { return 2 * n_points; }
    template <int NW, int CHECK, bool TRAJ, int BLOCK, bool LDS, bool LOSS, bool WSUM, int ROW = 0>
    static constexpr auto kernel() {
        if constexpr (ROW != 0 || LDS || (WSUM && TRAJ)) return nullptr;
        else return rk4_sweep_split_kernel<NW, CHECK, TRAJ, BLOCK, LOSS, WSUM>;
    }
};

}  // namespace psa
