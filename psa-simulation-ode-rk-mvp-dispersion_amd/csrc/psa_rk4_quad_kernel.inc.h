// psa_rk4_quad_kernel.inc.h -- float64 RK4 sweep of the 4-wave model with FOUR LANES PER SWEEP POINT (gfx950).
//
// Why: the reference's own scenarios are tiny sweeps (main.py: 1, 30 and 100 points; BASELINE config 1 is a single run), where
// the chip is empty and the only cost is the length of the dependent instruction stream per lane.  One lane per point issues
// 300.7 instructions per step, two lanes per point 183.6 per lane (psa_rk4_split_kernel.inc.h); here lane r = lane & 3 of a
// quad holds ONE wave of the point (0: pump 1, 1: pump 2, 2: signal, 3: idler) and issues ~155:
//
//     dA_u/dz = (-alpha/2 + i*gamma*f_u) A_u + i*conj(A_v) * F        v = the pair partner (lane ^ 1)
//     F = E_lane * Q,   Q = (A_u A_v) of the OTHER pair (lane ^ 2),   E_lane = 2*gamma*exp(+i*dbeta*z) for the pumps,
//                                                                     its conjugate for the sidebands (yaman_model.py:174-181)
//     f_u = 2*S - |A_u|^2,  S = the quad's sum of |A|^2 (two DPP exchange levels)
//
// Per RHS evaluation and lane: |A|^2 2, S 6 (two moves + an add per level), gamma*f 2, partner's (x, y) 4 moves, A_u*A_v 4,
// the other pair's product 4 moves, F 4, the two 4-deep chains 8  =>  34 (16 of them v_mov_b32_dpp); per step 4 x 34 + 18.
// Every wave of the point goes through the arithmetic it goes through in the two-lane kernel; the only difference is that
// the second lane of a pair forms A_u*A_v with its own wave as the FMA's exact factor (one ulp), so the layouts agree to
// ~1e-12 after 1e4 steps, like one lane and two lanes do.  Measured: x0.81-0.88 of the two-lane kernel's time for
// N <= 4 096 (tools/quad_lane_probe.hip, profiles/r03_quad_lane_probe.log); chosen by
// the cost model of psa_rk4_f64.hip while 4*N lanes still give every wave its own SIMD (N <= 16 384 on MI355X).
// The regrouped RK4 step, the phase recurrence on the absolute seed grid, both z-loops and the save / NaN semantics (exact
// index by replay) are the shared ones of psa_rk4_carried.inc.h -- see that file; trajectory stores as rk4_sweep_kernel.
#pragma once
#include "psa_rk4_carried.inc.h"
#include "psa_rk4_kernel.inc.h"
#include "psa_rk4_split_kernel.inc.h"

namespace psa {

// (ox, oy) = (bx, by) + c * dA/dz of the lane's wave (stage coefficient c folded into g, tg, ha, E as in yaman_stage)
template <bool LOSS>
__device__ __forceinline__ void quad_stage(const double x, const double y, const double bx, const double by, const double Er,
                                           const double Ei, const double g, const double tg, const double ha, double &ox,
                                           double &oy) {
    const double p = fma_(x, x, y * y);
    const double s1 = p + quad_xchg<QUAD_PAIR>(p);             // the pair's |A_u|^2 + |A_v|^2 (the two-lane kernel's own sum)
    const double s = s1 + quad_xchg<QUAD_OTHER>(s1);           // + the other pair's
    const double gj = fma_(-g, p, tg * s);
    const double X = quad_xchg<QUAD_PAIR>(x), Y = quad_xchg<QUAD_PAIR>(y);
    // A_own * A_partner: the two lanes of a pair form the same product with the roles of their FMA's exact and rounded
    // factor exchanged, so their copies may differ in the last bit (the pumps then see pair products one ulp apart): rounding
    // noise of the size every layout has, not worth the four selects per evaluation that would remove it
    const double qr = fma_(x, X, -(y * Y)), qi = fma_(x, Y, y * X);
    const double Qr = quad_xchg<QUAD_OTHER>(qr), Qi = quad_xchg<QUAD_OTHER>(qi);
    const double Fr = fma_(Er, Qr, -(Ei * Qi)), Fi = fma_(Er, Qi, Ei * Qr);
    if constexpr (LOSS) {
        ox = fma_(Y, Fr, fma_(-X, Fi, fma_(-gj, y, fma_(ha, x, bx))));
        oy = fma_(X, Fr, fma_(Y, Fi, fma_(gj, x, fma_(ha, y, by))));
    } else {
        ox = fma_(Y, Fr, fma_(-X, Fi, fma_(-gj, y, bx)));
        oy = fma_(X, Fr, fma_(Y, Fi, fma_(gj, x, by)));
    }
}

// WSUM: the per-wave summary (see rk4_sweep_kernel).  Every lane already tracks |A|^2 of its own wave (pe, pm), so each lane
// writes its wave's rows and no loop state is added.
template <int CHECK, bool TRAJ, int BLOCK, bool LOSS, bool WSUM = false>
__global__ void __launch_bounds__(BLOCK) rk4_sweep_quad_kernel(const SweepArgs<double> A) {
    static_assert(!WSUM || !TRAJ, "the per-wave summary exists for launches without trajectory");
    constexpr int NW = 4;
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long idx = gid >> 2;   // sweep point: the four lanes of a quad share one
    const int role = (int)(gid & 3);  // = the wave this lane holds
    const long long N = A.n_points;
    if (idx >= N) return;             // the four lanes of a quad leave together

    double a[2] = {A.a0[(long long)(2 * role) * A.a0_ld + idx * A.a0_stride],
                   A.a0[(long long)(2 * role + 1) * A.a0_ld + idx * A.a0_stride]};   // (re, im) of the lane's wave
    const double g = A.gamma[idx * A.gamma_stride];
    const double ha = -0.5 * A.alpha[idx * A.alpha_stride];
    const double dbd = (role < 2) ? A.dbeta[idx] : -A.dbeta[idx];   // pumps: E, sidebands: conj(E)
    const CarriedConsts K = carried_consts(g, ha, dbd, A.z_max, A.n_steps);
    const double e_amp = K.tg_d;
    double Er = e_amp, Ei = 0.0;

    double pe = fma_(a[0], a[0], a[1] * a[1]);   // meaningful on the signal's lane (role 2), which writes the summary
    double pm = pe;
    auto nonfinite_on = [&](const double (&v)[2]) -> bool {   // any component of the POINT non-finite
        double t = fma_(v[1], 0.0, fma_(v[0], 0.0, 0.0));
        t += quad_xchg<QUAD_PAIR>(t);
        t += quad_xchg<QUAD_OTHER>(t);
        return t != t;
    };

    // trajectory rows [row][wave][ld][2]: the lane's wave is its role, so the address is a wave-uniform row base plus the
    // per-lane constant 32-bit offset (role * ld + idx) * 16 (the C-ABI keeps 4 * ld * 16 B < 2^32 for these launches)
    using Pair = typename PairOf<double>::type;
    const long long LD = A.traj_ld;
    const unsigned lane_off = (unsigned)((unsigned long long)(role * LD + idx) * sizeof(Pair));
    auto store_traj_row = [&](const int r) {
        store_pair_nt(reinterpret_cast<const char *>(A.traj) + (long long)r * NW * LD * (long long)sizeof(Pair), lane_off, Pair{a[0], a[1]});
    };
    auto store_a_end = [&]() {
        A.a_end[(long long)(2 * role) * N + idx] = a[0];
        A.a_end[(long long)(2 * role + 1) * N + idx] = a[1];
        if constexpr (WSUM) A.p_wave_end[(long long)role * N + idx] = fma_(a[0], a[0], a[1] * a[1]);
    };
    if constexpr (TRAJ) store_traj_row(0);
    if (A.n_steps / A.save_every == 0) store_a_end();   // no saved row after z = 0

    auto stage = [&](auto full, const double (&y)[2], const double (&base)[2], const double er, const double ei, double (&out)[2]) {
        if constexpr (decltype(full)::value) quad_stage<LOSS>(y[0], y[1], base[0], base[1], er, ei, K.g_h, K.tg_h, K.ha_h, out[0], out[1]);
        else quad_stage<LOSS>(y[0], y[1], base[0], base[1], er, ei, K.g_d, K.tg_d, K.ha_d, out[0], out[1]);
    };
    auto step_on = [&](double (&y)[2], double &er, double &ei) { carried_step<2>(y, er, ei, K.rc, K.rs, stage); };
    auto seed_on = [&](const int step, double &er, double &ei) { carried_seed(e_amp, dbd, K.hd, step, er, ei); };
    auto write_summary = [&](const long long bad) {
        if (role == 2) {
            A.p_end[idx] = pe;
            A.p_max[idx] = pm;
        }
        if (role == 0) A.first_bad[idx] = bad;
        if constexpr (WSUM) A.p_wave_max[(long long)role * N + idx] = pm;
    };

    // ---- save_every == 1 with a trajectory: every step is a saved row
    if constexpr (TRAJ) {
        if (A.save_every == 1) {
            auto summarise = [&]() {
                pe = fma_(a[0], a[0], a[1] * a[1]);
                pm = pe > pm ? pe : pm;               // NaN is made to propagate after the loop (it is sticky in y)
            };
            const long long bad = carried_every_step_loop<CHECK>(a, Er, Ei, A.n_steps, step_on, seed_on, nonfinite_on, summarise, store_traj_row);
            if (pe != pe) pm = pe;
            store_a_end();
            write_summary(bad);
            return;
        }
    }

    // ---- z-loop, event driven.  Four steps per trip, then two, then one: with one wave per SIMD a taken back-edge is ~32
    // exposed cycles (tools/issue_probe.hip); four against two measured -0.5 % (config-5 shard) ... -1.2 % (4 096 points, four lanes)
    auto summarise = [&]() {
        pe = fma_(a[0], a[0], a[1] * a[1]);
        pm = (pe > pm || pe != pe) ? pe : pm;
    };
    auto save_row = [&](const int row, const bool last) {
        if constexpr (TRAJ) store_traj_row(row);
        if (last) store_a_end();
    };
    write_summary(carried_event_loop<CHECK, 4>(a, Er, Ei, A.n_steps, A.save_every, step_on, seed_on, nonfinite_on, summarise, save_row));
}

// Four lanes per point: the 4-wave model's register layout only; the per-wave summary without trajectory.
struct QuadLanes {
    static long long lanes(long long n_points) { return 4 * n_points; }
    template <int NW, int CHECK, bool TRAJ, int BLOCK, bool LDS, bool LOSS, bool WSUM, int ROW = 0>
    static constexpr auto kernel() {
        if constexpr (ROW != 0 || NW != 4 || LDS || (WSUM && TRAJ)) return nullptr;
        else return rk4_sweep_quad_kernel<CHECK, TRAJ, BLOCK, LOSS, WSUM>;
    }
};

}  // namespace psa
