// psa_rk4_kernel.inc.h -- the RK4 sweep kernel for gfx950 (included by psa_rk4_f64.hip / psa_rk4_f32.hip).
//
// One sweep point per lane, the whole z-loop inside the kernel, state in VGPRs.
// Replaces, per point:  integrators.integrate_fixed_step (integrators.py:68-142) driving
// integrators.rk4_step (:25-61) on yaman_model.rhs_yaman_simplified (yaman_model.py:10-52),
// plus the saved-row reduction of the sweep drivers (scan_mismtach.py:376-381).
//
// What bounds it: FP64 vector FMA issue (16 lanes/clk/SIMD on CDNA4), NOT HBM and not MFMA:
// a point reads 8..88 B and writes 88 B for its entire z-loop, and the RHS is an elementwise
// complex polynomial (no contraction to tile).  So the design rules here are
//   * minimum DP instructions per step (288 for 4 waves, 144 where waves 2 and 4 mirror 1 and 3; see the counts in DESIGN.md),
//   * no transcendental in the steady-state loop.  The fused float64 4-wave step (FRAME) integrates the sidebands in a frame
//     anchored at the midpoint of each step, where the phase factor 2*d*gamma*exp(i*dbeta*(z - z_mid)) takes the same four
//     values in every step -- lane constants, two of them real -- and the state moves to the next step's frame by one
//     rotation of the sidebands: nothing is carried and nothing re-seeded.  Only what leaves the kernel as amplitudes (A[-1],
//     trajectory rows) is taken out of the frame, by F(step) = exp(i*dbeta*(z_step + d)/2): one function of the absolute step
//     index, an exact sincos at the multiples of RESYNC and one rotation per step from there, carried by the trajectory
//     instantiations (+4 per step) and built once, where A[-1] is stored, by the others.  Six waves, float32 and the LDS
//     variant carry E(z) = 2*gamma*exp(i*dbeta*z) by a complex rotation per half step, re-seeded from an exact sincos at
//     every multiple of RESYNC steps (64 in float64: drift <= 128 multiplications ~1.4e-14, far inside the 1e-9 budget),
//   * all per-lane arrays statically indexed and in VGPRs (178 for the bench instantiation: 2 waves/SIMD; capping
//     at 168 (3 waves) or 128 (4 waves, 16 spilled) was measured no faster -- the loop is issue-bound),
//   * wave-uniform control flow only (save stride, resync and NaN tracking never diverge),
//   * SoA global layout: every load/store instruction of a wave is one contiguous 512-B run.
//
// The independent variable follows the reference grid: z_i = i * (z_max / n_steps)
// (np.linspace, integrators.py:195) formed from the INTEGER step index, never accumulated.
#pragma once
#include "psa_launch.inc.h"
#include "psa_rk4_prims.inc.h"
#include "psa_rk4_stage.inc.h"

namespace psa {

// ---- the sweep kernel ------------------------------------------------------------------------------
// LDS = true is the layout the north-star sketches (state and k1..k4 staged in LDS, [component][lane] so a wave's
// ds_read/ds_write_b64 touches 64 consecutive 8-byte words: conflict-free).  It exists for the A/B in DESIGN.md
// section 5: the register-resident form wins because the LDS round trips buy nothing (no data is shared
// between lanes) and cost issue slots next to an already saturated FP64 pipe.
#ifndef PSA_SWEEP_KERNEL_ATTR   // A/B hook (tools/ab_build.sh): e.g. -DPSA_SWEEP_KERNEL_ATTR='__attribute__((amdgpu_waves_per_eu(3)))'
#define PSA_SWEEP_KERNEL_ATTR
#endif
// WSUM = true adds the per-wave summary (A.p_wave_end / A.p_wave_max, SoA [NW][N]; register layout without trajectory
// only): |A_j|^2 of every wave with the expression the signal's summary uses, so wave 2's columns are p_end / p_max bit for
// bit.  The end value is formed where a_end is written; only the NW running maxima are loop state.
//
// The per-lane body is sweep_point<..., MIRROR>: everything behind the a0 loads.  MIRROR = true (float64, 4 waves, register
// layout) is the same body on HALF the state -- y = [Re A1, Im A1, Re A3, Im A3], the stage yaman_stage_mirrored -- for
// points whose a0 has A2 == A1 and A4 == A3 bit for bit (every scenario of the reference: equal pumps, equal signal and
// idler seeds, zero phases).  The step, the rotations, the re-seeds, the event loop, the checkpoint and replay, the block
// test and the tail are the one text below for both; the outputs are the full record, waves 2 and 4 written from the
// registers of waves 1 and 3.  144 DP instructions per step instead of 288 (32 + 30 + 30 + 32 stages, 12 + 4, 4 to move the frame).
//
// ROW > 0 (the frame-anchored summary kernels only) is the same body for launches whose save_every IS ROW, known when the
// kernel is compiled: a saved row of the z-loop is then ROW steps in straight line (see "z-loop by saved rows" below).
template <typename T, int NW, int CHECK, bool TRAJ, int BLOCK, bool LDS, bool LOSS, bool WSUM, bool MIRROR, int ROW = 0>
__device__ __forceinline__ void sweep_point(const SweepArgs<T> &A, const long long idx, T (&y)[MIRROR ? NW : 2 * NW]) {
    static_assert(!MIRROR || (sizeof(T) == 8 && NW == 4 && !LDS), "the mirrored body exists for the fused float64 4-wave step");
    static_assert(ROW == 0 || (sizeof(T) == 8 && NW == 4 && !LDS && !TRAJ), "a fixed row length exists for the row-driven z-loop");
    constexpr int NC = 2 * NW;                  // components of the record
    constexpr int NS = MIRROR ? NW : NC;        // components of the state this lane carries
    constexpr int NWS = NS / 2;                 // waves of that state
    constexpr int SIG = MIRROR ? 2 : 4;         // Re A_sig in the state
    constexpr int NP = (NW - 2) / 2;
    constexpr int RESYNC = Phase<T>::RESYNC;
    auto at = [](const int c) { return MIRROR ? (((c >> 2) << 1) | (c & 1)) : c; };   // record component -> state component
    const long long N = A.n_points;

    const T g = A.gamma[idx * A.gamma_stride];
    const T tg = g + g;
    const T ha = T(-0.5) * A.alpha[idx * A.alpha_stride];
    double dbd[NP];
    dbd[0] = (double)A.dbeta[idx];
    if constexpr (NP == 2) dbd[1] = (double)A.dbeta2[idx];

    const double hd = A.z_max / (double)A.n_steps;  // np.linspace step
    const T h = (T)hd, hh = (T)(0.5 * hd), h6 = (T)(hd / 6.0);
    // stage coefficients folded into the physics constants: d = h/2 (stages 1, 2, 4) and h (stage 3)
    const T g_d = hh * g, tg_d = hh * tg, ha_d = hh * ha;
    const T g_h = h * g, tg_h = h * tg, ha_h = h * ha;
    const T third = T(1.0 / 3.0);
    constexpr bool FUSE = (sizeof(T) == 8) && !LDS;   // fused-stage step: float64 register variant only
    const T e_amp = FUSE ? tg_d : tg;  // modulus of the phase factor: 2*d*gamma (fused) or 2*gamma
    // FRAME: the fused 4-wave step integrates the sidebands in a frame anchored at the midpoint of each step (rk4_step_on)
    // and carries no phase factor at all
    constexpr bool FRAME = FUSE && NW == 4;

    T rc[NP], rs[NP], Er[NP], Ei[NP];  // half-step rotator and the running 2*gamma*exp(i dbeta z)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        Phase<T>::eval(dbd[p] * (0.5 * hd), rc[p], rs[p]);
        Er[p] = e_amp;
        Ei[p] = T(0);
    }
    // FRAME: the phase factor at the two ends of a step, e*conj(r) and e*r = (ec, -+es); e (= tg_d) and 2e (= tg_h) in between
    const T ec = e_amp * rc[0], es = e_amp * rs[0];
    // F(step) = exp(i*dbeta*(z_step + d)/2): what the sidebands of the frame of step `step` carry over the record's.
    // ONE function of the absolute step index -- an exact sincos at the multiples of RESYNC, one rotation by r per step
    // from there -- so that a row is the same bits whether F was carried through the loop (TRAJ) or built for that row.
    auto frame_seed = [&](const int step, T &fc, T &fs) {   // step a multiple of RESYNC
        Phase<T>::eval(dbd[0] * (0.5 * fma_((double)step, hd, 0.5 * hd)), fc, fs);
    };
    auto frame_at = [&](const int step, T &fc, T &fs) {
        const int k = step % RESYNC;
        frame_seed(step - k, fc, fs);
#pragma nounroll
        for (int q = 0; q < k; ++q) rotate(fc, fs, rc[0], rs[0]);
    };
    // record <- frame: pumps as they are, sidebands times conj(F), one expression for both (the exchange still permutes).
    // The summaries are moduli of the FRAME's sidebands and must be the record's to a few ulp (|A_j|^2 of a row against
    // p_wave_end / p_wave_max: 1e-15).  F carried k steps from a seed is off unit modulus by k roundings of r that all have one
    // sign (|r| - 1 is a constant of the lane, up to 5.5e-17): up to 7e-15 in |F|^2 before the next seed.  So the F that is
    // applied is renormalised to first order, F * (1 - (|F|^2 - 1)/2), the defect formed without cancellation error; what is
    // left is its square, ~1e-29.  A function of F alone: carried or rebuilt, the row has the same bits.
    auto leave_frame = [&](const T (&b)[NS], const T fc, const T fs, T (&a)[NS]) {
        const T ce = T(-0.5) * fma_(fs, fs, fma_(fc, fc, T(-1)));
        const T nc = fma_(fc, ce, fc), ns = fma_(fs, ce, fs);
#pragma unroll
        for (int c = 0; c < SIG; ++c) a[c] = b[c];
#pragma unroll
        for (int c = SIG; c < NS; c += 2) {
            a[c] = fma_(b[c], nc, b[c + 1] * ns);
            a[c + 1] = fma_(b[c + 1], nc, -(b[c] * ns));
        }
    };
    T Fc = T(1), Fs = T(0);            // FRAME && TRAJ: F of the step about to run, carried through the loop

    T pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);  // |A_sig|^2 at the last saved row (z = 0 is a saved row)
    T pm = pe;                             // np.max over saved rows
    long long bad = -1;
    T pwm[WSUM ? NWS : 1];                 // WSUM: np.max of |A_j|^2 over saved rows, every wave of the state
    if constexpr (WSUM) {
#pragma unroll
        for (int j = 0; j < NWS; ++j) pwm[j] = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
    }
    auto store_a_end = [&](const T (&a)[NS]) {   // A[-1] (a: y in the record's variables); with WSUM also |A_j|^2 of that row, from y
#pragma unroll
        for (int c = 0; c < NC; ++c) A.a_end[(long long)c * N + idx] = a[at(c)];
        if constexpr (WSUM) {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const T xr = y[at(2 * j)], xi = y[at(2 * j + 1)];
                A.p_wave_end[(long long)j * N + idx] = fma_(xr, xr, xi * xi);
            }
        }
    };

    const int se = A.save_every;
    const int n_rows = A.n_steps / se;                                 // saved rows after z = 0
    const int n_run = (CHECK != CHECK_NONE) ? A.n_steps : n_rows * se;  // the tail only matters for check_nan

    // trajectory rows: device layout [row][wave][N][2] -- each lane stores one (re, im) pair = 16 B (f64), so a wave
    // instruction writes 1 KiB contiguously (the widest coalesced store; half the store instructions of per-component rows).
    // The wave-uniform part of the address (row, wave) stays in SGPRs and the lane contributes a 32-bit byte offset
    // (global_store ... saddr form): no vector instruction is spent on addressing.  The C-ABI keeps N * sizeof(Pair) < 2^32
    // for trajectory launches.
    using Pair = typename PairOf<T>::type;
    const long long LD = A.traj_ld;   // points per (row, wave) region: N, or N padded off a power of two (psa_traj_ld)
    const unsigned lane_off = (unsigned)idx * (unsigned)sizeof(Pair);
    auto store_traj_row_of = [&](const int r, const T (&a)[NS]) {
        const char *rowb = reinterpret_cast<const char *>(A.traj) + (long long)r * NW * LD * (long long)sizeof(Pair);
#pragma unroll
        for (int j = 0; j < NW; ++j)
            store_pair_nt(rowb + (long long)j * LD * (long long)sizeof(Pair), lane_off, Pair{a[at(2 * j)], a[at(2 * j + 1)]});
    };
    auto store_traj_row = [&](const int r) {     // FRAME: F is F(step) of the row's step
        if constexpr (FRAME) {
            T a[NS];
            leave_frame(y, Fc, Fs, a);
            store_traj_row_of(r, a);
        } else {
            store_traj_row_of(r, y);
        }
    };
    auto store_a_end_at = [&](const int step) {  // A[-1] = the state after `step` steps
        if constexpr (FRAME) {
            T a[NS], fc = Fc, fs = Fs;
            if constexpr (!TRAJ) frame_at(step, fc, fs);
            leave_frame(y, fc, fs, a);
            store_a_end(a);
        } else {
            store_a_end(y);
        }
    };
    // z = 0 is a0 as given: row 0, and A[-1] when no row follows, are written before the frame is entered
    if constexpr (TRAJ) store_traj_row_of(0, y);
    if (n_rows == 0) store_a_end(y);
    if constexpr (FRAME) {                       // B = A * F(0) on the sidebands
        frame_seed(0, Fc, Fs);
#pragma unroll
        for (int c = SIG; c < NS; c += 2) rotate(y[c], y[c + 1], Fc, Fs);
    }

    // LDS-staged variant: sm_k[stage][component][lane] and sm_y[component][lane] (volatile: the traffic is the point)
    __shared__ T sm_store[LDS ? 5 * NC * BLOCK : 1];
    volatile T *sm_y = sm_store + threadIdx.x;
    volatile T *sm_k = sm_store + NC * BLOCK + threadIdx.x;
    if constexpr (LDS) {
#pragma unroll
        for (int c = 0; c < NC; ++c) sm_y[c * BLOCK] = y[c];
    }
    auto rk4_step_lds = [&](const int step_index) {
        if constexpr (LDS) {
            T k[NC], ys[NC];
            const T coef[3] = {hh, hh, h};
#pragma unroll
            for (int c = 0; c < NC; ++c) ys[c] = sm_y[c * BLOCK];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                yaman_rhs<T, NW>(ys, Er, Ei, g, tg, ha, k);
#pragma unroll
                for (int c = 0; c < NC; ++c) sm_k[(st * NC + c) * BLOCK] = k[c];
                if (st == 0 || st == 2) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) rotate(Er[p], Ei[p], rc[p], rs[p]);
                }
                if (st < 3) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) ys[c] = fma_(coef[st], (T)sm_k[(st * NC + c) * BLOCK], (T)sm_y[c * BLOCK]);
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const T k1 = sm_k[(0 * NC + c) * BLOCK], k2 = sm_k[(1 * NC + c) * BLOCK];
                const T k3 = sm_k[(2 * NC + c) * BLOCK], k4 = sm_k[(3 * NC + c) * BLOCK];
                y[c] = fma_(h6, fma_(T(2), k3, fma_(T(2), k2, k1)) + k4, (T)sm_y[c * BLOCK]);
                sm_y[c * BLOCK] = y[c];
            }
            if constexpr (CHECK == CHECK_EXACT) {
                if (bad < 0 && any_nonfinite<T, NC>(y)) bad = step_index;
            }
        }
    };

    // ---- one classic RK4 step (integrators.py:54-59) in 288 DP instructions (4 waves; 144 on the mirrored state; six
    // waves, which carry the phase factor, 468).
    // Each stage's axpy is folded into the RHS chains (yaman_stage, FUSED): with d = h/2
    //     Y2 = y + d*f(z, y)          Y3 = y + d*f(z+d, Y2)          Y4 = y + 2d*f(z+d, Y3)
    //     t  = Y2 + 2*Y3 + Y4 - 4*y                 ( = d*k1 + 2d*k2 + 2d*k3 )
    //     D  = t + d*f(z+h, Y4)                     ( = d*(k1 + 2*k2 + 2*k3 + k4) )
    //     y <- y + D/3                              ( = y + h/6*(k1 + 2*k2 + 2*k3 + k4) )
    // which is the reference's k1..k4 combination regrouped (no change of variables, same truncation error; the
    // regrouping costs ~1 ulp(y) of rounding noise per step, ~1e-13 after 1e5 steps).  Six waves: (Er, Ei) carries
    // 2*d*gamma*exp(i*dbeta*z), on entry at z_step, on exit rotated to z_step + h.
    // MIRROR: the same step on the half state, every stage yaman_stage_mirrored.
    auto stage = [&](auto reale, const T (&a)[NS], const T (&base)[NS], const T (&er)[NP], const T (&ei)[NP], const T g_c,
                     const T tg_c, const T ha_c, T (&out)[NS]) {
        constexpr bool RE = decltype(reale)::value;
        if constexpr (MIRROR) yaman_stage_mirrored<T, LOSS, true, RE>(a, base, er[0], ei[0], g_c, tg_c + tg_c, ha_c, out);
        else yaman_stage<T, NW, true, LOSS, true, RE>(a, base, er, ei, g_c, tg_c, ha_c, out);
    };
    constexpr std::false_type cplx{};
    constexpr std::true_type real{};
    // FRAME (4 waves): 288 (144 mirrored).  A Runge-Kutta step is exactly invariant under a CONSTANT linear change of
    // variables, so the step is taken on B = diag(1, 1, tau, tau) * A with tau = exp(+i*dbeta*(z + d)/2) fixed over the step:
    // the equations keep their form with the phase factor 2*d*gamma*exp(i*dbeta*(z' - (z + d))), which is e*conj(r), e, e, e*r
    // at the four stages of EVERY step (stage 3 takes it doubled, with its coefficient h) -- lane constants, real in the
    // middle -- and nothing is carried or re-seeded.  Moving
    // from the frame of one step to the next multiplies the sidebands by r = exp(i*dbeta*d), the same expression for both
    // (so the exchange of the members still permutes the outputs bit for bit).  Between steps the map is linear and exact:
    // method, grid and truncation error are the reference's, only rounding moves: the modulus of the rounded r, <= 5.5e-17
    // off one, now accumulates in the sidebands -- ONE rotation per step, so their moduli are off by n (|r| - 1) of themselves,
    // <= 5.5e-12 after 1e5 steps, as long as the pumps are undepleted (the equations are then linear in the sidebands).  That
    // product is NOT a bound on the result: |r| - 1 acts as a gain error on both sidebands, and where they have grown to the
    // pumps' scale the propagation carries it further.  Measured against an 80-bit run on G8's 64 mismatches at 1e5 steps:
    // a_end off by up to 1.5e-11 of the point's largest wave, 2.7 n (|r| - 1); a scaling by each lane's own |r| planted into
    // the 80-bit run gives 1.46e-11, by 1 + 5.5e-17 in every lane 2.1e-11 (tests/test_gpu_truth.py,
    // tests/truth_cases.g8_long_frame_drift).  The record leaves the frame by conj(F(step)).
    auto rk4_step_on = [&](T (&y)[NS], T (&Er)[NP], T (&Ei)[NP]) {
        T Y2[NS], Y3[NS], Y4[NS], t[NS], D[NS];
        if constexpr (FRAME) {
            const T c1[NP] = {ec}, s1[NP] = {-es}, s4[NP] = {es}, e1[NP] = {tg_d}, e2[NP] = {tg_h};
            stage(cplx, y, y, c1, s1, g_d, tg_d, ha_d, Y2);    // Y2 = y + d k1      e*conj(r)
            stage(real, Y2, y, e1, e1, g_d, tg_d, ha_d, Y3);   // Y3 = y + d k2      e
            stage(real, Y3, y, e2, e2, g_h, tg_h, ha_h, Y4);   // Y4 = y + h k3      2e
#pragma unroll
            for (int c = 0; c < NS; ++c) t[c] = fma_(T(2), Y3[c], fma_(T(-4), y[c], Y2[c])) + Y4[c];
            stage(cplx, Y4, t, c1, s4, g_d, tg_d, ha_d, D);    // D = t + d k4       e*r
#pragma unroll
            for (int c = 0; c < NS; ++c) y[c] = fma_(D[c], third, y[c]);
#pragma unroll
            for (int c = SIG; c < NS; c += 2) rotate(y[c], y[c + 1], rc[0], rs[0]);   // into the frame of the next step
            return;
        }
        stage(cplx, y, y, Er, Ei, g_d, tg_d, ha_d, Y2);  // Y2 = y + d k1
#pragma unroll
        for (int p = 0; p < NP; ++p) rotate(Er[p], Ei[p], rc[p], rs[p]);  // z + h/2
        stage(cplx, Y2, y, Er, Ei, g_d, tg_d, ha_d, Y3);  // Y3 = y + d k2
        T E2r[NP], E2i[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            E2r[p] = Er[p] + Er[p];
            E2i[p] = Ei[p] + Ei[p];
        }
        stage(cplx, Y3, y, E2r, E2i, g_h, tg_h, ha_h, Y4);  // Y4 = y + h k3
#pragma unroll
        for (int c = 0; c < NS; ++c) t[c] = fma_(T(2), Y3[c], fma_(T(-4), y[c], Y2[c])) + Y4[c];
#pragma unroll
        for (int p = 0; p < NP; ++p) rotate(Er[p], Ei[p], rc[p], rs[p]);  // z + h
        stage(cplx, Y4, t, Er, Ei, g_d, tg_d, ha_d, D);  // D = t + d k4
#pragma unroll
        for (int c = 0; c < NS; ++c) y[c] = fma_(D[c], third, y[c]);
    };
    // The per-step finite test of the reference (integrators.py:132-135) is NOT in the float64 step: CHECK_EXACT finds the
    // exact index by REPLAY (below) -- the forward pass tests once per saved row, like CHECK_BLOCK.
    auto rk4_step_reg = [&](const int) {
        rk4_step_on(y, Er, Ei);
        if constexpr (FRAME && TRAJ) rotate(Fc, Fs, rc[0], rs[0]);   // F of the next step (re-seeded where a row is due)
    };

    // ---- float32: the classic low-storage form (y, y_stage, accumulator; 320 instructions).  The regrouping above
    // quantises every stage increment to ulp(y); harmless at 1e-16 but measured 17x worse at float32 (6.7e-3 vs
    // 3.8e-4 relative after 1e4 steps), so single precision keeps k1..k4 at full precision.
    T y_lo[NS];  // Kahan residue of the state (float32 path only)
#pragma unroll
    for (int c = 0; c < NS; ++c) y_lo[c] = T{};
    auto rk4_step_classic = [&](const int step_index) {
        if constexpr (!FUSE) {
            T k[NC], ys[NC], acc[NC];
            yaman_rhs<T, NW, LOSS>(y, Er, Ei, g, tg, ha, k);  // k1 at z
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                acc[c] = k[c];
                ys[c] = fma_(hh, k[c], y[c]);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) rotate(Er[p], Ei[p], rc[p], rs[p]);  // z + h/2
            yaman_rhs<T, NW, LOSS>(ys, Er, Ei, g, tg, ha, k);  // k2
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                acc[c] = fma_(T(2), k[c], acc[c]);
                ys[c] = fma_(hh, k[c], y[c]);
            }
            yaman_rhs<T, NW, LOSS>(ys, Er, Ei, g, tg, ha, k);  // k3
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                acc[c] = fma_(T(2), k[c], acc[c]);
                ys[c] = fma_(h, k[c], y[c]);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) rotate(Er[p], Ei[p], rc[p], rs[p]);  // z + h
            yaman_rhs<T, NW, LOSS>(ys, Er, Ei, g, tg, ha, k);  // k4
            // compensated (Kahan) state update: keeps the part of the increment that y + inc rounds away (see the
            // packed kernel); without it float32 drifts ~n * ulp and misses its 1e-3 tolerance at 1e6 steps.
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const T inc = fma_(h6, acc[c] + k[c], y_lo[c]);
                const T sum = y[c] + inc;
                y_lo[c] = inc - (sum - y[c]);
                y[c] = sum;
            }
            if constexpr (CHECK == CHECK_EXACT) {
                if (bad < 0 && any_nonfinite<T, NC>(y)) bad = step_index;
            }
        }
    };
    auto rk4_step = [&](const int step_index) {
        if constexpr (FUSE) rk4_step_reg(step_index);
        else rk4_step_classic(step_index);
    };

    auto write_summary = [&]() {
        A.p_end[idx] = pe;
        A.p_max[idx] = pm;
        A.first_bad[idx] = bad;
        if constexpr (WSUM) {
#pragma unroll
            for (int j = 0; j < NW; ++j) A.p_wave_max[(long long)j * N + idx] = pwm[at(2 * j) / 2];
        }
    };
    auto seed_phase_on = [&](const int step, T (&Er)[NP], T (&Ei)[NP]) {   // exact re-seed of the phase recurrence at z = step * h
        const double z = (double)step * hd;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            T c, s;
            Phase<T>::eval(dbd[p] * z, c, s);
            Er[p] = e_amp * c;
            Ei[p] = e_amp * s;
        }
    };
    auto seed_phase = [&](const int step) { seed_phase_on(step, Er, Ei); };

    // ---- CHECK_EXACT for the float64 register variant: exact first_bad_step at the price of the block test.  The state at
    // the last test point (y, and with six waves the carried phase factor) is kept; when a test finds a lane of the
    // wave newly non-finite, the steps since then are REPLAYED on a copy with the reference's per-step test
    // (integrators.py:132-135).  The replay repeats the forward pass operation for operation (same chunks, same re-seeds,
    // same FMA sequence), so it reproduces this kernel's own trajectory bit for bit and the index it finds is exact.  Only
    // waves with a failing lane ever take the (wave-uniform) branch: +16 VGPRs (+8 on the mirrored state), no instruction in the steady-state loop
    // (the per-step test cost 9.9 of 310.6 instructions per step, profiles/r03_c2x_pmc.csv).
    constexpr bool REPLAY = FUSE && CHECK == CHECK_EXACT;
    T y_chk[REPLAY ? NS : 1], Er_chk[REPLAY && !FRAME ? NP : 1], Ei_chk[REPLAY && !FRAME ? NP : 1];   // FRAME carries no phase factor
    int i_chk = 0;
    auto checkpoint = [&](const int step) {
        if constexpr (REPLAY) {
#pragma unroll
            for (int c = 0; c < NS; ++c) y_chk[c] = y[c];
            if constexpr (!FRAME) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    Er_chk[p] = Er[p];
                    Ei_chk[p] = Ei[p];
                }
            }
            i_chk = step;
        }
    };
    auto exact_test = [&](const int i_now) {   // at a test point: y is the state after step i_now - 1
        if constexpr (REPLAY) {
            const bool newly_bad = bad < 0 && any_nonfinite<T, NS>(y);
            if (__builtin_amdgcn_ballot_w64(newly_bad) != 0) {
                T yy[NS], er[NP], ei[NP];
#pragma unroll
                for (int c = 0; c < NS; ++c) yy[c] = y_chk[c];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    er[p] = FRAME ? T(0) : Er_chk[FRAME ? 0 : p];
                    ei[p] = FRAME ? T(0) : Ei_chk[FRAME ? 0 : p];
                }
                int ii = i_chk;
                while (ii < i_now) {
                    if constexpr (!FRAME) {
                        if (ii % RESYNC == 0) seed_phase_on(ii, er, ei);   // the forward pass seeds at the same steps
                    }
                    const int to_seed = FRAME ? i_now - ii : RESYNC - ii % RESYNC;   // FRAME: the step has no seeds to repeat
                    const int e = (i_now - ii > to_seed) ? ii + to_seed : i_now;
#pragma nounroll
                    for (int st = ii; st < e; ++st) {
                        rk4_step_on(yy, er, ei);
                        if (bad < 0 && any_nonfinite<T, NS>(yy)) bad = st;
                    }
                    ii = e;
                }
            }
            checkpoint(i_now);
        }
    };

    // ---- save_every == 1 with a trajectory: EVERY step is a saved row (integrators.py:137), the path's HBM-bound regime
    // (64 B per point per step against ~300 FP64 instructions: right at the ridge).  A dedicated loop keeps the per-row
    // work to what the row needs -- |A_sig|^2, a running maximum, the block-mode finite test, four streaming stores -- with
    // no event bookkeeping between steps, two steps per trip so the stores of one row issue under the next step.
    if constexpr (TRAJ && !LDS) {
        if (se == 1) {
            auto save_row = [&](const int r) {
                pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
                pm = pe > pm ? pe : pm;               // NaN is made to propagate after the loop (it is sticky in y)
                if constexpr (CHECK == CHECK_BLOCK || (CHECK == CHECK_EXACT && FUSE)) {   // a row is a step here: exact either way
                    if (bad < 0 && any_nonfinite<T, NS>(y)) bad = r - 1;
                }
                store_traj_row(r);
            };
            int i = 0;
            while (i < n_run) {                       // n_run == n_steps == n_rows
                if constexpr (!FRAME) seed_phase(i);
                const int end = (n_run - i > RESYNC) ? i + RESYNC : n_run;
                for (; i + 2 <= end; i += 2) {        // i is even: only the second row of a trip can fall on a multiple of RESYNC
                    rk4_step(i);
                    save_row(i + 1);
                    rk4_step(i + 1);
                    if constexpr (FRAME) {
                        if ((i + 2) % RESYNC == 0) frame_seed(i + 2, Fc, Fs);
                    }
                    save_row(i + 2);
                }
                if (i < end) {
                    rk4_step(i);
                    save_row(i + 1);
                    ++i;
                }
            }
            if (pe != pe) pm = pe;                    // np.max over the saved rows propagates NaN
            if constexpr (FRAME) {
                T a[NS];
                leave_frame(y, Fc, Fs, a);            // F(n_run), as the last row's
#pragma unroll
                for (int c = 0; c < NC; ++c) A.a_end[(long long)c * N + idx] = a[at(c)];
            } else {
#pragma unroll
                for (int c = 0; c < NC; ++c) A.a_end[(long long)c * N + idx] = y[at(c)];
            }
            write_summary();
            return;
        }
    }

    // ---- z-loop by saved rows: the frame-anchored summary kernels (FRAME without trajectory) have no seed event, so the only
    // events are the rows and the end.  One loop over blocks of steps -- n_rows of save_every, then the unsaved tail (check_nan
    // only) through the same step text -- with no bookkeeping between the steps of a block: the odd step and the odd pair
    // first, then trips of PSA_ROW_TRIP steps.  With one wave per SIMD every taken branch is an exposed instruction refetch
    // (~32 cycles, profiles/r03_issue_probe.log): a row of the event loop below took nine at save_every = 10 (eleven in the general
    // loop), this one takes three (profiles/row_loop.log; tools/isa_loop_stats.py --row walks a row through the built loop).
    // The row itself is straight-line -- |A_sig|^2, the maxima, the block-mode test as a select -- and ONE counter, `until`,
    // stands between it and the back-edge.  Everything rare hangs off that counter reaching zero: the exact test (REPLAY),
    // and at the last row A[-1], the power summaries and the switch to the tail.  The tail runs as one more block whose row
    // work is discarded: p_end / p_max (and the per-wave maxima) are already in memory, and in block mode the row's test at
    // i = n_run is the tail's (first_bad_step = n_run - 1).
    // The exact test need not run on every row: a non-finite component never becomes finite again (every chain of the next
    // stage and the state update take it in; the save_every == 1 loop above relies on the same), so a lane that fails anywhere
    // in a group of rows is still non-finite at the group's end, and the replay from the checkpoint finds the same first step
    // whatever the distance.  The forward test, ballot and checkpoint run after every G-th row, G the largest count with
    // G * save_every <= 64 (at least 1), after the last row and after the tail: a replay never covers more than
    // max(save_every, 64) steps.  Groups are counted in rows from z = 0, so what is tested does not depend on the wave.
#ifndef PSA_ROW_TRIP            // A/B hook (make EXTRA=-DPSA_ROW_TRIP=2): steps per trip of the row loop, 4 or 2
#define PSA_ROW_TRIP 4
#endif
    if constexpr (FRAME && !TRAJ) {
        static_assert(PSA_ROW_TRIP == 4 || PSA_ROW_TRIP == 2, "the row loop runs 4 or 2 steps per trip");
        auto write_powers = [&]() {
            A.p_end[idx] = pe;
            A.p_max[idx] = pm;
            if constexpr (WSUM) {
#pragma unroll
                for (int j = 0; j < NW; ++j) A.p_wave_max[(long long)j * N + idx] = pwm[at(2 * j) / 2];
            }
        };
        const int tail = n_run - n_rows * se;
        const int rows_per_test = se < 64 ? 64 / se : 1;
        auto span_of = [&](const int rows) { return (REPLAY && rows > rows_per_test) ? rows_per_test : rows; };
        int left = n_rows > 0 ? n_rows : -1;   // saved rows still ahead of the last rare stop; -1: the block is the tail
        int m = left < 0 ? tail : se;          // steps per block, and its full trips (carried: the loop forms neither per row)
        int trips = m / PSA_ROW_TRIP;
        int span = left < 0 ? 1 : span_of(left);
        [[maybe_unused]] int i_row = 0;        // block mode: the step index of the row
        auto row_work = [&](const int steps) {   // the row after a block of `steps` steps
            pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
            pm = (pe > pm || pe != pe) ? pe : pm;  // np.max propagates NaN
            if constexpr (WSUM) {
#pragma unroll
                for (int j = 0; j < NWS; ++j) {
                    const T pj = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
                    pwm[j] = (pj > pwm[j] || pj != pj) ? pj : pwm[j];
                }
            }
            if constexpr (CHECK == CHECK_BLOCK) {
                i_row += steps;
                if (bad < 0 && any_nonfinite<T, NS>(y)) bad = i_row - 1;
            }
        };
        checkpoint(0);
        if (left < 0) write_powers();          // no row after z = 0
        int until = span;
        // ROW > 0: the saved rows of a launch whose save_every is ROW.  The block is ROW steps in straight line, the row work
        // and the counter: one basic block, nothing to pick, count or skip -- 10 instructions outside the steps and one taken
        // branch per row, where the run-time loop below has 23 and three at save_every = 10 (profiles/fixed_rows.log).
        // The same steps, the same row work, the same test points: no bit depends on which loop ran the rows.  What is rare
        // hangs off `until` as below; after the last row the tail, if any, is one block of the run-time loop.  The host picks
        // this instantiation for save_every == ROW only (launch_sweep_f64); any other stride takes the run-time loop here too.
        if constexpr (ROW > 0) {
            if (se == ROW && left > 0) {
                for (;;) {
#pragma unroll
                    for (int q = 0; q < ROW; ++q) rk4_step_reg(0);
                    row_work(ROW);
                    if (--until != 0) continue;                   // wave-uniform; the back-edge of every other row
                    left -= span;
                    exact_test((n_rows - left) * ROW);
                    if (left == 0) break;
                    until = span = span_of(left);
                }
                store_a_end_at(n_rows * ROW);  // A[-1]: the last saved row, not necessarily z_max (R8)
                write_powers();
                left = -1;
                m = tail;
                trips = m / PSA_ROW_TRIP;
                until = 1;
            }
        }
        if (m > 0) {
            for (;;) {
                if (m & 1) rk4_step_reg(0);
                if constexpr (PSA_ROW_TRIP == 4) {
                    if (m & 2) {
                        rk4_step_reg(0);
                        rk4_step_reg(0);
                    }
                }
                for (int q = trips; q > 0; --q) {
                    rk4_step_reg(0);
                    rk4_step_reg(0);
                    if constexpr (PSA_ROW_TRIP == 4) {
                        rk4_step_reg(0);
                        rk4_step_reg(0);
                    }
                }
                row_work(m);
                if (--until != 0) continue;                       // wave-uniform; the back-edge of every other row
                if (left > 0) left -= span;
                exact_test(left < 0 ? n_run : (n_rows - left) * se);
                if (left < 0) break;
                if (left > 0) {
                    until = span = span_of(left);
                    continue;
                }
                store_a_end_at(n_rows * se);   // A[-1]: the last saved row, not necessarily z_max (R8)
                write_powers();
                if (tail == 0) break;
                left = -1;
                m = tail;
                trips = m / PSA_ROW_TRIP;
                until = 1;
            }
        }
        A.first_bad[idx] = bad;
        return;
    }

    // ---- z-loop, event driven (trajectory, six waves, float32, LDS): the steps between two events (a saved row, a phase
    // re-seed, the end) run in a branch-free 2x-unrolled inner loop.  With one wave per SIMD (65 536 points fill the chip
    // exactly once) every taken branch is an exposed instruction refetch -- see DESIGN.md section 5.
    // Seeds fall on the ABSOLUTE grid i = 0, RESYNC, 2*RESYNC, ... whatever save_every is (the save_every == 1 loop above does
    // the same), so the computed trajectory does not depend on which rows are saved -- as upstream, where the stride only
    // selects rows (integrators.py:137-140): A[-1] at any stride equals the same row of the every-step run bit for bit.
    // FRAME has no phase factor to seed.  With a trajectory its F is seeded on the same grid, AFTER the steps that reach a
    // multiple of RESYNC and before the row that may be due there (F(step) is seeded, not carried, at the multiples);
    // without one there is no seed event at all and F is built where A[-1] is stored (store_a_end_at).
    int i = 0;
    int row = 0;
    checkpoint(0);
    int next_save = (n_rows > 0) ? se : 0x7fffffff;
    int next_seed = !FRAME ? 0 : ((TRAJ && n_run >= RESYNC) ? RESYNC : 0x7fffffff);
    while (i < n_run) {
        if constexpr (!FRAME) {
            if (i == next_seed) {          // wave-uniform: exact re-seed of the phase recurrence at z_i = i*h
                seed_phase(i);
                next_seed = (n_run - i > RESYNC) ? i + RESYNC : 0x7fffffff;   // no overflow near 2^31 steps
            }
        }
        int end = n_run < next_seed ? n_run : next_seed;
        end = end < next_save ? end : next_save;
        const int m = end - i;
        int j = 0;
        if constexpr (LDS) {
            for (; j < m; ++j) rk4_step_lds(i + j);
        } else {
            for (; j + 2 <= m; j += 2) {
                rk4_step(i + j);
                rk4_step(i + j + 1);
            }
            if (j < m) rk4_step(i + j);
        }
        i = end;
        if constexpr (FRAME && TRAJ) {
            if (i == next_seed) {          // wave-uniform: F(i) exactly
                frame_seed(i, Fc, Fs);
                next_seed = (n_run - i >= RESYNC) ? i + RESYNC : 0x7fffffff;
            }
        }
        if (i == next_save) {  // (i % save_every == 0), integrators.py:137 -- wave-uniform
            ++row;
            pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
            pm = (pe > pm || pe != pe) ? pe : pm;  // np.max propagates NaN
            if constexpr (WSUM) {
#pragma unroll
                for (int j = 0; j < NWS; ++j) {
                    const T pj = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
                    pwm[j] = (pj > pwm[j] || pj != pj) ? pj : pwm[j];
                }
            }
            if constexpr (CHECK == CHECK_BLOCK) {
                if (bad < 0 && any_nonfinite<T, NS>(y)) bad = i - 1;
            }
            exact_test(i);
            if constexpr (TRAJ) store_traj_row(row);
            if (row == n_rows) {  // A[-1]: the last saved row, not necessarily z_max (R8)
                store_a_end_at(i);
                next_save = 0x7fffffff;
            } else {
                next_save += se;
            }
        }
    }
    if constexpr (CHECK == CHECK_BLOCK) {  // covers the unsaved tail
        if (bad < 0 && n_run > 0 && any_nonfinite<T, NS>(y)) bad = n_run - 1;
    }
    if (n_run > i_chk) exact_test(n_run);   // the unsaved tail (REPLAY only; compiled out otherwise)
    write_summary();
}

// Does every live lane of this wave start MIRRORED?  A lane agrees when A2 == A1 and A4 == A3 as bit patterns (+0 and -0
// differ: their products differ in sign) and all eight components are finite (a NaN payload need not survive the same way
// in both loops).  One ballot over the active lanes: the answer is wave-uniform.
__device__ __forceinline__ bool wave_starts_mirrored(const double (&y)[8]) {
    bool same = true;
#pragma unroll
    for (int c = 0; c < 8; c += 4) {
        same = same && __builtin_bit_cast(long long, y[c]) == __builtin_bit_cast(long long, y[c + 2]) &&
               __builtin_bit_cast(long long, y[c + 1]) == __builtin_bit_cast(long long, y[c + 3]);
    }
    const bool objects = !same || any_nonfinite<double, 8>(y);
    return __builtin_amdgcn_ballot_w64(objects) == 0;
}

template <typename T, int NW, int CHECK, bool TRAJ, int BLOCK, bool LDS = false, bool LOSS = true, bool WSUM = false, int ROW = 0>
__global__ void __launch_bounds__(BLOCK) PSA_SWEEP_KERNEL_ATTR rk4_sweep_kernel(const SweepArgs<T> A) {
    static_assert(!WSUM || (!TRAJ && !LDS), "the per-wave summary exists for the register layout without trajectory");
    constexpr int NC = 2 * NW;
    const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= A.n_points) return;

    // -- per-point inputs: one coalesced load per array (512 B per wave instruction in f64)
    T y[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = A.a0[(long long)c * A.a0_ld + idx * A.a0_stride];
    // float64, 4 waves, register layout: a wave whose live lanes all start mirrored integrates waves 1 and 3 only.  The
    // branch is taken once, before the z-loop; the lanes past n_points have left and do not vote.
    if constexpr (sizeof(T) == 8 && NW == 4 && !LDS) {
        if (wave_starts_mirrored(y)) {
            // The mirrored body loads A1 and A3 again, through an index the compiler cannot see through: with y[0], y[1],
            // y[4], y[5] handed over instead, those four registers stay live into both branches, the general branch works on
            // copies of them and every instantiation needs 8 VGPRs more (206 instead of 198 in the headline one).
            long long idx_m = idx;
            asm volatile("" : "+v"(idx_m));
            T ym[NW];
#pragma unroll
            for (int c = 0; c < NW; ++c) ym[c] = A.a0[(long long)(c < 2 ? c : c + 2) * A.a0_ld + idx_m * A.a0_stride];
            sweep_point<T, NW, CHECK, TRAJ, BLOCK, LDS, LOSS, WSUM, true, ROW>(A, idx_m, ym);
            return;
        }
    }
    sweep_point<T, NW, CHECK, TRAJ, BLOCK, LDS, LOSS, WSUM, false, ROW>(A, idx, y);
}

// One lane per point.  LDS staging (an A/B variant: 5 * 2*NW * 64 * sizeof(T) bytes of LDS, 20 KB for f64 with 4 waves)
// is one 64-thread wave per workgroup with the loss links; the per-wave summary is register-only, without trajectory,
// in 256-thread workgroups.  A fixed row length (ROW, Pick::row) exists for the row-driven z-loop alone: float64, 4 waves,
// register layout, no trajectory.
template <typename T> struct OneLane {
    static long long lanes(long long n_points) { return n_points; }
    template <int NW, int CHECK, bool TRAJ, int BLOCK, bool LDS, bool LOSS, bool WSUM, int ROW = 0>
    static constexpr auto kernel() {
        if constexpr ((WSUM && (TRAJ || LDS || BLOCK != 256)) || (LDS && (BLOCK != 64 || !LOSS))) return nullptr;
        else if constexpr (ROW != 0 && (sizeof(T) != 8 || NW != 4 || TRAJ || LDS)) return nullptr;
        else return rk4_sweep_kernel<T, NW, CHECK, TRAJ, BLOCK, LDS, LOSS, WSUM, ROW>;
    }
};

// ---- the one launch path of every sweep kernel family (OneLane, SplitLanes, QuadLanes, PackedPoints) ------------
// The layout choice (launch_sweep_f64 / launch_sweep_f32) fills a Pick; launch_family turns its runtime values into
// template arguments once.  A family says how many lanes its launch takes and which instantiations exist: a
// combination that does not is never named, so the set of compiled kernels is exactly the families' own.
struct Pick {
    int n_waves, check, block;  // 4 | 6, CheckMode, 64 | 256
    bool traj, lds, lossless, wsum;
    int row;                    // 0, or the save_every the kernel is compiled for (PSA_FIXED_ROW; launch_sweep_f64 sets it)
};
constexpr int PSA_FIXED_ROW = 10;   // the stride of the headline, of every driver default and of the goldens

// What every layout shares, filled for one lane per point: the check mode, trajectory and per-wave summary (from the
// buffers), LDS staging and BLOCK64 (LDS staging is always 64 threads; BLOCK64 is rejected with the per-wave summary,
// so those launches get 256), and LOSSLESS -- the caller's promise that alpha == 0 for every point, which compiles the
// 8 loss links per RHS out -- for the register layout only.
template <typename T>
static Pick pick_one_lane(int n_waves, uint32_t flags, const SweepArgs<T> &a) {
    Pick p;
    p.n_waves = n_waves;
    p.check = check_mode(flags);
    p.traj = a.traj != nullptr;
    p.wsum = a.p_wave_end != nullptr;
    p.lds = (flags & PSA_OPT_LDS_STAGING) != 0;
    p.lossless = (flags & PSA_OPT_LOSSLESS) && !p.lds;
    p.block = (p.lds || (flags & PSA_OPT_BLOCK64)) ? 64 : 256;
    p.row = 0;
    return p;
}

template <typename Family, typename T>
static hipError_t launch_family(hipStream_t s, const Pick &p, const SweepArgs<T> &a) {
    if (a.n_points == 0) return hipSuccess;   // before the dispatch: an empty sweep succeeds whatever it names
    return with_int<4, 6>(p.n_waves, [&](auto nw) {
    return with_int<CHECK_NONE, CHECK_BLOCK, CHECK_EXACT>(p.check, [&](auto check) {
    return with_int<64, 256>(p.block, [&](auto blk) {
    return with_bool(p.traj, [&](auto traj) {
    return with_bool(p.lds, [&](auto lds) {
    return with_bool(p.lossless, [&](auto lossless) {
    return with_bool(p.wsum, [&](auto wsum) {
    return with_int<PSA_FIXED_ROW, 0>(p.row, [&](auto row) {
        constexpr auto k = Family::template kernel<nw, check, traj, blk, lds, !lossless, wsum, row>();
        if constexpr (std::is_null_pointer_v<std::remove_const_t<decltype(k)>>) {
            return hipErrorInvalidDeviceFunction;   // no such instantiation: the layout choice never picks one
        } else {
            return launch_lanes(reinterpret_cast<const void *>(k), Family::lanes(a.n_points), p.block, 0, a, s);
        }
    }); }); }); }); }); }); }); });
}

}  // namespace psa
