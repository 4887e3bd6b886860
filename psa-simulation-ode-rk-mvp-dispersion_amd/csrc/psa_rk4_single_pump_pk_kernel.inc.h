// psa_rk4_single_pump_pk_kernel.inc.h -- float32 RK4 sweep of the SINGLE-PUMP three-wave model [p, s, i] with TWO sweep points per
// lane (packed math), gfx950.  The equations are those of psa_rk4_single_pump_kernel.inc.h, the layout and the
// arithmetic those of rk4_sweep_pk_kernel (psa_rk4_pk_kernel.inc.h, psa_rk4_pk_body.inc.h):
//
//   layout   two points per lane as psa_rk4_pk_frame.inc.h lays them out (PkLane); a trajectory row is one 16-byte store per wave
//            of the model in a full wave.  N = 1 runs here too: there is no scalar float32 kernel for this model.
//   step     classic low-storage RK4 (y, y_stage, accumulator) on the UN-FUSED right-hand side: the fused regrouped stage of the
//            float64 kernel needs the stage coefficient folded into five constants per stage kind, which float32 rounds
//            (DESIGN.md 5.1).  E = 2*gamma*exp(i*dbeta*z) is carried by the half-step rotation and re-seeded every
//            Phase<float>::RESYNC steps on the absolute grid from a float64-reduced phase.  The sidebands read
//            conj(E)/2 * A_p^2 as conj(E) * (Re(A_p^2)/2 + i*m), m = x_p*y_p = Im(A_p^2)/2: the halving of Re(A_p^2) is exact, so
//            no second phase factor H = E/2 is carried.
//   state    compensated as in the packed 4-wave body: y = yb + dl, the increments collect in the small offset dl, which is
//            folded into yb with its rounding residue (Fast2Sum) where the phase is re-seeded.
//   loss     one register layout, with the loss links; PSA_OPT_LOSSLESS is accepted as a promise and runs this instantiation.
//
// Every packed operation is an explicit fma_, a bare product that feeds one, or an add of such results, so -ffp-contract=fast
// has nothing left to fuse and the output does not depend on the instantiation.  Per stage 51 packed instructions (|A_j|^2: 6,
// S and g_j: 6, A_s A_i: 4, E A_s A_i: 4, Re(A_p^2), its half and m: 3, conj(E) (..): 4, six 4-deep chains: 24); per step
// 4 * 51 + 30 (stage inputs and accumulator) + 18 (sum, offset, state) + 8 (two rotations) = 260 for two points, plus the
// per-step finite test of CHECK_EXACT (6) and 18 / RESYNC for the fold; as built, tools/single_pump_timing.py --static.
//
// Shared with the other packed kernels (psa_rk4_pk_frame.inc.h): the lane's points with load2 / store2, the finite test, the
// fold and the row maxima.  Still this kernel's own text, as in rk4_sweep_comb_pk_kernel and psa_rk4_pk_body.inc.h: the stores
// of a saved row, of the last one and of first_bad, and the event loop -- as shared functions they compile to other code
// (DESIGN.md 3.3d).  The body is not psa_rk4_pk_body.inc.h with a third stage: that body's VGPR counts depend on how it is
// included (see its head), and the three-wave model has neither a signal summary (p_end / p_max) nor a dbeta2 nor a mirrored
// form, so most of that text would sit behind switches.  Control flow is wave-uniform: branches on kernel arguments, loop
// counters, wave_full or nothing; lane-dependent branches hold loads and stores only.  Check modes as the packed kernel: per
// packed half, exact = a test after every step (no replay), block = at saved rows and after the last step.
//
// Out of scope: a lossless instantiation, a mirrored / lane-pair variant, a save_every == 1 fast loop, chains, RK45.
#pragma once
#include "psa_launch.inc.h"
#include "psa_rk4_pk_frame.inc.h"

namespace psa {

// k = dA/dz of a = [Re p, Im p, Re s, Im s, Re i, Im i] at the phase factor (Er, Ei) = 2*gamma*exp(i*dbeta*z)
__device__ __forceinline__ void single_pump_rhs_pk(const f32x2 (&a)[6], const f32x2 Er, const f32x2 Ei, const f32x2 g, const f32x2 tg,
                                                   const f32x2 ha, const f32x2 half, f32x2 (&k)[6]) {
    using V = f32x2;
    const V xp = a[0], yp = a[1], xs = a[2], ys = a[3], xi = a[4], yi = a[5];
    const V ypyp = yp * yp;   // shared by |A_p|^2 and Re A_p^2
    const V p[3] = {fma_(xp, xp, ypyp), fma_(xs, xs, ys * ys), fma_(xi, xi, yi * yi)};
    const V s = (p[0] + p[1]) + p[2];
    const V gs = tg * s;   // gamma * 2S
    V gj[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) gj[j] = fma_(-g, p[j], gs);   // gamma * (2S - P_j)
    const V qr = fma_(xs, xi, -(ys * yi)), qi = fma_(xs, yi, ys * xi);          // A_s A_i
    const V Fpr = fma_(Er, qr, -(Ei * qi)), Fpi = fma_(Er, qi, Ei * qr);        // E A_s A_i: drives the pump
    const V hp = half * fma_(xp, xp, -ypyp);                                   // Re A_p^2 / 2 (exact halving)
    const V m = yp * xp;                                                       // Im A_p^2 / 2
    const V Fsr = fma_(Er, hp, Ei * m), Fsi = fma_(Er, m, -(Ei * hp));          // conj(E)/2 A_p^2: drives signal and idler
    // pump: (ha + i g_p) A_p + i conj(A_p) Fp
    k[0] = fma_(yp, Fpr, fma_(-xp, Fpi, fma_(-gj[0], yp, ha * xp)));
    k[1] = fma_(xp, Fpr, fma_(yp, Fpi, fma_(gj[0], xp, ha * yp)));
    // signal: (ha + i g_s) A_s + i conj(A_i) Fs ;  idler: (ha + i g_i) A_i + i conj(A_s) Fs
    k[2] = fma_(yi, Fsr, fma_(-xi, Fsi, fma_(-gj[1], ys, ha * xs)));
    k[3] = fma_(xi, Fsr, fma_(yi, Fsi, fma_(gj[1], xs, ha * ys)));
    k[4] = fma_(ys, Fsr, fma_(-xs, Fsi, fma_(-gj[2], yi, ha * xi)));
    k[5] = fma_(xs, Fsr, fma_(ys, Fsi, fma_(gj[2], xi, ha * yi)));
}

template <int CHECK, bool TRAJ, int BLOCK>
__global__ void __launch_bounds__(BLOCK) rk4_sweep_single_pump_pk_kernel(const SinglePumpArgs<float> A) {
    using V = f32x2;
    constexpr int NW = 3, NC = 6;
    constexpr int RESYNC = Phase<float>::RESYNC;
    PkLane L;
    if (!L.init((long long)blockIdx.x * BLOCK + threadIdx.x, A.n_points)) return;
    const long long N = L.N;

    V y[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = L.load2(A.a0 + (long long)c * A.a0_ld, A.a0_stride);
    const V g = L.load2(A.gamma, A.gamma_stride);
    const V tg = g + g;
    const V ha = splat2(-0.5f) * L.load2(A.alpha, A.alpha_stride);
    double dbd[2];
    {
        const V d0 = L.load2(A.dbeta, 1);
        dbd[0] = (double)d0.x;
        dbd[1] = (double)d0.y;
    }
    const double hd = A.z_max / (double)A.n_steps;
    const V h = splat2((float)hd), hh = splat2((float)(0.5 * hd)), h6 = splat2((float)(hd / 6.0));
    const V two = splat2(2.0f), half = splat2(0.5f);

    V rc, rs, Er = tg, Ei = V{};
    auto seed = [&](const double z, V &outc, V &outs, const V amp) {
        float c0, s0, c1, s1;
        Phase<float>::eval(dbd[0] * z, c0, s0);
        Phase<float>::eval(dbd[1] * z, c1, s1);
        outc = amp * (V){c0, c1};
        outs = amp * (V){s0, s1};
    };
    seed(0.5 * hd, rc, rs, splat2(1.0f));   // half-step rotator exp(i*dbeta*h/2)
    auto seed_phase = [&](const int step) { seed((double)step * hd, Er, Ei, tg); };   // exact re-seed at z = step * h

    // Compensated state y = yb + dl (see psa_rk4_pk_body.inc.h): folded where the phase is re-seeded.
    V yb[NC], dl[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        yb[c] = y[c];
        dl[c] = V{};
    }
    auto fold = [&]() { pk_fold(y, [&](const int c) -> V & { return yb[c]; }, [&](const int c) -> V & { return dl[c]; }); };
    int bad[2] = {-1, -1};   // step indices are below 2^31: widened where they are stored
    V pm[NW];   // np.max of |A_j|^2 over saved rows (z = 0 is one)
#pragma unroll
    for (int j = 0; j < NW; ++j) pm[j] = pk_abs2(y[2 * j], y[2 * j + 1]);
    auto track = [&](const int step) { pk_track(y, step, bad); };
    auto store_a_end = [&]() {   // the last saved row and |A_j|^2 there
#pragma unroll
        for (int c = 0; c < NC; ++c) L.store2(A.a_end + (long long)c * N, y[c]);
#pragma unroll
        for (int j = 0; j < NW; ++j) L.store2(A.p_wave_end + (long long)j * N, pk_abs2(y[2 * j], y[2 * j + 1]));
    };

    const int se = A.save_every;
    const int n_rows = A.n_steps / se;
    const int n_run = (CHECK != CHECK_NONE) ? A.n_steps : n_rows * se;
    // trajectory rows [row][wave][ld][2]: the lane's two points are adjacent, so each wave of the model is ONE 16-B streaming
    // store per lane; the (row, wave) base stays in SGPRs and the lane adds a 32-bit byte offset (the C-ABI keeps ld * 8 B below
    // 2^31 for trajectory launches), as in rk4_sweep_pk_kernel
    const long long LD = A.traj_ld;
    const unsigned lane_off = (unsigned)L.idx * 16u;
    auto store_traj_row = [&](const int r) {
        const char *rowb = reinterpret_cast<const char *>(A.traj) + (long long)r * NW * LD * 8;
        if (L.wave_full) {
#pragma unroll
            for (int j = 0; j < NW; ++j)
                store_quad_nt(rowb + (long long)j * LD * 8, lane_off, (f32x4){y[2 * j].x, y[2 * j + 1].x, y[2 * j].y, y[2 * j + 1].y});
        } else {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const char *wb = rowb + (long long)j * LD * 8;
                store_pair_nt(wb, lane_off, (f32x2){y[2 * j].x, y[2 * j + 1].x});
                if (L.live1) store_pair_nt(wb, lane_off + 8u, (f32x2){y[2 * j].y, y[2 * j + 1].y});
            }
        }
    };
    if constexpr (TRAJ) store_traj_row(0);
    if (n_rows == 0) store_a_end();   // no saved row after z = 0

    auto rk4_step = [&](const int step_index) {  // low storage: y, y_stage, accumulator
        V k[NC], ys[NC], acc[NC];
        single_pump_rhs_pk(y, Er, Ei, g, tg, ha, half, k);
#pragma unroll
        for (int c = 0; c < NC; ++c) { acc[c] = k[c]; ys[c] = fma_(hh, k[c], y[c]); }
        rotate(Er, Ei, rc, rs);   // z + h/2
        single_pump_rhs_pk(ys, Er, Ei, g, tg, ha, half, k);
#pragma unroll
        for (int c = 0; c < NC; ++c) { acc[c] = fma_(two, k[c], acc[c]); ys[c] = fma_(hh, k[c], y[c]); }
        single_pump_rhs_pk(ys, Er, Ei, g, tg, ha, half, k);
#pragma unroll
        for (int c = 0; c < NC; ++c) { acc[c] = fma_(two, k[c], acc[c]); ys[c] = fma_(h, k[c], y[c]); }
        rotate(Er, Ei, rc, rs);   // z + h
        single_pump_rhs_pk(ys, Er, Ei, g, tg, ha, half, k);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#ifdef PSA_SINGLE_PUMP_F32_PLAIN   // A/B hook (tools/single_pump_timing.py --f32, the accuracy pass): plain y += inc
            y[c] = fma_(h6, acc[c] + k[c], y[c]);
#else
            dl[c] = fma_(h6, acc[c] + k[c], dl[c]);   // the increment joins the small offset ...
            y[c] = yb[c] + dl[c];                     // ... and y is the rounded state again (next stage input, saved rows)
#endif
        }
        if constexpr (CHECK == CHECK_EXACT) track(step_index);
    };

    // seeds (and the folds of the compensated state) on the absolute grid i = 0, RESYNC, ...: the trajectory does not depend on
    // save_every; rows, the last saved row and the tail steps that only the check runs are events of one loop
    int i = 0, row = 0;
    int next_save = (n_rows > 0) ? se : 0x7fffffff;
    int next_seed = 0;
    while (i < n_run) {
        if (i == next_seed) {
            seed_phase(i);
#ifndef PSA_SINGLE_PUMP_F32_PLAIN
            fold();
#endif
            next_seed = (n_run - i > RESYNC) ? i + RESYNC : 0x7fffffff;
        }
        int end = n_run < next_seed ? n_run : next_seed;
        end = end < next_save ? end : next_save;
        const int m = end - i;
        int j = 0;
        for (; j + 2 <= m; j += 2) {
            rk4_step(i + j);
            rk4_step(i + j + 1);
        }
        if (j < m) rk4_step(i + j);
        i = end;
        if (i == next_save) {
            ++row;
            pk_row_max(y, pm);
            if constexpr (CHECK == CHECK_BLOCK) track(i - 1);
            if constexpr (TRAJ) store_traj_row(row);
            if (row == n_rows) {
                store_a_end();
                next_save = 0x7fffffff;
            } else {
                next_save += se;
            }
        }
    }
    if constexpr (CHECK == CHECK_BLOCK) {
        if (n_run > 0) track(n_run - 1);
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) L.store2(A.p_wave_max + (long long)j * N, pm[j]);
    A.first_bad[L.pt[0]] = bad[0];
    if (L.live1) A.first_bad[L.pt[1]] = bad[1];
}

}  // namespace psa
