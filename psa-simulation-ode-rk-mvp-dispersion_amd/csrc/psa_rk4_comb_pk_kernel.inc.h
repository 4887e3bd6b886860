// psa_rk4_comb_pk_kernel.inc.h -- float32 RK4 sweep of the CW MULTI-LINE ("frequency comb") model with TWO sweep points per
// lane (packed math), gfx950.  The equations and the discretisation are those of psa_rk4_comb_kernel.inc.h, the
// layout and the arithmetic those of psa_rk4_single_pump_pk_kernel.inc.h; DESIGN.md 3.3f.
//
//   layout   two points per lane as psa_rk4_pk_frame.inc.h lays them out (PkLane); a trajectory row is one 16-byte store per line
//            in a full wave.  N = 1 runs here too: there is no scalar float32 kernel for this model.
//   step     classic low-storage RK4 (y, y_stage, accumulator) on the UN-FUSED right-hand side k = dA/dz: the stage
//            coefficient is an operand of the stage-input FMA and is not folded into gamma and alpha, which float32 would
//            round.  u_m = exp(i kappa_m z) is carried by two half-step rotations per step and re-seeded every
//            COMB_PK_RESYNC steps on the absolute grid from a float64-reduced phase; kappa_m is read again from memory there.
//            Once per step |u_m| is brought back to one (a Newton step): what is carried must not keep a modulus offset.
//   state    compensated: y = yb + dl, the increments collect in the small offset dl, which is folded into yb (pk_fold, through
//            the accessors that know where a component lives) where the phases are re-seeded.
//   loss     one register layout, with the loss links; PSA_OPT_LOSSLESS is accepted as a promise and runs this instantiation.
//   check    CHECK tests every half after every step (no block mode, no replay): first_bad_step is exact per point.
//
// Every packed operation is an explicit fma_, a bare product that feeds one, or an add of such results, so -ffp-contract=fast
// has nothing left to fuse and a point's result does not depend on the instantiation, the block size, N or its half.  Per stage
// 6 M^2 + 10 M packed instructions (B: 4M, C_0: 2M, C_d: 2M(M-1), S: 4M^2 - 2M, conj(u) S: 4M, k with its loss link: 4M); per
// step 4 stages + 10M (stage inputs and accumulator) + 6M (sum, offset, state) + 8M (two rotations) + 5M (|u| = 1) = 24 M^2 +
// 69 M for two points, plus 2M for the test of CHECK and 6M / COMB_PK_RESYNC for the fold; as built, tools/comb_timing.py --f32 --static.
//
// No instantiation uses scratch memory.  What is touched once per step lives, from the M that needs it, in the lane's own LDS
// column (comb_pk_lds_vectors): the half-step rotators, then dl, then yb; sched_barrier fences keep the stages apart there.
// Control flow is wave-uniform: branches on kernel arguments, loop counters, wave_full or nothing; lane-dependent branches hold
// loads and stores only, and no lane reads another lane's data.
//
// From psa_rk4_pk_frame.inc.h: the lane's points with load2 / store2 / pin_points, the finite test, the fold, |A|^2.  This
// kernel's own, as in the single-pump kernel: the row maxima, the stores of a row, of the last one and of first_bad, and the
// event loop (DESIGN.md 3.3d says what each of them compiled to as a shared function).
//
// Out of scope: a lossless instantiation, a scalar (one point per lane) kernel, chains, RK45, lane-group layouts.
#pragma once
#include "psa_launch.inc.h"
#include "psa_rk4_pk_frame.inc.h"

namespace psa {

// steps between two exact seeds of u_m (and two folds of the state)
#ifndef PSA_COMB_F32_RESYNC     // A/B hook (tools/comb_timing.py --f32)
#define PSA_COMB_F32_RESYNC Phase<float>::RESYNC
#endif
constexpr int COMB_PK_RESYNC = PSA_COMB_F32_RESYNC;

// k = dA/dz of a = [Re A_0, Im A_0, ..., Re A_{M-1}, Im A_{M-1}] at u = (ur, ui); ha = -alpha/2.  Line m's (Re k_m, Im k_m) goes
// to emit(m, ., .) as soon as it exists; a[2m] and a[2m + 1] are not read after it, so emit may overwrite them.
template <int M, typename Emit>
__device__ __forceinline__ void comb_rhs_pk(const f32x2 (&a)[2 * M], const f32x2 (&ur)[M], const f32x2 (&ui)[M], const f32x2 g,
                                            const f32x2 ha, Emit &&emit) {
    using V = f32x2;
    V br[M], bi[M];   // B_m = A_m u_m
#pragma unroll
    for (int m = 0; m < M; ++m) {
        br[m] = fma_(a[2 * m], ur[m], -(a[2 * m + 1] * ui[m]));
        bi[m] = fma_(a[2 * m], ui[m], a[2 * m + 1] * ur[m]);
    }
    V cr[M], ci[M];   // C_d, d >= 0; C_0 is real
    {
        V s = fma_(bi[0], bi[0], br[0] * br[0]);
#pragma unroll
        for (int n = 1; n < M; ++n) s = fma_(bi[n], bi[n], fma_(br[n], br[n], s));
        cr[0] = s;
        ci[0] = V{};
    }
#pragma unroll
    for (int d = 1; d < M; ++d) {
        V sr = fma_(bi[d], bi[0], br[d] * br[0]);
        V si = fma_(-br[d], bi[0], bi[d] * br[0]);
#pragma unroll
        for (int n = 1; n + d < M; ++n) {
            sr = fma_(bi[n + d], bi[n], fma_(br[n + d], br[n], sr));
            si = fma_(-br[n + d], bi[n], fma_(bi[n + d], br[n], si));
        }
        cr[d] = sr;
        ci[d] = si;
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        V sr = br[m] * cr[0], si = bi[m] * cr[0];   // l = m: C_0
#pragma unroll
        for (int l = 0; l < M; ++l) {
            if (l == m) continue;
            const int d = m - l;
            const V c_r = cr[d < 0 ? -d : d];
            const V c_i = d < 0 ? -ci[-d] : ci[d];   // C_{-d} = conj(C_d)
            sr = fma_(-bi[l], c_i, fma_(br[l], c_r, sr));
            si = fma_(bi[l], c_r, fma_(br[l], c_i, si));
        }
        const V wr = fma_(ur[m], sr, ui[m] * si);      // conj(u_m) S_m
        const V wi = fma_(ur[m], si, -(ui[m] * sr));
        emit(m, fma_(-g, wi, ha * a[2 * m]), fma_(g, wr, ha * a[2 * m + 1]));
    }
}

// The block size is the launch's (64 or 256 threads); both run this one instantiation.
template <int M, bool CHECK>
__global__ void __launch_bounds__(256) rk4_sweep_comb_pk_kernel(const CombArgs<float> A) {
    using V = f32x2;
    constexpr int NC = 2 * M;
    constexpr int RESYNC = COMB_PK_RESYNC;
    PkLane L;   // pin_points() is called where the z-loop loads or stores per point
    if (!L.init((long long)blockIdx.x * blockDim.x + threadIdx.x, A.n_points)) return;
    const long long N = L.N;

    V y[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = L.load2(A.a0 + (long long)c * A.a0_ld, A.a0_stride);
    const V g = L.load2(A.gamma, A.gamma_stride);
    const V ha = splat2(-0.5f) * L.load2(A.alpha, A.alpha_stride);
    const double hd = A.z_max / (double)A.n_steps;   // np.linspace step
    const V h = splat2((float)hd), hh = splat2((float)(0.5 * hd)), h6 = splat2((float)(hd / 6.0));
    const V two = splat2(2.0f);

    // the lane's own LDS column [vector][2M][blockDim]; the compiler barrier at the head of a step keeps the reads inside it
    constexpr int LDSV = comb_pk_lds_vectors(M);
    constexpr bool ROT_LDS = LDSV >= 1, DL_LDS = LDSV >= 2, YB_LDS = LDSV >= 3;
    extern __shared__ f32x2 comb_pk_lds[];
    V *const lds = comb_pk_lds + threadIdx.x;
    const unsigned lds_ld = blockDim.x;
    auto lds_at = [&](const int vec, const int c) -> V & { return lds[(unsigned)(vec * NC + c) * lds_ld]; };

    auto eval2 = [&](const int m, const double z, V &c, V &s) {   // exp(i kappa_m z) of both halves; kappa_m from memory
        const V kap = L.load2(A.kappa + (long long)m * N, 1);
        float c0, s0, c1, s1;
        Phase<float>::eval((double)kap.x * z, c0, s0);
        Phase<float>::eval((double)kap.y * z, c1, s1);
        c = (V){c0, c1};
        s = (V){s0, s1};
    };
    V ur[M], ui[M], rc[ROT_LDS ? 1 : M], rs[ROT_LDS ? 1 : M];
#pragma unroll
    for (int m = 0; m < M; ++m) {   // the half-step rotators exp(i kappa_m h/2)
        V c, s;
        eval2(m, 0.5 * hd, c, s);
        if constexpr (ROT_LDS) lds_at(0, 2 * m) = c, lds_at(0, 2 * m + 1) = s;
        else rc[m] = c, rs[m] = s;
        ur[m] = splat2(1.0f), ui[m] = V{};
    }
    auto rotate_all = [&]() {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            if constexpr (ROT_LDS) rotate(ur[m], ui[m], lds_at(0, 2 * m), lds_at(0, 2 * m + 1));
            else rotate(ur[m], ui[m], rc[m], rs[m]);
        }
    };
    // One Newton step towards |u_m| = 1, u (3 - |u|^2) / 2, once per RK4 step.  The rounded rotator and the roundings of the
    // rotations leave |u_m| a few 1e-8 off one, and what is carried keeps that offset until the next seed: the self- and
    // cross-phase terms, |u|^2-fold products of the pump lines, then turn a_end at a rate that stays put for the rest of the seed
    // interval.  Without this step (-DPSA_COMB_F32_NORENORM) a_end sits 7.5x..16x off the compensated float32 statement from
    // M = 4 on, in proportion to the seed interval (profiles/comb_f32_timing.log); renormalised every step the offset is one rounding, as that of a fresh cos / sin pair.
    auto renormalise = [&]() {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const V f = fma_(splat2(-0.5f), fma_(ur[m], ur[m], ui[m] * ui[m]), splat2(1.5f));
            ur[m] = ur[m] * f;
            ui[m] = ui[m] * f;
        }
    };
    auto seed = [&](const int step) {   // exact u_m at z = step * h
        L.pin_points();
        const double z = (double)step * hd;
#pragma unroll
        for (int m = 0; m < M; ++m) eval2(m, z, ur[m], ui[m]);
    };

    // Compensated state y = yb + dl (see psa_rk4_pk_body.inc.h): folded where the phases are re-seeded.
    V yb[YB_LDS ? 1 : NC], dl[DL_LDS ? 1 : NC];
    auto yb_at = [&](const int c) -> V & { if constexpr (YB_LDS) return lds_at(2, c); else return yb[c]; };
    auto dl_at = [&](const int c) -> V & { if constexpr (DL_LDS) return lds_at(1, c); else return dl[c]; };
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        yb_at(c) = y[c];
        dl_at(c) = V{};
    }
    auto fold = [&]() { pk_fold(y, yb_at, dl_at); };
    int bad[2] = {-1, -1};   // step indices are below 2^31: widened where they are stored
    V pm[M];   // np.max of |A_m|^2 over saved rows (z = 0 is one)
#pragma unroll
    for (int m = 0; m < M; ++m) pm[m] = pk_abs2(y[2 * m], y[2 * m + 1]);
    auto track = [&](const int step) { pk_track(y, step, bad); };
    auto store_a_end = [&]() {   // the last saved row and |A_m|^2 there
        L.pin_points();
#pragma unroll
        for (int c = 0; c < NC; ++c) L.store2(A.a_end + (long long)c * N, y[c]);
#pragma unroll
        for (int m = 0; m < M; ++m) L.store2(A.p_wave_end + (long long)m * N, pk_abs2(y[2 * m], y[2 * m + 1]));
    };

    const int se = A.save_every;
    const int n_rows = A.n_steps / se;                      // saved rows after z = 0
    const int n_run = CHECK ? A.n_steps : n_rows * se;      // the tail only matters for the check
    // trajectory rows [row][line][ld][2]: the lane's two points are adjacent, so each line is ONE 16-B streaming store per lane;
    // the (row, line) base stays in SGPRs and the lane adds a 32-bit byte offset (the C-ABI keeps ld * 8 B below 2^31 for
    // trajectory launches), as in rk4_sweep_pk_kernel
    const bool traj = A.traj != nullptr;
    const long long LD = A.traj_ld;
    const unsigned lane_off = (unsigned)L.idx * 16u;
    auto store_traj_row = [&](const int r) {
        const char *rowb = reinterpret_cast<const char *>(A.traj) + (long long)r * M * LD * 8;
        if (L.wave_full) {
#pragma unroll
            for (int m = 0; m < M; ++m)
                store_quad_nt(rowb + (long long)m * LD * 8, lane_off, (f32x4){y[2 * m].x, y[2 * m + 1].x, y[2 * m].y, y[2 * m + 1].y});
        } else {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const char *wb = rowb + (long long)m * LD * 8;
                store_pair_nt(wb, lane_off, (f32x2){y[2 * m].x, y[2 * m + 1].x});
                if (L.live1) store_pair_nt(wb, lane_off + 8u, (f32x2){y[2 * m].y, y[2 * m + 1].y});
            }
        }
    };
    if (traj) store_traj_row(0);
    if (n_rows == 0) store_a_end();   // no saved row after z = 0

    // with part of the state in LDS the registers are nearly full: the scheduler then keeps each stage to itself, since work of
    // the next one hoisted across the boundary lengthens live ranges until the allocator spills
    auto fence = [&]() {
        if constexpr (LDSV > 0) __builtin_amdgcn_sched_barrier(0);
    };
    auto rk4_step = [&](const int step_index) {  // low storage: y, y_stage, accumulator
        if constexpr (LDSV > 0) asm volatile("" ::: "memory");
        V ys[NC], acc[NC];
        comb_rhs_pk<M>(y, ur, ui, g, ha, [&](const int m, const V kr, const V ki) {
            acc[2 * m] = kr, acc[2 * m + 1] = ki;
            ys[2 * m] = fma_(hh, kr, y[2 * m]), ys[2 * m + 1] = fma_(hh, ki, y[2 * m + 1]);
        });
        rotate_all();   // z + h/2
        fence();
        comb_rhs_pk<M>(ys, ur, ui, g, ha, [&](const int m, const V kr, const V ki) {
            acc[2 * m] = fma_(two, kr, acc[2 * m]), acc[2 * m + 1] = fma_(two, ki, acc[2 * m + 1]);
            ys[2 * m] = fma_(hh, kr, y[2 * m]), ys[2 * m + 1] = fma_(hh, ki, y[2 * m + 1]);
        });
        fence();
        comb_rhs_pk<M>(ys, ur, ui, g, ha, [&](const int m, const V kr, const V ki) {
            acc[2 * m] = fma_(two, kr, acc[2 * m]), acc[2 * m + 1] = fma_(two, ki, acc[2 * m + 1]);
            ys[2 * m] = fma_(h, kr, y[2 * m]), ys[2 * m + 1] = fma_(h, ki, y[2 * m + 1]);
        });
        rotate_all();   // z + h
#ifndef PSA_COMB_F32_NORENORM   // A/B hook (tools/comb_timing.py --f32, the accuracy pass): u_m carried as it is between two seeds
        renormalise();
#endif
        fence();
        auto update = [&](const int c, const V kc) {
#ifdef PSA_COMB_F32_PLAIN   // A/B hook (tools/comb_timing.py --f32, the accuracy pass): plain y += inc
            y[c] = fma_(h6, acc[c] + kc, y[c]);
#else
            const V d = fma_(h6, acc[c] + kc, dl_at(c));   // the increment joins the small offset ...
            dl_at(c) = d;
            y[c] = yb_at(c) + d;                           // ... and y is the rounded state again (next stage input, saved rows)
#endif
        };
        // the last stage reads all of ys before y changes: B is formed first, the loss link reads ys, and acc is its own array
        comb_rhs_pk<M>(ys, ur, ui, g, ha, [&](const int m, const V kr, const V ki) {
            update(2 * m, kr);
            update(2 * m + 1, ki);
        });
        fence();
        if constexpr (CHECK) track(step_index);
    };

    // seeds (and the folds of the compensated state) on the absolute grid i = 0, RESYNC, ...: the trajectory does not depend on
    // save_every; rows, the last saved row and the tail steps that only the check runs are events of one loop
    int i = 0, row = 0;
    int next_save = (n_rows > 0) ? se : 0x7fffffff;
    int next_seed = 0;
    while (i < n_run) {
        if (i == next_seed) {
            seed(i);
#ifndef PSA_COMB_F32_PLAIN
            fold();
#endif
            next_seed = (n_run - i > RESYNC) ? i + RESYNC : 0x7fffffff;   // no overflow near 2^31 steps
        }
        int end = n_run < next_seed ? n_run : next_seed;
        end = end < next_save ? end : next_save;
#pragma nounroll
        for (; i < end; ++i) rk4_step(i);
        if (i == next_save) {
            ++row;
#pragma unroll
            for (int m = 0; m < M; ++m) {   // pk_row_max(y, pm) in its place moves one instruction of the unchecked M = 10 kernel
                const V pw = pk_abs2(y[2 * m], y[2 * m + 1]);
                pm[m].x = (pw.x > pm[m].x || pw.x != pw.x) ? pw.x : pm[m].x;   // np.max propagates NaN
                pm[m].y = (pw.y > pm[m].y || pw.y != pw.y) ? pw.y : pm[m].y;
            }
            if (traj) store_traj_row(row);
            if (row == n_rows) {   // the last saved row, not necessarily z_max
                store_a_end();
                next_save = 0x7fffffff;
            } else {
                next_save += se;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) L.store2(A.p_wave_max + (long long)m * N, pm[m]);
    A.first_bad[L.pt[0]] = bad[0];
    if (L.live1) A.first_bad[L.pt[1]] = bad[1];
}

}  // namespace psa
