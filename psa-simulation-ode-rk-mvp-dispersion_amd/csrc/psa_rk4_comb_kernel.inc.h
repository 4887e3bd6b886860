// psa_rk4_comb_kernel.inc.h -- float64 RK4 sweep of the CW MULTI-LINE ("frequency comb") model (gfx950): M lines on a
// uniform frequency grid w_0 + m*dw and EVERY four-wave-mixing product among them that falls on the grid.  Build-defined,
// no reference counterpart.
//
//     lines m = 0..M-1 ascending in frequency, field A_m e^{i kappa_m z},  u_m(z) = exp(i kappa_m z),  B_m = A_m u_m
//     C_d = sum_n B_{n+d} conj(B_n)        both indices inside 0..M-1;  C_{-d} = conj(C_d),  C_0 = sum |B|^2
//     S_m = sum_l B_l C_{m-l}              = sum over every ordered triple k + l - n = m of B_k B_l conj(B_n)
//     dA_m/dz = -alpha/2 A_m + i gamma conj(u_m) S_m
//
// S_m holds SPM and XPM ((2 sum_j P_j - P_m) B_m), pump-pump, pump-signal and signal-signal mixing in one expression at
// O(M^2) per right-hand side; products outside the grid are dropped.  Only kappa_k + kappa_l - kappa_n - kappa_m ever acts,
// so kappa + a + b*m is the same system.  M = 3 is the single-pump model of psa_rk4_single_pump_kernel.inc.h with lines
// [0, 1, 2] = waves [s, p, i] and kappa_0 + kappa_2 - 2 kappa_1 = dbeta.
//
// Layout: one sweep point per lane, the whole z-loop in the kernel, the state in registers, M a template parameter
// (3..PSA_MAX_LINES).  Live per lane: y, the stage state, the accumulator t, u_m and the half-step rotators (2M doubles each),
// B and C inside a stage; kappa_m is NOT kept: it is read again from memory at every re-seed.  Every instantiation has
// ScratchSize 0; for that M >= 10 keeps its rotators in LDS and its stages apart (comb_rotators_in_lds).
//
// The method is that of psa_rk4_carried.inc.h with M carried factors instead of one:
//
//  * Step.  Classic RK4 regrouped as there: Y2 = y + d k1, Y3 = y + d k2, Y4 = y + h k3, D = t + d k4 with
//    t = Y2 + 2 Y3 + Y4 - 4 y (formed as the stages deliver), y += D/3; the stage coefficient is folded into gamma and alpha.
//  * Phase.  u_m is seeded exactly (one sincos of kappa_m * (i*h)) on the ABSOLUTE grid i = 0, RESYNC, 2*RESYNC, ... and
//    rotated by exp(i kappa_m h/2) twice per step in between, so the saved rows do not depend on save_every.
//  * Rows.  Row 0 is z = 0, a row follows every step with (i+1) % save_every == 0, a_end / p_wave_end are the last saved row,
//    p_wave_max the NaN-propagating maximum over the saved rows.  Without a check the loop ends at the last saved row.
//  * Check.  With CHECK the point is tested after EVERY step (2M + 3 instructions next to the step's 24 M^2 + 56 M): there is
//    no block mode and no replay, first_bad_step is always the exact index; the steps behind the last saved row run for it.
//  * Control flow is wave-uniform (kernel arguments and loop counters only; the test is two selects), and no lane reads another
//    lane's data: a failing lane cannot change its neighbours' bits.
//
// Per stage 6 M^2 + 10 M DP instructions (B: 4M, C_0: 2M, C_d: 2M(M-1), S: 4M^2 - 2M, conj(u) S: 4M, the links: 4M; 2M
// fewer without loss), per step 4 stages + 6M (t) + 2M (update) + 8M (two rotations) = 24 M^2 + 56 M.
//
// Out of scope: RK45, lane-group layouts, process-group sharding, non-uniform grids.  (Float32: psa_rk4_comb_pk_kernel.inc.h.)
#pragma once
#include "psa_launch.inc.h"
#include "psa_rk4_prims.inc.h"

namespace psa {

// out = base + c * dA/dz of a = [Re A_0, Im A_0, ..., Re A_{M-1}, Im A_{M-1}] with u = (ur, ui); c is folded into
// cg = c*gamma and cha = -c*alpha/2.
template <int M, bool LOSS>
__device__ __forceinline__ void comb_stage(const double (&a)[2 * M], const double (&base)[2 * M], const double (&ur)[M],
                                           const double (&ui)[M], const double cg, const double cha, double (&out)[2 * M]) {
    double br[M], bi[M];   // B_m = A_m u_m
#pragma unroll
    for (int m = 0; m < M; ++m) {
        br[m] = fma_(a[2 * m], ur[m], -(a[2 * m + 1] * ui[m]));
        bi[m] = fma_(a[2 * m], ui[m], a[2 * m + 1] * ur[m]);
    }
    double cr[M], ci[M];   // C_d, d >= 0; C_0 is real
    {
        double s = fma_(bi[0], bi[0], br[0] * br[0]);
#pragma unroll
        for (int n = 1; n < M; ++n) s = fma_(bi[n], bi[n], fma_(br[n], br[n], s));
        cr[0] = s;
        ci[0] = 0.0;
    }
#pragma unroll
    for (int d = 1; d < M; ++d) {
        double sr = fma_(bi[d], bi[0], br[d] * br[0]);
        double si = fma_(-br[d], bi[0], bi[d] * br[0]);
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
        double sr = br[m] * cr[0], si = bi[m] * cr[0];   // l = m: C_0
#pragma unroll
        for (int l = 0; l < M; ++l) {
            if (l == m) continue;
            const int d = m - l;
            const double c_r = cr[d < 0 ? -d : d];
            const double c_i = d < 0 ? -ci[-d] : ci[d];   // C_{-d} = conj(C_d)
            sr = fma_(-bi[l], c_i, fma_(br[l], c_r, sr));
            si = fma_(bi[l], c_r, fma_(br[l], c_i, si));
        }
        const double wr = fma_(ur[m], sr, ui[m] * si);      // conj(u_m) S_m
        const double wi = fma_(ur[m], si, -(ui[m] * sr));
        if constexpr (LOSS) {
            out[2 * m] = fma_(-cg, wi, fma_(cha, a[2 * m], base[2 * m]));
            out[2 * m + 1] = fma_(cg, wr, fma_(cha, a[2 * m + 1], base[2 * m + 1]));
        } else {
            out[2 * m] = fma_(-cg, wi, base[2 * m]);
            out[2 * m + 1] = fma_(cg, wr, base[2 * m + 1]);
        }
    }
}

struct CombConsts {
    double hd, g_d, ha_d, g_h, ha_h;   // h; gamma and -alpha/2 times d = h/2 (stages 1, 2, 4) and times h (stage 3)
};

// One RK4 step; u enters at z_step and leaves rotated to z_step + h.  rotator(m, c, s) delivers exp(i kappa_m h/2).
template <int M, bool LOSS, typename Rotator>
__device__ __forceinline__ void comb_step(double (&y)[2 * M], double (&ur)[M], double (&ui)[M], Rotator &rotator,
                                          const CombConsts &K) {
    constexpr int NC = 2 * M;
    double Y2[NC], Y3[NC], Y4[NC], t[NC], D[NC];
    auto rotate_all = [&]() {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            double c, s;
            rotator(m, c, s);
            rotate(ur[m], ui[m], c, s);
        }
    };
    // with the rotators in LDS the registers are nearly full: the scheduler then keeps each stage to itself, since work of the
    // next one hoisted across the boundary lengthens live ranges until the allocator spills
    auto fence = [&]() {
        if constexpr (comb_rotators_in_lds(M)) __builtin_amdgcn_sched_barrier(0);
    };
    comb_stage<M, LOSS>(y, y, ur, ui, K.g_d, K.ha_d, Y2);
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = fma_(-4.0, y[c], Y2[c]);
    rotate_all();   // z + h/2
    fence();
    comb_stage<M, LOSS>(Y2, y, ur, ui, K.g_d, K.ha_d, Y3);
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = fma_(2.0, Y3[c], t[c]);
    fence();
    comb_stage<M, LOSS>(Y3, y, ur, ui, K.g_h, K.ha_h, Y4);
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = t[c] + Y4[c];
    rotate_all();   // z + h
    fence();
    comb_stage<M, LOSS>(Y4, t, ur, ui, K.g_d, K.ha_d, D);
    const double third = 1.0 / 3.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = fma_(D[c], third, y[c]);
}

// The block size is the launch's (64 or 256 threads); both run this one instantiation.
template <int M, bool CHECK, bool LOSS>
__global__ void __launch_bounds__(256) rk4_sweep_comb_kernel(const CombArgs<double> A) {
    constexpr int NC = 2 * M;
    constexpr int RESYNC = Phase<double>::RESYNC;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long N = A.n_points;
    if (idx >= N) return;

    double a[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = A.a0[(long long)c * A.a0_ld + idx * A.a0_stride];
    const double g = A.gamma[idx * A.gamma_stride];
    const double ha = -0.5 * A.alpha[idx * A.alpha_stride];
    CombConsts K;
    K.hd = A.z_max / (double)A.n_steps;   // np.linspace step
    const double hh = 0.5 * K.hd;
    K.g_d = hh * g, K.ha_d = hh * ha, K.g_h = K.hd * g, K.ha_h = K.hd * ha;
    // the half-step rotators exp(i kappa_m h/2): in registers, or (ROT_LDS) in the lane's own LDS column [2M][blockDim], read
    // back twice per step; the compiler barrier keeps those reads inside the step instead of hoisting them into registers
    constexpr bool ROT_LDS = comb_rotators_in_lds(M);
    extern __shared__ double comb_lds[];
    double *const lds = comb_lds + threadIdx.x;
    const unsigned lds_ld = blockDim.x;
    double ur[M], ui[M], rc[ROT_LDS ? 1 : M], rs[ROT_LDS ? 1 : M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double c, s;
        Phase<double>::eval(A.kappa[(long long)m * N + idx] * hh, c, s);
        if constexpr (ROT_LDS) lds[(2 * m) * lds_ld] = c, lds[(2 * m + 1) * lds_ld] = s;
        else rc[m] = c, rs[m] = s;
        ur[m] = 1.0, ui[m] = 0.0;
    }
    auto rotator = [&](const int m, double &c, double &s) {
        if constexpr (ROT_LDS) c = lds[(2 * m) * lds_ld], s = lds[(2 * m + 1) * lds_ld];
        else c = rc[m], s = rs[m];
    };
    auto seed = [&](const int step) {   // exact u_m at z = step * h; kappa_m comes from memory, not from a register
        const double z = (double)step * K.hd;
#pragma unroll
        for (int m = 0; m < M; ++m) Phase<double>::eval(A.kappa[(long long)m * N + idx] * z, ur[m], ui[m]);
    };

    double pm[M];   // np.max of |A_m|^2 over saved rows (z = 0 is one)
#pragma unroll
    for (int m = 0; m < M; ++m) pm[m] = fma_(a[2 * m], a[2 * m], a[2 * m + 1] * a[2 * m + 1]);
    auto store_a_end = [&]() {   // the last saved row and |A_m|^2 there
#pragma unroll
        for (int c = 0; c < NC; ++c) A.a_end[(long long)c * N + idx] = a[c];
#pragma unroll
        for (int m = 0; m < M; ++m) A.p_wave_end[(long long)m * N + idx] = fma_(a[2 * m], a[2 * m], a[2 * m + 1] * a[2 * m + 1]);
    };
    // trajectory rows [row][line][ld][2]: a wave-uniform (row, line) base and the lane's 32-bit byte offset; the C-ABI keeps
    // ld * 16 below 2^32 for trajectory launches
    using Pair = typename PairOf<double>::type;
    const bool traj = A.traj != nullptr;
    const long long LD = A.traj_ld;
    const unsigned lane_off = (unsigned)idx * (unsigned)sizeof(Pair);
    auto store_traj_row = [&](const int r) {
        const char *rowb = reinterpret_cast<const char *>(A.traj) + (long long)r * M * LD * (long long)sizeof(Pair);
#pragma unroll
        for (int m = 0; m < M; ++m)
            store_pair_nt(rowb + (long long)m * LD * (long long)sizeof(Pair), lane_off, Pair{a[2 * m], a[2 * m + 1]});
    };
    if (traj) store_traj_row(0);

    const int se = A.save_every;
    const int n_rows = A.n_steps / se;                      // saved rows after z = 0
    const int n_run = CHECK ? A.n_steps : n_rows * se;      // the tail only matters for the check
    if (n_rows == 0) store_a_end();                         // no saved row after z = 0
    long long bad = -1;
    int i = 0, row = 0;
    int next_save = (n_rows > 0) ? se : 0x7fffffff;
    while (i < n_run) {
        const int phase = i % RESYNC;
        if (phase == 0) seed(i);
        const int to_seed = RESYNC - phase;
        int end = (n_run - i > to_seed) ? i + to_seed : n_run;   // no overflow near 2^31 steps
        end = end < next_save ? end : next_save;
#pragma nounroll
        for (; i < end; ++i) {
            if constexpr (ROT_LDS) asm volatile("" ::: "memory");
            comb_step<M, LOSS>(a, ur, ui, rotator, K);
            if constexpr (CHECK) {   // two selects, no branch: the test runs in every lane after every step
                const long long hit = any_nonfinite<double, NC>(a) ? (long long)i : -1;
                bad = bad < 0 ? hit : bad;
            }
        }
        if (i == next_save) {
            ++row;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double pw = fma_(a[2 * m], a[2 * m], a[2 * m + 1] * a[2 * m + 1]);
                pm[m] = (pw > pm[m] || pw != pw) ? pw : pm[m];   // np.max propagates NaN
            }
            if (traj) store_traj_row(row);
            const bool last = row == n_rows;   // the last saved row, not necessarily z_max
            if (last) store_a_end();
            next_save = last ? 0x7fffffff : next_save + se;
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) A.p_wave_max[(long long)m * N + idx] = pm[m];
    A.first_bad[idx] = bad;
}

}  // namespace psa
