// psa_rk4_pairs_kernel.inc.h -- float64 RK4 sweep of the MULTI-CHANNEL model: two pumps and K = 1..16 signal/idler pairs,
// ONE LANE PER PAIR (gfx950).  Build-defined, like the 6-wave model it extends; K = 1 is the reference's
// system (yaman_model.py:123-186), K = 2 the 6-wave model of rk4_sweep_kernel.
//
//     waves [p1, p2, s_1, i_1, ..., s_K, i_K],  P_j = |A_j|^2,  S = sum_j P_j,  E_k(z) = 2*gamma*exp(i*dbeta_k*z)
//     dA_p1/dz = (-alpha/2 + i*gamma*(2S - P_p1)) A_p1 + i*conj(A_p2) * sum_k E_k A_sk A_ik        (p2: p1 <-> p2)
//     dA_sk/dz = (-alpha/2 + i*gamma*(2S - P_sk)) A_sk + i*conj(A_ik) * conj(E_k) A_p1 A_p2        (ik: sk <-> ik)
//
// The channels couple through pump depletion and SPM/XPM only: FWM products BETWEEN channels (signal-signal mixing) are not
// modelled.
//
// Layout: L lanes per sweep point, L the power of two >= K in {2, 4, 8, 16} (K = 1 runs with L = 2 and one dark lane; a lane
// never holds more than one pair, so K = 5 pays for 8 lanes).  Lane r = gid % L holds pair r AND ITS OWN COPY OF BOTH PUMPS:
// four complex amplitudes, the state of the 4-wave one-lane kernel, however many channels there are -- a one-lane kernel for
// K = 16 would keep ~270 doubles live.  Lanes r >= K are padding: a dark pair (zero amplitudes, dbeta = 0) that adds exact
// zeros to every sum and writes nothing.  L divides 16, so a point never straddles a DPP row and its L lanes enter and leave
// the kernel together.
//
// Per RHS evaluation a lane forms three values for the point's sums -- its pair's power P_s + P_i and the complex pair
// product E_k A_s A_i -- and the L lanes all-reduce these three doubles by a butterfly of DPP moves (quad_perm:[1,0,3,2],
// quad_perm:[2,3,0,1], row_half_mirror, row_mirror; two v_mov_b32_dpp and one add per double and level).  Everything else is
// the arithmetic of the 4-wave stage (yaman_stage) on the lane's own four amplitudes.
//
// The pump copies of a point stay BIT-IDENTICAL in all its lanes.  Each butterfly level adds a register value to the
// partner's register value; IEEE addition commutes, so the two lanes of a level hold equal bits afterwards, and by
// induction all L lanes hold the same three sums.  The pumps' arithmetic reads only these sums, the pumps themselves and
// per-point constants (gamma, alpha, h), through the same instruction stream in every lane: equal inputs, equal outputs.
// The per-lane quantities (the pair, its E_k) enter the pumps through the sums alone.  This holds under -ffp-contract=fast
// because every value handed to the butterfly is the RESULT of an explicit fma or of an add, never of a bare multiply:
// contraction fuses a multiply with the add that consumes it, and a level `v + partner(v)` whose v were an unrounded product
// on the own side and a rounded one on the partner's would break the symmetry.  With no multiply feeding a level there is
// nothing to fuse.  Lane 0 writes the pumps; the sidebands are written by their own lanes.
//
// No divergent control flow surrounds an exchange (DPP reads lanes that EXEC has disabled): the non-finite test is an
// all-reduce followed by a ballot, as in rk4_sweep_quad_kernel, and loads and stores are the only lane-dependent branches.
//
// The regrouped RK4 step, the phase recurrence with seeds on the absolute RESYNC grid, the event-driven z-loop, the save /
// NaN semantics and the replay that finds the exact first_bad_step are the shared ones of psa_rk4_carried.inc.h (see that
// file).  `bad` and the non-finite test's result are the same in the L lanes of a point, so no exchange runs with part of
// a point masked off.
//
// Saved rows (TRAJ): row 0 is z = 0, then one row per save, [row][wave][ld] (re, im) pairs like every other family.  Lane 0
// stores the two pumps, lane r < K its pair's waves 2 + 2r and 3 + 2r, a padding lane nothing: one 16-byte store per wave, so
// of a wave's 64 lanes 64/L write CONSECUTIVE points of one wave region.  The stores sit where the
// summary stores sit, outside every exchange.  Chains of spans are joined outside the kernel (psa_chain.hip).
//
// Out of scope: float32, LDS staging, RK45, a dedicated save_every == 1 loop.
#pragma once
#include "psa_launch.inc.h"
#include "psa_rk4_carried.inc.h"
#include "psa_rk4_prims.inc.h"

namespace psa {

// Sum of v over the L lanes of a point, the same bits in every one of them.  v must be the result of an fma or an add.
template <int L> __device__ __forceinline__ double pairs_allreduce(double v) {
    static_assert(L == 2 || L == 4 || L == 8 || L == 16, "L lanes per point: a power of two that divides a DPP row");
    v += quad_xchg<QUAD_PAIR>(v);
    if constexpr (L >= 4) v += quad_xchg<QUAD_OTHER>(v);
    if constexpr (L >= 8) v += quad_xchg<ROW_HALF_MIRROR>(v);
    if constexpr (L >= 16) v += quad_xchg<ROW_MIRROR>(v);
    return v;
}

// out = base + c * dA/dz of the lane's four waves a = [Re p1, Im p1, Re p2, Im p2, Re s, Im s, Re i, Im i] (stage
// coefficient c folded into g, tg, ha, E as in yaman_stage).  With one pair lit the sums are that pair's own values plus
// exact zeros, and the arithmetic is the pairwise form of yaman_stage<double, 4, true> (CROSS = false) operation for
// operation.  The RK4 sweep of rk4_sweep_kernel takes the crosswise form: the same triple products in another order, so
// the two kernels agree to rounding there, not bit for bit.
template <int L, bool LOSS>
__device__ __forceinline__ void pairs_stage(const double (&a)[8], const double (&base)[8], const double Er, const double Ei,
                                            const double g, const double tg, const double ha, double (&out)[8]) {
    double p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
    const double s = (p[0] + p[1]) + pairs_allreduce<L>(p[2] + p[3]);   // every wave of the point
    const double gs = tg * s;
    double gj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gj[j] = fma_(-g, p[j], gs);

    auto link = [&](const double gsig, const double v, const int c) -> double {
        if constexpr (LOSS) return fma_(gsig, v, fma_(ha, a[c], base[c]));
        else return fma_(gsig, v, base[c]);
    };
    const double x1 = a[0], y1 = a[1], x2 = a[2], y2 = a[3], xs = a[4], ys = a[5], xi = a[6], yi = a[7];
    const double q12r = fma_(x1, x2, -(y1 * y2)), q12i = fma_(x1, y2, y1 * x2);   // A_p1 A_p2
    const double qr = fma_(xs, xi, -(ys * yi)), qi = fma_(xs, yi, ys * xi);        // A_s A_i
    // sum_k E_k (A_s A_i)_k: drives both pumps
    const double Fpr = pairs_allreduce<L>(fma_(Er, qr, -(Ei * qi)));
    const double Fpi = pairs_allreduce<L>(fma_(Er, qi, Ei * qr));
    // conj(E_k) (A_p1 A_p2): drives this lane's signal and idler
    const double Fsr = fma_(Er, q12r, Ei * q12i);
    const double Fsi = fma_(Er, q12i, -(Ei * q12r));
    out[0] = fma_(y2, Fpr, fma_(-x2, Fpi, link(-gj[0], y1, 0)));
    out[1] = fma_(x2, Fpr, fma_(y2, Fpi, link(gj[0], x1, 1)));
    out[2] = fma_(y1, Fpr, fma_(-x1, Fpi, link(-gj[1], y2, 2)));
    out[3] = fma_(x1, Fpr, fma_(y1, Fpi, link(gj[1], x2, 3)));
    out[4] = fma_(yi, Fsr, fma_(-xi, Fsi, link(-gj[2], ys, 4)));
    out[5] = fma_(xi, Fsr, fma_(yi, Fsi, link(gj[2], xs, 5)));
    out[6] = fma_(ys, Fsr, fma_(-xs, Fsi, link(-gj[3], yi, 6)));
    out[7] = fma_(xs, Fsr, fma_(ys, Fsi, link(gj[3], xi, 7)));
}

template <int L, int CHECK, int BLOCK, bool LOSS, bool TRAJ>
__global__ void __launch_bounds__(BLOCK) rk4_sweep_pairs_kernel(const PairsArgs A) {
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long idx = gid / L;          // sweep point: its L lanes share one
    const int r = (int)(gid % L);           // = the pair this lane holds
    const long long N = A.n_points;
    if (idx >= N) return;                   // the L lanes of a point leave together
    const bool lit = r < A.n_pairs;         // padding lanes: a dark pair
    const int rr = lit ? r : 0;             // ... that reads pair 0's (in-bounds) entries and drops them

    double a[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = A.a0[(long long)c * A.a0_ld + idx * A.a0_stride];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double v = A.a0[(long long)(4 + 4 * rr + c) * A.a0_ld + idx * A.a0_stride];
        a[4 + c] = lit ? v : 0.0;
    }
    const double g = A.gamma[idx * A.gamma_stride];
    const double ha = -0.5 * A.alpha[idx * A.alpha_stride];
    const double db = A.dbeta[(long long)rr * N + idx];
    const double dbd = lit ? db : 0.0;
    const CarriedConsts K = carried_consts(g, ha, dbd, A.z_max, A.n_steps);
    const double e_amp = K.tg_d;
    double Er = e_amp, Ei = 0.0;

    double pm[4];                           // np.max of |A_j|^2 over saved rows (z = 0 is one): p1, p2, s, i
#pragma unroll
    for (int j = 0; j < 4; ++j) pm[j] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
    auto nonfinite_on = [&](const double (&v)[8]) -> bool {   // any component of the POINT non-finite
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) t = fma_(v[c], 0.0, t);
        t = pairs_allreduce<L>(t);
        return t != t;
    };

    // lane 0 writes the pumps (waves 0, 1), lane r < K its pair (waves 2 + 2r, 3 + 2r)
    auto store_a_end = [&]() {
        if (r == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) A.a_end[(long long)c * N + idx] = a[c];
#pragma unroll
            for (int j = 0; j < 2; ++j) A.p_wave_end[(long long)j * N + idx] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
        }
        if (lit) {
#pragma unroll
            for (int c = 0; c < 4; ++c) A.a_end[(long long)(4 + 4 * r + c) * N + idx] = a[4 + c];
#pragma unroll
            for (int j = 2; j < 4; ++j)
                A.p_wave_end[(long long)(2 * r + j) * N + idx] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
        }
    };
    // trajectory rows [row][wave][ld][2].  The wave a lane stores depends on the lane, so the (row, wave) base is not
    // wave-uniform as it is in the one-lane kernels: each lane keeps the 64-bit address of its first wave's pair in row 0
    // and steps it by whole rows; plain C++ stores, so the compiler sees the 16-byte store hazard itself.  The C-ABI keeps
    // ld * 16 below 2^32, the bound of every float64 row launch.
    using Pair = typename PairOf<double>::type;
    const long long LD = A.traj_ld;
    const long long row_pairs = (long long)(2 + 2 * A.n_pairs) * LD;
    Pair *const pump_row0 = reinterpret_cast<Pair *>(A.traj) + idx;                       // wave 0; wave 1 is LD further
    Pair *const pair_row0 = pump_row0 + (long long)(2 + 2 * rr) * LD;                     // wave 2 + 2r; 3 + 2r is LD further
    auto store_traj_row = [&](const int row) {
        if (r == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                __builtin_nontemporal_store(Pair{a[2 * j], a[2 * j + 1]}, pump_row0 + (long long)row * row_pairs + (long long)j * LD);
        }
        if (lit) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                __builtin_nontemporal_store(Pair{a[4 + 2 * j], a[5 + 2 * j]}, pair_row0 + (long long)row * row_pairs + (long long)j * LD);
        }
    };
    if constexpr (TRAJ) store_traj_row(0);
    if (A.n_steps / A.save_every == 0) store_a_end();   // no saved row after z = 0

    auto stage = [&](auto full, const double (&y)[8], const double (&base)[8], const double er, const double ei, double (&out)[8]) {
        if constexpr (decltype(full)::value) pairs_stage<L, LOSS>(y, base, er, ei, K.g_h, K.tg_h, K.ha_h, out);
        else pairs_stage<L, LOSS>(y, base, er, ei, K.g_d, K.tg_d, K.ha_d, out);
    };
    auto step_on = [&](double (&y)[8], double &er, double &ei) { carried_step<8>(y, er, ei, K.rc, K.rs, stage); };
    auto seed_on = [&](const int step, double &er, double &ei) { carried_seed(e_amp, dbd, K.hd, step, er, ei); };
    auto summarise = [&]() {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const double pw = fma_(a[2 * w], a[2 * w], a[2 * w + 1] * a[2 * w + 1]);
            pm[w] = (pw > pm[w] || pw != pw) ? pw : pm[w];   // np.max propagates NaN
        }
    };
    auto save_row = [&](const int row, const bool last) {
        if constexpr (TRAJ) store_traj_row(row);
        if (last) store_a_end();
    };
    const long long bad = carried_event_loop<CHECK, 2>(a, Er, Ei, A.n_steps, A.save_every, step_on, seed_on, nonfinite_on, summarise, save_row);
    if (r == 0) {
        A.p_wave_max[idx] = pm[0];
        A.p_wave_max[N + idx] = pm[1];
        A.first_bad[idx] = bad;
    }
    if (lit) {
        A.p_wave_max[(long long)(2 * r + 2) * N + idx] = pm[2];
        A.p_wave_max[(long long)(2 * r + 3) * N + idx] = pm[3];
    }
}

}  // namespace psa
