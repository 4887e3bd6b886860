// psa_rk4_pk_kernel.inc.h -- float32 sweep with TWO sweep points per lane (packed math), gfx950.
//
// Why: on this chip a float32 VALU instruction without packing sustains the same one-per-4-cycles issue rate as float64
// (tools/sp_peak.hip: v_fma_f32 tops out at 0.239 wave-instructions per clock per SIMD = 75 TFLOP/s at ANY occupancy), so a
// one-point-per-lane float32 kernel runs no faster than the float64 one.  Packing points (2i, 2i+1) into the two halves of a
// 64-bit register pair turns every instruction of the step into v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: the same
// instruction count advances twice the points (129.5 TFLOP/s measured with one wave per SIMD -- the shape of BASELINE
// config 4's per-GPU shard -- and 140-147 with four or more).  Same algorithm and arithmetic as the scalar float32 kernel
// (classic low-storage RK4 on the un-fused RHS with a compensated state update, phase factor re-seeded from a
// float64-reduced sincos every 16 steps), so the two agree to rounding.
//
// Of psa_rk4_pk_frame.inc.h this kernel and its body use the finite test, the fold, splat2 and the f32x2_u type: with the lane
// record (PkLane) or its load2 / store2 in place of the spelled-out prologue and lambdas, 24 of the unit's instantiations compile
// to other code (store2 as a method: 2 VGPRs more in every one), and this unit's device code is held to the text it had before
// the frame existed.
#pragma once
#include "psa_rk4_kernel.inc.h"
#include "psa_rk4_pk_frame.inc.h"

namespace psa {

// Does every live lane of this wave start MIRRORED in both of its points?  As wave_starts_mirrored: A2 == A1 and A4 == A3
// as bit patterns -- one 64-bit compare per packed pair, so both halves must agree, +0 and -0 differ -- and all eight
// components of both halves finite.  One ballot over the active lanes: the answer is wave-uniform.
__device__ __forceinline__ bool wave_starts_mirrored_pk(const f32x2 (&y)[8]) {
    bool same = true;
    f32x2 t = f32x2{};
#pragma unroll
    for (int c = 0; c < 8; c += 4) {
        same = same && __builtin_bit_cast(long long, y[c]) == __builtin_bit_cast(long long, y[c + 2]) &&
               __builtin_bit_cast(long long, y[c + 1]) == __builtin_bit_cast(long long, y[c + 3]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) t = fma_(y[c], f32x2{}, t);   // NaN exactly for a non-finite component, per half
    const bool objects = !same || t.x != t.x || t.y != t.y;
    return __builtin_amdgcn_ballot_w64(objects) == 0;
}

// WSUM: the per-wave summary (see rk4_sweep_kernel), both packed points at once.
//
// The per-lane body is psa_rk4_pk_body.inc.h.  4 waves: a wave whose live lanes all start mirrored IN BOTH packed points runs
// it with MIRROR = true -- waves 1 and 3 only, see rk4_sweep_kernel.  One branch before the z-loop; the lanes past n_points
// have left and do not vote, and the odd-tail lane's slot 1 is its slot 0 again.
template <int NW, int CHECK, bool TRAJ, int BLOCK, bool WSUM = false>
__global__ void __launch_bounds__(BLOCK) rk4_sweep_pk_kernel(const SweepArgs<float> A) {
    static_assert(!WSUM || !TRAJ, "the per-wave summary exists for launches without trajectory");
    using V = f32x2;
    constexpr int NC = 2 * NW;
    constexpr int NP = (NW - 2) / 2;
    constexpr int RESYNC = Phase<float>::RESYNC;
    const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long N = A.n_points;
    const long long pt[2] = {2 * idx, (2 * idx + 1 < N) ? 2 * idx + 1 : 2 * idx};  // odd tail: slot 1 mirrors slot 0
    if (pt[0] >= N) return;
    const bool live1 = 2 * idx + 1 < N;  // slot 1 holds a real point (else computed but never stored)

    // wave-uniform: every lane of this wave holds two real points -> 8-B loads / stores of the adjacent pair, 16-B trajectory
    // stores; the (at most one) wave with the odd tail or past-the-end lanes takes the element-wise path
    const bool wave_full = __builtin_amdgcn_readfirstlane((int)(2 * (idx | 63) + 1 < N)) != 0;
    auto load2 = [&](const float *base, const int stride) -> V {   // base[pt0 * stride], base[pt1 * stride]
        if (stride == 0) return splat2(base[0]);
        if (wave_full) return *reinterpret_cast<const f32x2_u *>(base + pt[0]);
        return (V){base[pt[0]], base[pt[1]]};
    };

    V y[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = load2(A.a0 + (long long)c * A.a0_ld, A.a0_stride);
    if constexpr (NW == 4) {
        if (wave_starts_mirrored_pk(y)) {
            // The mirrored body loads A1 and A3 again, through an index the compiler cannot see through, so that no a0 register
            // stays live into both branches (see rk4_sweep_kernel) -- an index taken from pt[0], which the general branch keeps
            // anyway, so that idx does not stay live up to the branch either: the general instantiations keep their VGPR counts.
            long long idx_m = pt[0];
            asm volatile("" : "+v"(idx_m));
            idx_m >>= 1;
            {
                constexpr bool MIRROR = true;
                const long long idx = idx_m;
                const long long pt[2] = {2 * idx, (2 * idx + 1 < N) ? 2 * idx + 1 : 2 * idx};
                const bool live1 = 2 * idx + 1 < N;
                auto load2 = [&](const float *base, const int stride) -> V {
                    if (stride == 0) return splat2(base[0]);
                    if (wave_full) return *reinterpret_cast<const f32x2_u *>(base + pt[0]);
                    return (V){base[pt[0]], base[pt[1]]};
                };
                V y[NW];
#pragma unroll
                for (int c = 0; c < NW; ++c) y[c] = load2(A.a0 + (long long)(c < 2 ? c : c + 2) * A.a0_ld, A.a0_stride);
#include "psa_rk4_pk_body.inc.h"
            }
            return;
        }
    }
    {
        constexpr bool MIRROR = false;
#include "psa_rk4_pk_body.inc.h"
    }
}

// Two float32 points per lane: register layout with the loss links only (no lossless form); the per-wave summary
// without trajectory, in 256-thread workgroups.
struct PackedPoints {
    static long long lanes(long long n_points) { return packed_lanes(n_points); }
    template <int NW, int CHECK, bool TRAJ, int BLOCK, bool LDS, bool LOSS, bool WSUM, int ROW = 0>
    static constexpr auto kernel() {
        if constexpr (ROW != 0 || LDS || !LOSS || (WSUM && (TRAJ || BLOCK != 256))) return nullptr;
        else return rk4_sweep_pk_kernel<NW, CHECK, TRAJ, BLOCK, WSUM>;
    }
};

}  // namespace psa
