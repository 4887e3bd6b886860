// psa_rk4_pk_frame.inc.h -- what the float32 kernels with TWO sweep points per lane share besides their step: which points a lane
// holds and how it loads and stores them, the finite test, the fold of the compensated state and the row maxima.  Used by
// rk4_sweep_single_pump_pk_kernel (all of it) and rk4_sweep_comb_pk_kernel (all but pk_row_max, which moves one instruction of
// one of its instantiations); rk4_sweep_pk_kernel (psa_rk4_pk_kernel.inc.h and its body) takes pk_track, pk_fold, splat2 and
// f32x2_u, since the lane record changes that unit's code in every form tried.
//
//   layout   lane i holds points 2i and 2i+1 in the halves of an f32x2, lanes = (N + 1) / 2; the odd tail's slot 1 repeats slot 0
//            and is never stored; a wave whose lanes all hold two real points (wave_full, wave-uniform) moves the adjacent pair
//            with 8-byte accesses at float alignment, the one other wave goes element by element.
//
// Every piece here leaves the device code of the three units the text it was with the piece spelled out in each kernel
// (tools/asm_equal.sh, profiles/pk_frame.log).  That is why the rest of the frame -- the first_bad store, the stores of a saved
// row and of the last one, and the loop that orders seeds, steps and rows -- is still each kernel's own text: as functions
// those pieces compile to other code, the last-row stores to 20 more VGPRs.  Keep to the forms used here when
// a piece is added: a kernel array that a lambda captures is no longer split into registers before inlining, so even the
// order of two declarations can change the code.
#pragma once
#include "psa_rk4_prims.inc.h"

namespace psa {

__device__ __forceinline__ f32x2 splat2(float x) { return (f32x2){x, x}; }

typedef float f32x2_u __attribute__((ext_vector_type(2), aligned(4)));   // an 8-B access at float alignment (odd N rows)

// |A|^2 of a packed pair
__device__ __forceinline__ f32x2 pk_abs2(const f32x2 re, const f32x2 im) { return fma_(re, re, im * im); }

// The points of one lane.
struct PkLane {
    long long idx, N;   // lane of the sweep, points of the sweep
    long long pt[2];    // odd tail: slot 1 repeats slot 0
    bool live1;         // slot 1 holds a real point (else computed but never stored)
    bool wave_full;     // wave-uniform: every lane of this wave holds two real points -> 8-B loads / stores of the adjacent pair,
                        // 16-B trajectory stores; the (at most one) wave with the odd tail or past-the-end lanes goes element-wise

    // false: the lane lies behind the last point and leaves the kernel.  wave_full is read among the lanes that stay.
    __device__ __forceinline__ bool init(const long long lane, const long long n_points) {
        idx = lane;
        N = n_points;
        pt[0] = 2 * idx;
        pt[1] = (2 * idx + 1 < N) ? 2 * idx + 1 : 2 * idx;
        live1 = 2 * idx + 1 < N;
        if (pt[0] >= N) return false;
        wave_full = __builtin_amdgcn_readfirstlane((int)(2 * (idx | 63) + 1 < N)) != 0;
        return true;
    }
    // The comb kernel calls this where its z-loop loads or stores per point: the indices pass through an empty asm there, so the
    // 2M-fold addresses formed from them stay inside that block.  Hoisted out of the loop as invariants they would be held in
    // registers across every step, and from M = 11 spilled to scratch memory.
    __device__ __forceinline__ void pin_points() { asm volatile("" : "+v"(pt[0]), "+v"(pt[1])); }

    __device__ __forceinline__ f32x2 load2(const float *base, const int stride) const {   // base[pt0 * stride], base[pt1 * stride]
        if (stride == 0) return splat2(base[0]);
        if (wave_full) return *reinterpret_cast<const f32x2_u *>(base + pt[0]);
        return (f32x2){base[pt[0]], base[pt[1]]};
    }
    __device__ __forceinline__ void store2(float *base, const f32x2 v) const {   // base[pt0], base[pt1]
        if (wave_full) {
            *reinterpret_cast<f32x2_u *>(base + pt[0]) = v;
        } else {
            base[pt[0]] = v.x;
            if (live1) base[pt[1]] = v.y;
        }
    }
};

// The finite test per packed half: sum_c 0*y_c is NaN exactly for a non-finite component.  bad[h] keeps the first such step.
template <int NC, typename Step>
__device__ __forceinline__ void pk_track(const f32x2 (&y)[NC], const int step, Step (&bad)[2]) {
    f32x2 t = f32x2{};
#pragma unroll
    for (int c = 0; c < NC; ++c) t = fma_(y[c], f32x2{}, t);
    if (bad[0] < 0 && t.x != t.x) bad[0] = step;
    if (bad[1] < 0 && t.y != t.y) bad[1] = step;
}

// Compensated state y = yb + dl: the increments collect in the small offset dl, which is folded here into the base yb with
// its rounding residue kept (Fast2Sum); yb_at(c) and dl_at(c) give the component wherever the kernel keeps it.
template <int NC, typename Yb, typename Dl>
__device__ __forceinline__ void pk_fold(f32x2 (&y)[NC], Yb &&yb_at, Dl &&dl_at) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x2 b = yb_at(c), d = dl_at(c);
        const f32x2 sum = b + d;
        dl_at(c) = d - (sum - b);
        yb_at(c) = sum;
        y[c] = sum;
    }
}

// np.max of |A_j|^2 over saved rows, which propagates NaN
template <int NW>
__device__ __forceinline__ void pk_row_max(const f32x2 (&y)[2 * NW], f32x2 (&pm)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const f32x2 pw = pk_abs2(y[2 * j], y[2 * j + 1]);
        pm[j].x = (pw.x > pm[j].x || pw.x != pw.x) ? pw.x : pm[j].x;
        pm[j].y = (pw.y > pm[j].y || pw.y != pw.y) ? pw.y : pm[j].y;
    }
}

}  // namespace psa
