// psa_rk4_prims.inc.h -- the device primitives every RK4 sweep kernel family is written in (gfx950): arithmetic types, streaming
// stores, the exact phase, the rotation, the finite test, the DPP lane exchange.  No kernel and no model.
#pragma once
#include <hip/hip_runtime.h>

namespace psa {

__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// two float32 sweep points per lane: <2 x float> arithmetic selects v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma_(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// (re, im) as one naturally aligned 2-element vector: 16-B (f64) / 8-B (f32) global stores
template <typename T> struct PairOf;
template <> struct PairOf<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct PairOf<float> { typedef float type __attribute__((ext_vector_type(2))); };

// Streaming store of one (re, im) pair at  sbase + voff : sbase wave-uniform (an SGPR pair), voff the lane's 32-bit byte
// offset.  This is the global_store "saddr" form; written as inline assembly because the compiler, left to itself, widens
// the lane offset to 64 bits inside the z-loop and then spends a v_lshl_add_u64 per store on the address.
// HAZARD: on gfx90a / gfx940 / gfx950 a VMEM store of MORE than 64 bits of data must not be followed within two wait
// states by a VALU instruction that overwrites the data VGPRs (LLVM's GCNHazardRecognizer inserts the s_nop for stores it
// can see; it cannot see into inline assembly).  The 16-B forms therefore carry their own two wait states (as two 4-byte
// `s_nop 0`, so that the 8-byte encodings after them stay on 8-byte boundaries): without them the packed
// float32 kernel, which assembles each store's four floats in a temporary it reuses at once, wrote corrupt rows.
#ifndef PSA_TRAJ_F64_MOD      // A/B hook (tools/ab_build.sh): -DPSA_TRAJ_F64_MOD='""' = default (write-back) stores
#define PSA_TRAJ_F64_MOD " nt"
#endif
__device__ __forceinline__ void store_pair_nt(const void *sbase, const unsigned voff, const PairOf<double>::type v) {
    asm volatile("global_store_dwordx4 %0, %1, %2" PSA_TRAJ_F64_MOD "\n\ts_nop 0\n\ts_nop 0" : : "v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ void store_pair_nt(const void *sbase, const unsigned voff, const PairOf<float>::type v) {
    asm volatile("global_store_dwordx2 %0, %1, %2 nt" : : "v"(voff), "v"(v), "s"(sbase) : "memory");
}
// two adjacent float32 points' (re, im) pairs in one 16-B store (the packed kernel: points 2i and 2i+1 share a lane)
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_quad_nt(const void *sbase, const unsigned voff, const f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 0\n\ts_nop 0" : : "v"(voff), "v"(v), "s"(sbase) : "memory");
}

// cos/sin of a float64 phase, delivered in the working precision.
template <typename T> struct Phase;
template <> struct Phase<double> {
    static constexpr int RESYNC = 64;  // steps after which the rotation recurrence is re-seeded exactly
    static __device__ __forceinline__ void eval(double ph, double &c, double &s) { sincos(ph, &s, &c); }
};
#ifndef PSA_F32_RESYNC          // A/B hook (tools/ab_build_f32.sh)
#define PSA_F32_RESYNC 16   // 20 / 32 / 64 measured within 2 % of each other on the config-4 shard; accuracy guard identical
#endif
template <> struct Phase<float> {
    static constexpr int RESYNC = PSA_F32_RESYNC;
    // dbeta*z reaches 1e4..1e5 rad at 1e6 steps: reduce in f64, then an f32 sincos on [-pi, pi].
    static __device__ __forceinline__ void eval(double ph, float &c, float &s) {
        const double r = ph - 6.283185307179586 * rint(ph * 0.15915494309189535);
        sincosf((float)r, &s, &c);
    }
};

// (Er,Ei) *= (rc,rs)
template <typename T>
__device__ __forceinline__ void rotate(T &Er, T &Ei, const T rc, const T rs) {
    const T nr = fma_(Er, rc, -(Ei * rs));
    const T ni = fma_(Er, rs, Ei * rc);
    Er = nr;
    Ei = ni;
}

// true iff any component is NaN/Inf: x*0 is NaN exactly for non-finite x.
template <typename T, int NC>
__device__ __forceinline__ bool any_nonfinite(const T (&y)[NC]) {
    T t = T(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) t = fma_(y[c], T(0), t);
    return t != t;
}

template <int CTRL> __device__ __forceinline__ double quad_xchg(const double v) {   // the lane CTRL names, by two DPP moves
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
constexpr int QUAD_PAIR = 0xB1;          // quad_perm:[1,0,3,2]: the pair partner
constexpr int QUAD_OTHER = 0x4E;         // quad_perm:[2,3,0,1]: the same role in the other pair
constexpr int ROW_HALF_MIRROR = 0x141;   // row_half_mirror: lane i <-> 7 - i of each 8
constexpr int ROW_MIRROR = 0x140;        // row_mirror: lane i <-> 15 - i of each 16

}  // namespace psa
