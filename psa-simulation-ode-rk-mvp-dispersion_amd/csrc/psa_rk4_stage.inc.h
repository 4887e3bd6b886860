// psa_rk4_stage.inc.h -- the right-hand side of the Agrawal-Yaman 4/6-wave model fused with the Runge-Kutta stage update
// (gfx950): what the RK4 sweep kernels (psa_rk4_kernel.inc.h, the packed body) and the adaptive kernel (psa_rk45.hip) evaluate.
#pragma once
#include "psa_rk4_prims.inc.h"

namespace psa {

// ---- right-hand side, fused with the Runge-Kutta stage update -------------------------------------------
// a  = [Re A1, Im A1, Re A2, ...];  returns  out = base + c * dA/dz(a)   (FUSED)   or   out = dA/dz(a)  (c = 1).
// The stage coefficient c never appears as an instruction: the caller passes it folded into the constants
//   g = c*gamma, tg = 2*c*gamma, ha = -c*alpha/2, (Er, Ei) = 2*c*gamma*exp(+i*dbeta*z)  per sideband pair,
// and `base` simply seeds the FMA chain that the un-fused form would start with a multiply.
//
//   dA_j/dz = (-alpha/2 + i*gamma*f_j) A_j + i*conj(partner) * F            (yaman_model.py:123-186)
//   f_j = P_j + 2*sum_{k!=j} P_k = 2*S - P_j                                 (yaman_model.py:148-151)
//   pumps:     F = 2*gamma*exp(+i dbeta z) * (A_s A_i)                        (yaman_model.py:174,177-178)
//   sidebands: F = 2*gamma*exp(-i dbeta z) * (A_p1 A_p2)                      (yaman_model.py:175,180-181)
// 64 DP instructions for NW = 4 either way (p: 8, S/g_j: 8, two products: 8, two F: 8, eight 4-deep chains: 32).
// LOSS = false is the reference's own `alpha == 0.0` branch (_linear_loss_terms returns zeros, yaman_model.py:130-131):
// the -alpha/2 links disappear from all 2*NW chains (8 instructions per evaluation for 4 waves).
//
// CROSS = true (4 waves; the RK4 sweep steps ask for it) pairs the same triple products CROSSWISE, at the same 64:
//   H23 = E*(conj(A2)*A3)   H14 = E*(conj(A1)*A4)
//   pump 1: i*H23*A4    pump 2: i*H14*A3    signal: i*conj(H14)*A2    idler: i*conj(H23)*A1
// (two conjugate products: 8, two H: 8, the chains as before).  Every pair of members -- waves 1 and 2, waves 3 and 4 -- is
// then ONE expression with the partner's operands exchanged, the H included: exchanging (A1 <-> A2, A3 <-> A4) permutes the
// outputs and changes no bit, and where A2 == A1 and A4 == A3 the two H are the same expression on the same operands, so
// half of the stage repeats the other half (yaman_stage_mirrored).  With six waves the pumps sum over the pairs and the
// crosswise form would cost 64 instead of 52: NW == 6 keeps the form above whatever CROSS says, and so does RK45
// (psa_rk45.hip: its goldens pin accepted and rejected step counts).
//
// REALE = true (crosswise 4 waves only; the frame-anchored step's two midpoint stages) is the same stage where the phase
// factor is REAL: Er[0] holds it, Ei is not read, and each H = e*b is two multiplications instead of a complex product.
template <typename T, int NW, bool FUSED, bool LOSS = true, bool CROSS = false, bool REALE = false>
__device__ __forceinline__ void yaman_stage(const T (&a)[2 * NW], const T (&base)[2 * NW],
                                            const T (&Er)[(NW - 2) / 2], const T (&Ei)[(NW - 2) / 2], const T g,
                                            const T tg, const T ha, T (&out)[2 * NW]) {
    static_assert(!REALE || (CROSS && NW == 4), "the real phase factor exists for the crosswise 4-wave stage");
    constexpr int NP = (NW - 2) / 2;
    T p[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) p[j] = fma_(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]);
    T s = (p[0] + p[1]) + (p[2] + p[3]);
    if constexpr (NW == 6) s += (p[4] + p[5]);
    const T gs = tg * s;  // c*gamma * 2S
    T gj[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) gj[j] = fma_(-g, p[j], gs);  // c*gamma * f_j

    // first two links of each chain: gsig * v  +  [ha * component]  [+ base]
    auto link = [&](const T gsig, const T v, const int c) -> T {
        if constexpr (LOSS) return fma_(gsig, v, FUSED ? fma_(ha, a[c], base[c]) : ha * a[c]);
        else return FUSED ? fma_(gsig, v, base[c]) : gsig * v;
    };

    const T x1 = a[0], y1 = a[1], x2 = a[2], y2 = a[3];
    if constexpr (CROSS && NW == 4) {
        const T x3 = a[4], y3 = a[5], x4 = a[6], y4 = a[7];
        const T b23r = fma_(x2, x3, y2 * y3), b23i = fma_(x2, y3, -(y2 * x3));  // conj(A2)*A3
        const T b14r = fma_(x1, x4, y1 * y4), b14i = fma_(x1, y4, -(y1 * x4));  // conj(A1)*A4
        const T h23r = REALE ? Er[0] * b23r : fma_(Er[0], b23r, -(Ei[0] * b23i));
        const T h23i = REALE ? Er[0] * b23i : fma_(Er[0], b23i, Ei[0] * b23r);
        const T h14r = REALE ? Er[0] * b14r : fma_(Er[0], b14r, -(Ei[0] * b14i));
        const T h14i = REALE ? Er[0] * b14i : fma_(Er[0], b14i, Ei[0] * b14r);
        // pump1: (ha + i g1) A1 + i H23 A4 ;  pump2: (ha + i g2) A2 + i H14 A3
        out[0] = fma_(-y4, h23r, fma_(-x4, h23i, link(-gj[0], y1, 0)));
        out[1] = fma_(x4, h23r, fma_(-y4, h23i, link(gj[0], x1, 1)));
        out[2] = fma_(-y3, h14r, fma_(-x3, h14i, link(-gj[1], y2, 2)));
        out[3] = fma_(x3, h14r, fma_(-y3, h14i, link(gj[1], x2, 3)));
        // signal: (ha + i g3) A3 + i conj(H14) A2 ;  idler: (ha + i g4) A4 + i conj(H23) A1
        out[4] = fma_(-y2, h14r, fma_(x2, h14i, link(-gj[2], y3, 4)));
        out[5] = fma_(x2, h14r, fma_(y2, h14i, link(gj[2], x3, 5)));
        out[6] = fma_(-y1, h23r, fma_(x1, h23i, link(-gj[3], y4, 6)));
        out[7] = fma_(x1, h23r, fma_(y1, h23i, link(gj[3], x4, 7)));
        return;
    }
    const T q12r = fma_(x1, x2, -(y1 * y2)), q12i = fma_(x1, y2, y1 * x2);  // A1*A2

    T Fpr = T{}, Fpi = T{};  // sum over pairs of E_p * (A_s A_i): drives both pumps
#pragma unroll
    for (int pr = 0; pr < NP; ++pr) {
        const int cs = 4 + 4 * pr;  // component index of Re A_signal of this pair
        const T xs = a[cs], ys = a[cs + 1], xi = a[cs + 2], yi = a[cs + 3];
        const T qr = fma_(xs, xi, -(ys * yi)), qi = fma_(xs, yi, ys * xi);  // A_s*A_i
        if (pr == 0) {
            Fpr = fma_(Er[pr], qr, -(Ei[pr] * qi));
            Fpi = fma_(Er[pr], qi, Ei[pr] * qr);
        } else {
            Fpr = fma_(Er[pr], qr, fma_(-Ei[pr], qi, Fpr));
            Fpi = fma_(Er[pr], qi, fma_(Ei[pr], qr, Fpi));
        }
        // conj(E_p) * (A1 A2): drives this pair's signal and idler
        const T Fsr = fma_(Er[pr], q12r, Ei[pr] * q12i);
        const T Fsi = fma_(Er[pr], q12i, -(Ei[pr] * q12r));
        const T gS = gj[2 + 2 * pr], gI = gj[3 + 2 * pr];
        // signal: (ha + i gS) A_s + i conj(A_i) Fs
        out[cs] = fma_(yi, Fsr, fma_(-xi, Fsi, link(-gS, ys, cs)));
        out[cs + 1] = fma_(xi, Fsr, fma_(yi, Fsi, link(gS, xs, cs + 1)));
        // idler:  (ha + i gI) A_i + i conj(A_s) Fs
        out[cs + 2] = fma_(ys, Fsr, fma_(-xs, Fsi, link(-gI, yi, cs + 2)));
        out[cs + 3] = fma_(xs, Fsr, fma_(ys, Fsi, link(gI, xi, cs + 3)));
    }
    // pump1: (ha + i g1) A1 + i conj(A2) Fp ;  pump2: (ha + i g2) A2 + i conj(A1) Fp
    out[0] = fma_(y2, Fpr, fma_(-x2, Fpi, link(-gj[0], y1, 0)));
    out[1] = fma_(x2, Fpr, fma_(y2, Fpi, link(gj[0], x1, 1)));
    out[2] = fma_(y1, Fpr, fma_(-x1, Fpi, link(-gj[1], y2, 2)));
    out[3] = fma_(x1, Fpr, fma_(y1, Fpi, link(gj[1], x2, 3)));
}

// ---- the stage for MIRRORED points: A2 == A1 and A4 == A3 bit for bit (4 waves) ------------------------------------
// The crosswise yaman_stage (CROSS) with the duplicates removed.  There, out[0..1] / out[2..3] are one expression with
// (A1, A4, H23) and (A2, A3, H14) exchanged, out[4..5] / out[6..7] likewise, and on a mirrored point H23 and H14 are the same
// expression on the same operands.  So a point that starts with equal pumps and equal sidebands keeps them equal, in every
// bit, through every stage and step, and half of the stage repeats the other half.  This is that stage restricted to waves
// 1 and 3 with the partner's operands replaced by the wave's own:  a = [Re A1, Im A1, Re A3, Im A3],  sg = 2*tg,
//   b = conj(A1)*A3,  h = E*b,   pump: i*h*A3,   sideband: i*conj(h)*A1.
// Every value keeps the expression it has there, with one exception:  tg * ((p0 + p0) + (p2 + p2))  is formed as
// (2*tg) * (p0 + p2).  Scaling by two commutes with rounding, so the two are the same number unless 2*(p0 + p2) overflows
// (a power above 2^1022); there the general form gives inf and this one a finite gs, but gj * max(|x|, |y|) >= g * 2^1532
// overflows all the same and the step ends non-finite in both -- first_bad_step is the same, only the inf / NaN pattern of
// a state that has already failed may differ.
// 32 DP instructions instead of 64 (p: 4, gs: 2, g_j: 2, b: 4, h: 4, four 4-deep chains: 16), in every stage of the step;
// 30 with REALE (h = Er*b: 2), as in yaman_stage.
// FUSED = false is the plain dA/dz, as in yaman_stage (the float32 steps).
template <typename T, bool LOSS = true, bool FUSED = true, bool REALE = false>
__device__ __forceinline__ void yaman_stage_mirrored(const T (&a)[4], const T (&base)[4], const T Er, const T Ei, const T g,
                                                     const T sg, const T ha, T (&out)[4]) {
    const T x1 = a[0], y1 = a[1], xs = a[2], ys = a[3];
    const T p0 = fma_(x1, x1, y1 * y1), p2 = fma_(xs, xs, ys * ys);
    const T gs = sg * (p0 + p2);
    const T g1 = fma_(-g, p0, gs), g3 = fma_(-g, p2, gs);
    auto link = [&](const T gsig, const T v, const int c) -> T {
        if constexpr (LOSS) return fma_(gsig, v, FUSED ? fma_(ha, a[c], base[c]) : ha * a[c]);
        else return FUSED ? fma_(gsig, v, base[c]) : gsig * v;
    };
    const T br = fma_(x1, xs, y1 * ys), bi = fma_(x1, ys, -(y1 * xs));  // conj(A1)*A3
    const T hr = REALE ? Er * br : fma_(Er, br, -(Ei * bi));
    const T hi = REALE ? Er * bi : fma_(Er, bi, Ei * br);
    out[0] = fma_(-ys, hr, fma_(-xs, hi, link(-g1, y1, 0)));
    out[1] = fma_(xs, hr, fma_(-ys, hi, link(g1, x1, 1)));
    out[2] = fma_(-y1, hr, fma_(x1, hi, link(-g3, ys, 2)));
    out[3] = fma_(x1, hr, fma_(y1, hi, link(g3, xs, 3)));
}

// plain dA/dz of the RK4 sweeps (the float32 steps and the LDS-staged A/B variant, which keep k1..k4 as such): crosswise for 4 waves
template <typename T, int NW, bool LOSS = true>
__device__ __forceinline__ void yaman_rhs(const T (&a)[2 * NW], const T (&Er)[(NW - 2) / 2],
                                          const T (&Ei)[(NW - 2) / 2], const T g, const T tg, const T ha,
                                          T (&k)[2 * NW]) {
    yaman_stage<T, NW, false, LOSS, true>(a, a, Er, Ei, g, tg, ha, k);
}

}  // namespace psa
