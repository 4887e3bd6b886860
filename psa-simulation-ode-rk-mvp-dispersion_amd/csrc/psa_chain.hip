// psa_chain.hip -- the span epilogue of a fibre chain (psa_rk4_chain_*): concatenated spans, each one launch of the
// unchanged RK4 sweep kernels, joined on the device without a host synchronisation.
//
// Gauge.  The sweep kernels integrate a span on its LOCAL coordinate zeta in [0, L_s] with the FWM factor e^{+-i dbeta_s
// zeta}; the physical factor is e^{+-i Theta(z)}, Theta(z) = Theta_s + dbeta_s zeta, Theta_s = sum_{k<s} dbeta_k L_k.  The
// kernels therefore integrate B with B_sig = A_sig e^{+i Theta_s} and every other wave equal to A (a3 a4 = b3 b4 e^{-i
// Theta_s}; the Kerr terms are phase-blind).  Six waves: the signal of pair k (waves 2 and 4) takes its own Theta^(k).
// Three waves [p, s, i] (the single-pump model, psa_rk4_single_pump_chain_*): the same rule with the signal at index 1
// (a_s a_i = b_s b_i e^{-i Theta_s}); `sig_wave` names the index, and that family has no p_end / p_max (both null).
// K signals (the multi-channel model, psa_rk4_pairs_chain_*): the six-wave rule for every pair, signal k at wave 2 + 2k with
// its own Theta^(k) = sum_{j<s} dbeta_{j,k} L_j; in the pumps' sum_k E_k A_sk A_ik every pair's phase cancels in its own term.
// M lines (the multi-line model, psa_rk4_comb_chain_*): the field of line m is A_m e^{i Phi_m(z)}, Phi_m = Phi_{s,m} + kappa_{s,m}
// zeta, Phi_{s,m} = sum_{j<s} kappa_{j,m} L_j, and EVERY line takes its own phase: B_m = A_m e^{+i Phi_{s,m}} turns the span's
// equations into the kernel's (A o U = B o e^{i kappa_s zeta}).  That is the K-signal rule with M "signals" at consecutive waves
// 0..M-1, kappa in the place of dbeta.
// In general: `n_sig` signals at waves sig_wave + sig_stride * k (stride 2: an idler after every signal; 1: the comb), signal 0
// with (theta, dbeta), signal k >= 1 with row k - 1 of (theta2, dbeta2), rows `sig_ld` elements apart.
// At the boundary s -> s+1 the next span starts from B'_j = T_s[j] B_j, times e^{+i dbeta_s L_s} for the signal(s);
// reported amplitudes are brought back to A with e^{-i Theta_s}.  Theta is kept per point in float64 in HBM for both
// precisions (the kernels form dbeta*z in float64 as well).
//
// One epilogue launch per span, one thread per point, every access a coalesced SoA row:
//   fold      spans >= 1 wrote their summary into scratch: p_max / p_wave_max NaN-propagating max into the running
//             buffers, p_end / p_wave_end replaced, first_bad_step first failure wins (+ the span's step offset);
//   traj      the span's saved rows: signal column(s) rotated by e^{-i Theta_s} (spans >= 1);
//   last      a_end (A frame) = the span's a_end rotated by e^{-i Theta_s};
//   boundary  otherwise: the next span's a0 = T_s B (+ the gauge phase), and Theta += dbeta_s L_s.
#include <hip/hip_runtime.h>

#include "psa_internal.h"

namespace psa {

namespace {

// z -> z e^{-i theta} (sign = -1) or z e^{+i theta} (sign = +1), in float64, rounded to T
template <typename T>
__device__ __forceinline__ void rotate(T &re, T &im, double c, double s) {
    const double r = (double)re, i = (double)im;
    re = (T)(r * c - i * s);
    im = (T)(r * s + i * c);
}

template <typename T>
__device__ __forceinline__ void nanmax_into(T &m, T v) {
    m = (v > m || v != v) ? v : m;   // np.max: a NaN on either side is sticky
}

template <typename T>
__global__ void __launch_bounds__(256) chain_epilogue_kernel(ChainEpilogue<T> e) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    const long long n = e.n;
    const int nw = e.n_waves, sig = e.sig_wave, stride = e.sig_stride;

    if (e.fold) {
        if (e.p_max) {
            nanmax_into(e.p_max[i], e.p_max_s[i]);
            e.p_end[i] = e.p_end_s[i];
        }
        const long long b = e.first_bad_s[i];
        if (e.first_bad[i] < 0 && b >= 0) e.first_bad[i] = b + e.step_offset;
        if (e.wave_end) {
            for (int w = 0; w < nw; ++w) {
                nanmax_into(e.wave_max[(long long)w * n + i], e.wave_max_s[(long long)w * n + i]);
                e.wave_end[(long long)w * n + i] = e.wave_end_s[(long long)w * n + i];
            }
        }
    }

    // signal k: wave sig + stride * k, its Theta and its mismatch
    auto theta_of = [&](const int k) -> double * { return k == 0 ? e.theta + i : e.theta2 + (long long)(k - 1) * e.sig_ld + i; };
    auto dbeta_of = [&](const int k) -> double {
        return (double)(k == 0 ? e.dbeta[i] : e.dbeta2[(long long)(k - 1) * e.sig_ld + i]);
    };

    if (e.a_end_out)   // last span: the state, brought to the A frame below
        for (int c = 0; c < 2 * nw; ++c) e.a_end_out[(long long)c * n + i] = e.a_end_s[(long long)c * n + i];

    if (!e.first) {   // Theta_s = 0 in the first span: nothing to rotate (the `theta` buffers are not read there)
        for (int k = 0; k < e.n_sig; ++k) {
            const int w = sig + stride * k;
            double c, s;
            sincos(-*theta_of(k), &s, &c);
            if (e.traj) {
                // rows [0, rows) of this span, (re, im) pairs at ((row * nw + w) * ld + i) * 2
                for (long long r = 0; r < e.rows; ++r) {
                    T *p = e.traj + ((r * nw + w) * e.traj_ld + i) * 2;
                    rotate(p[0], p[1], c, s);
                }
            }
            if (e.a_end_out) rotate(e.a_end_out[(long long)(2 * w) * n + i], e.a_end_out[(long long)(2 * w + 1) * n + i], c, s);
        }
    }
    if (e.a_end_out) return;

    // boundary s -> s+1: B' = T_s B, signal k times e^{+i dbeta_s,k L_s}; Theta^(k) += dbeta_s,k L_s
    for (int w = 0; w < nw; ++w) {
        T re = e.a_end_s[(long long)(2 * w) * n + i], im = e.a_end_s[(long long)(2 * w + 1) * n + i];
        const int k = (w - sig) / stride;
        if (w >= sig && (w - sig) % stride == 0 && k < e.n_sig) {
            double *th = theta_of(k);
            const double ph = dbeta_of(k) * e.seg_len;
            *th = (e.first ? 0.0 : *th) + ph;
            double sp, cp;
            sincos(ph, &sp, &cp);
            rotate(re, im, cp, sp);
        }
        if (e.transfer) {
            const long long j = e.transfer_stride ? i : 0;
            const long long ld = e.transfer_stride ? n : 1;
            const double tr = (double)e.transfer[(long long)(2 * w) * ld + j];
            const double ti = (double)e.transfer[(long long)(2 * w + 1) * ld + j];
            const double r = (double)re, m = (double)im;
            re = (T)(tr * r - ti * m);
            im = (T)(tr * m + ti * r);
        }
        e.a0_next[(long long)(2 * w) * n + i] = re;
        e.a0_next[(long long)(2 * w + 1) * n + i] = im;
    }
}

template <typename T>
hipError_t launch_epilogue(hipStream_t s, const ChainEpilogue<T> &e) {
    if (e.n == 0) return hipSuccess;
    hipLaunchKernelGGL((chain_epilogue_kernel<T>), dim3((unsigned)((e.n + 255) / 256)), dim3(256), 0, s, e);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_chain_epilogue_f64(hipStream_t s, const ChainEpilogue<double> &e) { return launch_epilogue(s, e); }
hipError_t launch_chain_epilogue_f32(hipStream_t s, const ChainEpilogue<float> &e) { return launch_epilogue(s, e); }

}  // namespace psa
