// psa_internal.h -- shared between the kernel TUs and the C-ABI TU (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psa_launch_rules.h"

namespace psa {

// Everything one sweep launch needs; passed by value as the kernel argument.
// All pointers are device pointers.  Strides are in elements: 1 = per point, 0 = broadcast.
template <typename T>
struct SweepArgs {
    const T *dbeta;      // [N]
    const T *dbeta2;     // [N] (6-wave) or nullptr
    const T *gamma;      // [N] | [1]
    const T *alpha;      // [N] | [1]
    const T *a0;         // SoA [2*NW][a0_ld]; a0_ld = N (per point) or 1 (broadcast, stride 0)
    T *a_end;            // SoA [2*NW][N]
    T *p_end;            // [N]
    T *p_max;            // [N]
    long long *first_bad;  // [N]
    T *traj;             // [n_saved][NW][traj_ld][2] ((re, im) pairs) or nullptr
    long long traj_ld;   // points per (row, wave) region of traj: n_points, or padded (psa_traj_ld)
    long long n_points;
    double z_max;
    int n_steps;
    int save_every;
    int gamma_stride, alpha_stride, a0_stride;  // 0 | 1
    long long a0_ld;
    // per-wave summary (the WSUM instantiations only; nullptr otherwise): SoA [NW][N]
    T *p_wave_end;       // |A_j|^2 at the last saved row
    T *p_wave_max;       // max over saved rows incl. z = 0 (NaN-propagating like np.max)
};

// Everything one adaptive (RK45) sweep launch needs; inputs as SweepArgs, per-point outputs SoA / [N].
template <typename T>
struct AdaptiveArgs {
    const T *dbeta, *dbeta2, *gamma, *alpha, *a0;
    T *a_end;                 // SoA [2*NW][N]
    T *p_end, *p_max;         // [N]
    int32_t *status;          // [N] 0 reached z_max, 1 step below the minimum, 2 max_steps attempts used
    T *z_end;                 // [N]
    long long *n_accepted, *n_rejected;   // [N]
    T *traj;                  // dense-output rows [n_out + 1][NW][traj_ld][2] or nullptr
    long long traj_ld;
    long long n_points;
    double z_max, rtol, atol, h_max, first_step;   // first_step 0: scipy's select_initial_step
    long long max_steps, n_out;
    int gamma_stride, alpha_stride, a0_stride;
    long long a0_ld;
};

// Everything one multi-channel sweep launch needs (two pumps and n_pairs signal/idler pairs, NW = 2 + 2*n_pairs waves
// [p1, p2, s_1, i_1, ..., s_K, i_K]; float64 only).  Strides as in SweepArgs; every output but the trajectory is always written.
struct PairsArgs {
    const double *dbeta;     // SoA [n_pairs][N]
    const double *gamma;     // [N] | [1]
    const double *alpha;     // [N] | [1]
    const double *a0;        // SoA [2*NW][a0_ld]
    double *a_end;           // SoA [2*NW][N]
    double *p_wave_end;      // SoA [NW][N] |A_j|^2 at the last saved row
    double *p_wave_max;      // SoA [NW][N] max over saved rows incl. z = 0 (NaN-propagating like np.max)
    long long *first_bad;    // [N]
    long long n_points;
    double z_max;
    int n_steps;
    int save_every;
    int n_pairs;             // 1..16
    int gamma_stride, alpha_stride, a0_stride;  // 0 | 1
    long long a0_ld;
    double *traj;            // [n_saved][NW][traj_ld][2] ((re, im) pairs) or nullptr
    long long traj_ld;       // points per (row, wave) region of traj: n_points, or padded (psa_traj_ld)
};

// Everything one single-pump sweep launch needs (one pump, a signal and an idler: NW = 3 waves [p, s, i]; float64 one point per
// lane, float32 two points per lane).  Strides as in SweepArgs; every output but the trajectory is always written.
template <typename T>
struct SinglePumpArgs {
    const T *dbeta;          // [N]
    const T *gamma;          // [N] | [1]
    const T *alpha;          // [N] | [1]
    const T *a0;             // SoA [6][a0_ld]
    T *a_end;                // SoA [6][N]
    T *p_wave_end;           // SoA [3][N] |A_j|^2 at the last saved row
    T *p_wave_max;           // SoA [3][N] max over saved rows incl. z = 0 (NaN-propagating like np.max)
    long long *first_bad;    // [N]
    T *traj;                 // [n_saved][3][traj_ld][2] ((re, im) pairs) or nullptr
    long long traj_ld;       // points per (row, wave) region of traj: n_points, or padded (psa_traj_ld)
    long long n_points;
    double z_max;
    int n_steps;
    int save_every;
    int gamma_stride, alpha_stride, a0_stride;  // 0 | 1
    long long a0_ld;
};

// Everything one multi-line ("comb") sweep launch needs (n_lines equally spaced lines, ascending in frequency; float64 one
// point per lane, float32 two points per lane).  Strides as in SweepArgs; every output but the trajectory is always written.
template <typename T>
struct CombArgs {
    const T *kappa;          // SoA [n_lines][N] propagation constant of every line, 1/length
    const T *gamma;          // [N] | [1]
    const T *alpha;          // [N] | [1]
    const T *a0;             // SoA [2*n_lines][a0_ld]
    T *a_end;                // SoA [2*n_lines][N]
    T *p_wave_end;           // SoA [n_lines][N] |A_m|^2 at the last saved row
    T *p_wave_max;           // SoA [n_lines][N] max over saved rows incl. z = 0 (NaN-propagating like np.max)
    long long *first_bad;    // [N]
    T *traj;                 // [n_saved][n_lines][traj_ld][2] ((re, im) pairs) or nullptr
    long long traj_ld;       // points per (row, line) region of traj: n_points, or padded (psa_traj_ld)
    long long n_points;
    double z_max;
    int n_steps;
    int save_every;
    int n_lines;             // 3..PSA_MAX_LINES
    int gamma_stride, alpha_stride, a0_stride;  // 0 | 1
    long long a0_ld;
};

// ---- sweep launchers: one kernel launch on s, nothing for n_points == 0; the caller has validated the arguments.  What they
// share is stated once: the rules (check mode, workgroup size, grid, LDS bytes; CheckMode) in psa_launch_rules.h, the dispatch
// and the launch in psa_launch.inc.h.  All take the trajectory from a.traj being non-null.
int simd_count(hipStream_t s);   // SIMDs (4 per CU) of the device a launch on s goes to, cached per device (psa_rk4_f64.hip)
// 4/6 waves: they own every launch-related PSA_OPT_* bit of `flags` (check mode, LDS staging, block size, LOSSLESS, the float64
// lane layout, float32 packing); the per-wave summary comes from a.p_wave_end being non-null (then no trajectory, LDS staging
// or BLOCK64).  256-thread workgroups unless BLOCK64 or LDS staging asks for 64; the two- and four-lane layouts take the rule.
hipError_t launch_sweep_f64(hipStream_t s, int n_waves, uint32_t flags, const SweepArgs<double> &a);
hipError_t launch_sweep_f32(hipStream_t s, int n_waves, uint32_t flags, const SweepArgs<float> &a);
// Multi-channel: pairs_lanes_per_point(n_pairs) * n_points lanes.  Reads CHECK_NAN / EXACT_STEP / LOSSLESS / BLOCK64; with a
// trajectory the workgroup is 256 whatever BLOCK64 says (1 <= n_pairs <= 16, the lanes fit the grid, traj_ld * 16 < 2^32).
hipError_t launch_sweep_pairs_f64(hipStream_t s, uint32_t flags, const PairsArgs &a);
// Single pump, one lane per point / two float32 points per lane.  They read CHECK_NAN / EXACT_STEP / LOSSLESS / BLOCK64
// (float32 has one register layout: LOSSLESS selects nothing); traj_ld * 16 < 2^32 in float64, traj_ld * 8 < 2^31 in float32.
hipError_t launch_sweep_single_pump_f64(hipStream_t s, uint32_t flags, const SinglePumpArgs<double> &a);
hipError_t launch_sweep_single_pump_f32(hipStream_t s, uint32_t flags, const SinglePumpArgs<float> &a);
// Multi-line, lanes as the single pump.  They read CHECK_NAN as a bool (the test runs after every step: EXACT_STEP selects
// nothing), LOSSLESS (nothing in float32) and BLOCK64 and pass the dynamic LDS bytes of their M and workgroup
// (3 <= n_lines <= PSA_MAX_LINES; trajectory bounds as the single pump).
hipError_t launch_sweep_comb_f64(hipStream_t s, uint32_t flags, const CombArgs<double> &a);
hipError_t launch_sweep_comb_f32(hipStream_t s, uint32_t flags, const CombArgs<float> &a);
// Adaptive (psa_rk45.hip): LOSSLESS is the only flag it reads; the workgroup is the rule without BLOCK64.
hipError_t launch_rk45_sweep_f64(hipStream_t s, int n_waves, uint32_t flags, const AdaptiveArgs<double> &a);

// aux kernels (psa_aux.hip)
hipError_t launch_aos_to_soa_f64(hipStream_t s, const double *aos, double *soa, long long n, int nc);
hipError_t launch_soa_to_aos_f64(hipStream_t s, const double *soa, double *aos, long long n, int nc);
hipError_t launch_aos_to_soa_f32(hipStream_t s, const float *aos, float *soa, long long n, int nc);
hipError_t launch_soa_to_aos_f32(hipStream_t s, const float *soa, float *aos, long long n, int nc);
// traj: device [rows][nw][n][2] -> NumPy [n][rows][nw][2]   (nc = 2*nw)
// `soa` points at the first point of the chunk; ld = points per row of the full device buffer (>= n)
hipError_t launch_traj_to_aos_f64(hipStream_t s, const double *soa, double *aos, long long n, long long ld, long long rows, int nc);
hipError_t launch_traj_to_aos_f32(hipStream_t s, const float *soa, float *aos, long long n, long long ld, long long rows, int nc);
hipError_t launch_yaman_rhs_f64(hipStream_t s, long long n, const double *z, const double *a, const double *gamma,
                                const double *alpha, const double *dbeta, double *out, double *lin, double *kerr,
                                double *fwm);
hipError_t launch_gain_summary_f64(hipStream_t s, long long n, const double *p_metric, const long long *first_bad,
                                   double p0_sig, int gain_db, double *gain_out, long long *best_index,
                                   double *best_gain, long long *n_finite, void *workspace);
hipError_t launch_gain_summary_f32(hipStream_t s, long long n, const float *p_metric, const long long *first_bad,
                                   double p0_sig, int gain_db, float *gain_out, long long *best_index,
                                   double *best_gain, long long *n_finite, void *workspace);
long long gain_summary_workspace_bytes(long long n);

// ---- fibre chains (psa_chain.hip): the epilogue launched after every span ------------------------------------
// All arrays are SoA device buffers over the n points; see psa_chain.hip for what each part does.
template <typename T>
struct ChainEpilogue {
    long long n;
    int n_waves;
    int sig_wave;               // the first wave that carries a Theta: 2 (two pumps in front), 1 (3 waves), 0 (the comb)
    int sig_stride;             // waves from one Theta-carrying wave to the next: 2 (an idler in between), 1 (the comb: every line)
    int n_sig;                  // signals, at waves sig_wave + sig_stride * k: 1 (3 and 4 waves), 2 (6 waves), K (the multi-channel
                                // model), M (the comb)
    int first;                  // span 0: Theta_0 = 0, no rotation, `theta` is initialised by the boundary
    int fold;                   // spans >= 1: fold the span's summary (the *_s buffers) into the running outputs
    const T *a_end_s;           // [2*NW][n] the span's a_end (B frame)
    const T *p_end_s, *p_max_s; // [n]
    const long long *first_bad_s;
    const T *wave_end_s, *wave_max_s;   // [NW][n] or nullptr
    T *p_end, *p_max;           // running outputs; both nullptr for a family without a signal summary (3 waves)
    long long *first_bad;
    T *wave_end, *wave_max;     // [NW][n] or nullptr
    long long step_offset;      // steps of the spans before this one
    double *theta, *theta2;     // float64 accumulated mismatch phase: [n] of signal 0, [n_sig - 1][sig_ld] of the others
    long long sig_ld;           // elements between the rows of theta2 and of dbeta2 (n where n_sig > 2 packs them)
    T *traj;                    // first row of this span in [rows][NW][traj_ld][2], or nullptr
    long long traj_ld, rows;
    T *a_end_out;               // last span: [2*NW][n] A-frame a_end; nullptr otherwise
    const T *transfer;          // boundary: [2*NW][n] (stride 1) or [2*NW] (stride 0); nullptr = identity
    int transfer_stride;
    const T *dbeta, *dbeta2;    // this span's: [n] of signal 0, [n_sig - 1][sig_ld] of the others
    double seg_len;
    T *a0_next;                 // [2*NW][n]
};
hipError_t launch_chain_epilogue_f64(hipStream_t s, const ChainEpilogue<double> &e);
hipError_t launch_chain_epilogue_f32(hipStream_t s, const ChainEpilogue<float> &e);

// ---- device-side dbeta producer (psa_dbeta.hip) ------------------------------------------------------------
constexpr int DBETA_MAX_ORDER = 8;
struct DbetaModel {
    double beta[DBETA_MAX_ORDER + 1];  // beta_n per length unit, n = 0..8 (DispersionParams.get_beta_n)
    double omega_ref, two_pi_c, atol, rtol;
    int method;        // 0 SYMMETRIC_EVEN, 1 GENERAL_TAYLOR
    int n_orders;      // SYMMETRIC_EVEN: even orders, summed in this order
    int orders[4];
    int max_order;     // GENERAL_TAYLOR
};
hipError_t launch_dbeta_grid_f64(hipStream_t s, const DbetaModel &m, double lambda1, const double *ax2, long long n2,
                                 const double *ax3, long long n3, long long first, long long n, double *out,
                                 unsigned char *valid);
hipError_t launch_dbeta_grid_f32(hipStream_t s, const DbetaModel &m, double lambda1, const double *ax2, long long n2,
                                 const double *ax3, long long n3, long long first, long long n, float *out,
                                 unsigned char *valid);
hipError_t launch_dbeta_pairs_f64(hipStream_t s, const DbetaModel &m, double omega_d, const double *ax1, long long n1,
                                  const double *ax2, long long n2, long long first, long long n, double *out1,
                                  double *out2);
hipError_t launch_dbeta_pairs_f32(hipStream_t s, const DbetaModel &m, double omega_d, const double *ax1, long long n1,
                                  const double *ax2, long long n2, long long first, long long n, float *out1,
                                  float *out2);

}  // namespace psa
