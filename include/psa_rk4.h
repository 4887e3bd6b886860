/*
 * psa_rk4.h -- C-ABI of libpsa_hip.so: the MI355X (gfx950) drop-in for the
 * reference's RK4 / Agrawal-Yaman hot path.
 *
 * The reference (Alxkov/PSA-simulation-ODE-RK-MVP-Dispersion) is pure Python and
 * has no FFI; its de-facto operator API is three nested call surfaces
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it
 * replaces (file:line into the upstream tree).  The binding a maintainer adds on
 * the reference side is a ctypes stub -- see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer;
 *   - return value: 0 ok, < 0 argument error (PSA_E_*), > 0 a hipError_t;
 *     psa_last_error() gives the message for the calling thread;
 *   - a per-point NUMERICAL failure (NaN/Inf) is never a return code: it is
 *     reported in first_bad_step[N] (the reference raises FloatingPointError
 *     per run, integrators.py:132-135, and its sweep drivers turn that into a
 *     NaN gain, scan_mismtach.py:391-392);
 *   - "host" functions are blocking and take host pointers in NumPy layout
 *     (complex128 = interleaved re,im); "_dev" functions take device (HBM)
 *     pointers in SoA layout and are asynchronous on the given hipStream_t;
 *   - thread-safe, also for concurrent calls on one device; no global mutable state
 *     except the per-thread error string and a mutex-protected pool of idle
 *     per-device call contexts (stream, events, <= 64 MB of device scratch, 1 MB of
 *     page-locked memory each) that the host-buffer entry points reuse between
 *     calls; psa_release_cache() destroys them.
 *
 * Wave order everywhere: [pump1, pump2, signal, idler] (n_waves = 4) or
 * [pump1, pump2, signal1, idler1, signal2, idler2] (n_waves = 6, build-defined
 * extension; the reference has no 6-wave model).  psa_rk4_sweep_* summarise wave
 * index 2 (the signal), as scan_mismtach.py:376 does; psa_rk4_sweep_waves_* add the
 * same summary for every wave (the idler's gain, the pumps' depletion).
 */
#ifndef PSA_RK4_H
#define PSA_RK4_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- argument-error codes (negative) ------------------------------------- */
#define PSA_OK            0
#define PSA_E_NWAVES     -1   /* n_waves not 4 or 6                                  */
#define PSA_E_NPOINTS    -2   /* n_points < 0                                        */
#define PSA_E_NSTEPS     -3   /* n_steps <= 0                                        */
#define PSA_E_ZMAX       -4   /* z_max <= 0 or not finite  (integrators.py:188-189)  */
#define PSA_E_SAVE_EVERY -5   /* save_every <= 0           (integrators.py:108-109)  */
#define PSA_E_NULLPTR    -6   /* a required pointer is NULL                          */
#define PSA_E_DEVICE     -7   /* device index out of range / no gfx950 device        */
#define PSA_E_DBETA2     -8   /* n_waves == 6 needs dbeta2; n_waves == 4 forbids it  */
#define PSA_E_TOO_LARGE  -9   /* trajectory does not fit (int64 / device memory), or n_points exceeds the launch grid */
#define PSA_E_DBETA_MODEL -10 /* dbeta producer: unknown method, bad even_orders / max_order / beta count  */
#define PSA_E_FLAGS      -11  /* options that exclude each other (two of SPLIT_POINT / ONE_LANE / QUAD_POINT, F32_SCALAR + F32_PACKED, QUAD with 6 waves) */
#define PSA_E_TOL        -12  /* psa_rk45_*: rtol < 100*DBL_EPSILON or not finite, atol <= 0 or not finite, h_max <= 0,
                                 first_step < 0 or not finite, max_steps < 1, n_out < 0 */
#define PSA_E_NPAIRS     -13  /* psa_rk4_sweep_pairs_*: n_pairs outside 1..PSA_MAX_PAIRS */
#define PSA_E_NLINES     (-14) /* psa_rk4_comb_*: n_lines outside 3..PSA_MAX_LINES (in parentheses, as a negative macro
                                   value should be; the thirteen above keep the spelling their tests read) */

/* The most points one launch takes: a launch has at most 2^32 - 1 threads in x and the two-lane float64 layout uses two
 * per point.  (2^31 - 256 float64 records are 189 GB: a 288 GB MI355X holds them, so the limit is stated, not theoretical.) */
#define PSA_MAX_POINTS   2147483392LL
/* The most signal/idler pairs of the multi-channel sweep (psa_rk4_sweep_pairs_*): one lane per pair, a point within one
 * 16-lane DPP row. */
#define PSA_MAX_PAIRS    16
/* The most lines of the multi-line ("comb") sweep (psa_rk4_comb_*): one point per lane (float64) or two (float32) with the
 * whole state in registers and LDS; 12 lines are the most that every instantiation holds without scratch memory
 * (DESIGN.md 3.3e, 3.3f). */
#define PSA_MAX_LINES    12

/* ---- flags ----------------------------------------------------------------- */
/* broadcast: the array has ONE entry used for every sweep point */
#define PSA_BCAST_GAMMA      (1u << 0)
#define PSA_BCAST_ALPHA      (1u << 1)
#define PSA_BCAST_A0         (1u << 2)
#define PSA_BCAST_TRANSFER   (1u << 3)   /* psa_rk4_chain_*: one transfer per boundary, used for every point */
/* options */
#define PSA_OPT_CHECK_NAN    (1u << 8)   /* SimulationConfig.check_nan (config.py:29): track first_bad_step over ALL
                                            n_steps (also the tail after the last saved row).  Without it
                                            first_bad_step is -1 everywhere and NaNs propagate silently.         */
#define PSA_OPT_EXACT_STEP   (1u << 9)   /* with CHECK_NAN: first_bad_step is the EXACT step index, as the reference's
                                            per-step test reports it (integrators.py:132-135).  float64: free -- the
                                            forward pass tests once per saved row and a wave with a newly failing point
                                            replays the steps since the previous test with a per-step test; float32:
                                            tested in the loop.  Without the flag first_bad_step is the LAST step of
                                            the first non-finite save block (the sweep drivers only need "did it
                                            fail").                                                                */
#define PSA_OPT_LDS_STAGING  (1u << 10)  /* keep y / y_stage / k-accumulator in LDS instead of VGPRs (the layout
                                            the north-star sketches; slower -- kept for the A/B in DESIGN.md)    */
#define PSA_OPT_BLOCK64      (1u << 11)  /* 64-thread workgroups (one wave) instead of 256                       */
#define PSA_OPT_LOSSLESS     (1u << 14)  /* the caller promises alpha == 0 for EVERY point: use the instantiation without
                                            the -alpha/2 terms (the reference's own `alpha == 0.0` branch,
                                            yaman_model.py:130-131; -10 % instructions).  The host-buffer entry points
                                            set it themselves when alpha is a broadcast 0; `_dev` callers pass it.    */
#define PSA_OPT_SPLIT_POINT  (1u << 15)  /* float64 only: force TWO LANES per sweep point (a point's waves divided between
                                            neighbouring lanes, partial sums exchanged by DPP): halves the sequential
                                            instruction stream per lane.  Default: chosen automatically when the sweep is
                                            smaller than the chip (2*N lanes still get one SIMD per wave: N <= 32 768).   */
#define PSA_OPT_QUAD_POINT   (1u << 18)  /* float64, n_waves == 4 only: force FOUR lanes per sweep point (one wave of the model
                                            per lane, sums and products exchanged by DPP within the quad): ~155
                                            instructions per step and lane.  Default: chosen automatically while 4*N
                                            lanes still get one SIMD per wave (N <= 16 384) -- the reference's own
                                            scenarios (1, 30, 100 points).                                          */
#define PSA_OPT_ONE_LANE     (1u << 16)  /* float64 only: never split a point over two lanes                              */
#define PSA_OPT_TRAJ_LD      (1u << 17)  /* `_dev` entry points: the trajectory buffer is [n_saved][n_waves][ld][2] with the
                                            leading dimension ld = psa_traj_ld(n_points, sizeof(element)) >= n_points
                                            instead of n_points: sizes whose wave regions would lie a multiple of 2 MiB
                                            apart are padded by 4 352 B, which lifts the store rate of every-step
                                            trajectories by 8-35 %.  The host-buffer entry points use
                                            it internally; the caller's array stays dense.                          */
#define PSA_OPT_F32_SCALAR   (1u << 12)  /* float32 only: force one sweep point per lane                          */
#define PSA_OPT_F32_PACKED   (1u << 13)  /* float32 only: force two points per lane (v_pk_fma_f32 packed math);
                                            this is also the default whenever n_points >= 2                      */

/* ---- environment ----------------------------------------------------------- */
int         psa_device_count(void);          /* number of visible HIP devices (0 if none / no driver) */
const char *psa_last_error(void);            /* message of the last failure on this thread            */
const char *psa_version(void);               /* "psa-hip <semver> gfx950"                              */
int64_t     psa_n_saved(int64_t n_steps, int32_t save_every);   /* n_steps / save_every + 1, integrators.py:115 */
int64_t     psa_traj_ld(int64_t n_points, int32_t elem_size);   /* leading dimension for PSA_OPT_TRAJ_LD (elem_size 4 | 8) */
int         psa_release_cache(void);         /* destroy the idle call contexts of every device; returns how many       */

/* ---- B3/B2: the sweep (host buffers, blocking) ----------------------------------
 * Replaces the body of the per-point loops scan_mismtach.py:357-392 and :694-738, i.e.
 * N x { simulation.run_single_simulation (simulation.py:349-357) -> integrators.integrate_interval
 * (integrators.py:150-204) -> integrate_fixed_step (:68-142) -> rk4_step (:25-61) ->
 * yaman_model.rhs_yaman_simplified (yaman_model.py:10-52) } plus the reduction
 * P3 = |A[:,2]|^2, max / last over saved rows (scan_mismtach.py:376-381, :27-40).
 *
 *   n_steps    = int(round(z_max/dz)) computed by the caller (integrators.py:194);
 *                the kernel steps on z_i = i * (z_max / n_steps)  (np.linspace, :195)
 *   dbeta      [N]   phase mismatch per point, 1/length          (parameters.py:236 CacheParams.delta_beta_1_m)
 *   dbeta2     [N]   second pair's mismatch (n_waves == 6) or NULL
 *   gamma      [N] | [1]    fiber.gamma_W_m   (parameters.py:166)
 *   alpha      [N] | [1]    fiber.alpha_1_m
 *   a0_re_im   [N][n_waves][2] | [1][n_waves][2]   initial amplitudes (simulation.py:103-123)
 *   a_end_re_im[N][n_waves][2]   state at the LAST SAVED row = step (n_steps/save_every)*save_every
 *   p_sig_end  [N]   |A_sig|^2 at that row            (gain_mode "end", scan_mismtach.py:36-37)
 *   p_sig_max  [N]   max over saved rows incl. z = 0  (gain_mode "max", :38-39; NaN-propagating like np.max)
 *   first_bad_step [N]  -1, or the 0-based step index after which the state was non-finite
 *   traj_or_null   [N][n_saved][n_waves][2]  every saved row (integrators.py:137-140), or NULL.  A launch with a
 *                  trajectory takes at most 2^27 - 1 points in float64 (2^28 - 1 in float32: rows are addressed with a
 *                  32-bit lane offset kept below 2^31; with PSA_OPT_SPLIT_POINT 2^32 / (n_waves * 16) - 1) and must fit
 *                  the device's free memory, else PSA_E_TOO_LARGE
 *   elapsed_ms_or_null  kernel time from hipEvents on the launch stream, or NULL
 */
int psa_rk4_sweep_f64(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                      int32_t save_every, const double *dbeta, const double *dbeta2, const double *gamma,
                      const double *alpha, const double *a0_re_im, uint32_t flags, double *a_end_re_im,
                      double *p_sig_end, double *p_sig_max, int64_t *first_bad_step, double *traj_or_null,
                      double *elapsed_ms_or_null);

/* float32 state/arithmetic variant (BASELINE config 4; build-defined, the reference forces complex128,
 * yaman_model.py:41-44).  The phase dbeta*z is still formed in float64.  z_max stays double. */
int psa_rk4_sweep_f32(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                      int32_t save_every, const float *dbeta, const float *dbeta2, const float *gamma,
                      const float *alpha, const float *a0_re_im, uint32_t flags, float *a_end_re_im,
                      float *p_sig_end, float *p_sig_max, int64_t *first_bad_step, float *traj_or_null,
                      double *elapsed_ms_or_null);

/* ---- the same sweep on buffers already resident in HBM (async on `stream`) -------
 * Device layout is SoA so that every wave instruction is a contiguous 512-B (f64) access:
 *   d_a0_soa    [2*n_waves][N] (or [2*n_waves][1] with PSA_BCAST_A0): row 2j = Re A_j, 2j+1 = Im A_j
 *   d_a_end_soa [2*n_waves][N]
 *   d_traj_soa  [n_saved][n_waves][ld][2] ((re, im) pairs: 16-B stores, 1 KiB per wave instruction) or NULL;
 *               ld = N, or psa_traj_ld(N, sizeof(element)) with PSA_OPT_TRAJ_LD (rows padded off a 2 MiB stride)
 * `stream` is a hipStream_t (NULL = default stream).  No allocation, no synchronisation: safe to capture
 * into a hipGraph.  This is what bench.py times and what the multi-GPU path calls per rank.
 */
int psa_rk4_sweep_f64_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                          int32_t save_every, const double *d_dbeta, const double *d_dbeta2,
                          const double *d_gamma, const double *d_alpha, const double *d_a0_soa, uint32_t flags,
                          double *d_a_end_soa, double *d_p_sig_end, double *d_p_sig_max,
                          int64_t *d_first_bad_step, double *d_traj_soa);

int psa_rk4_sweep_f32_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                          int32_t save_every, const float *d_dbeta, const float *d_dbeta2, const float *d_gamma,
                          const float *d_alpha, const float *d_a0_soa, uint32_t flags, float *d_a_end_soa,
                          float *d_p_sig_end, float *d_p_sig_max, int64_t *d_first_bad_step, float *d_traj_soa);

/* ---- the sweep with a per-wave power summary ----------------------------------------------------------------
 * psa_rk4_sweep_f64 / _f32 (and their _dev forms) with two more outputs: the end and maximum power of EVERY wave, so the
 * idler's conversion gain and the pumps' depletion need no trajectory.  The reference's seeded mismatch scan applies
 * _select_power_metric to the idler as well as the signal and reports Gi next to Gs (scan_mismtach.py:139-153, :183-199).
 *   p_wave_end [N][n_waves]   |A_j|^2 at the last saved row (the row of a_end); column 2 == p_sig_end bit for bit
 *   p_wave_max [N][n_waves]   max of |A_j|^2 over the saved rows incl. z = 0, NaN-propagating like np.max; column 2 ==
 *                             p_sig_max bit for bit
 * _dev forms: d_p_wave_end_soa / d_p_wave_max_soa are [n_waves][N] device buffers; asynchronous on `stream`.
 * Everything else -- arguments, a_end, p_sig_*, first_bad_step, the layout flags and the automatic layout choice -- is as
 * for psa_rk4_sweep_*, with these restrictions (PSA_E_FLAGS): traj_or_null must be NULL (a trajectory holds every wave
 * already), and PSA_OPT_LDS_STAGING and PSA_OPT_BLOCK64 are not offered.
 */
int psa_rk4_sweep_waves_f64(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                            int32_t save_every, const double *dbeta, const double *dbeta2, const double *gamma,
                            const double *alpha, const double *a0_re_im, uint32_t flags, double *a_end_re_im,
                            double *p_sig_end, double *p_sig_max, int64_t *first_bad_step, double *traj_or_null,
                            double *elapsed_ms_or_null, double *p_wave_end, double *p_wave_max);
int psa_rk4_sweep_waves_f32(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                            int32_t save_every, const float *dbeta, const float *dbeta2, const float *gamma,
                            const float *alpha, const float *a0_re_im, uint32_t flags, float *a_end_re_im,
                            float *p_sig_end, float *p_sig_max, int64_t *first_bad_step, float *traj_or_null,
                            double *elapsed_ms_or_null, float *p_wave_end, float *p_wave_max);
int psa_rk4_sweep_waves_f64_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                                int32_t save_every, const double *d_dbeta, const double *d_dbeta2,
                                const double *d_gamma, const double *d_alpha, const double *d_a0_soa, uint32_t flags,
                                double *d_a_end_soa, double *d_p_sig_end, double *d_p_sig_max,
                                int64_t *d_first_bad_step, double *d_traj_soa, double *d_p_wave_end_soa,
                                double *d_p_wave_max_soa);
int psa_rk4_sweep_waves_f32_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                                int32_t save_every, const float *d_dbeta, const float *d_dbeta2, const float *d_gamma,
                                const float *d_alpha, const float *d_a0_soa, uint32_t flags, float *d_a_end_soa,
                                float *d_p_sig_end, float *d_p_sig_max, int64_t *d_first_bad_step, float *d_traj_soa,
                                float *d_p_wave_end_soa, float *d_p_wave_max_soa);

/* ---- a chain of fibre spans with mid-stage transfers (copier - mid-stage - PSA) ----------------------------------
 * S = n_segments >= 1 spans, each ONE launch of the sweep kernel above on the layout the automatic selector picks, joined
 * on the device by a small epilogue kernel per span (no host synchronisation between spans).  Span s has
 *   n_steps[s], seg_len[s]   host arrays [S]: steps and length (n_steps[s] = int(round(L_s/dz_s)); every n_steps[s]
 *                            must be a multiple of save_every, else PSA_E_SAVE_EVERY)
 *   dbeta [S][N], dbeta2 [S][N] (n_waves == 6, else NULL)
 *   gamma, alpha  [S][N], or [S] with PSA_BCAST_GAMMA / PSA_BCAST_ALPHA
 * and between span s and s+1 the per-wave complex transfer T_s[j] (amplitude gain times e^{i phase}):
 *   transfer  [S-1][N][n_waves][2], or [S-1][n_waves][2] with PSA_BCAST_TRANSFER; NULL = identity
 * The FWM phase is the ACCUMULATED mismatch Theta(z) = sum_{k<s} dbeta_k L_k + dbeta_s zeta (zeta: the local coordinate).
 * The kernels integrate span s in the gauge B_sig = A_sig e^{+i Theta_s} (signal of pair k for 6 waves: its own Theta),
 * so a boundary is B' = T_s B with the signal(s) also multiplied by e^{+i dbeta_s L_s}; Theta is kept per point in float64.
 * Outputs, all in the physical (A) frame:
 *   a_end, p_sig_end     the last saved row of the last span
 *   p_sig_max            max over every saved row of every span (each span's z = 0 row is the post-transfer state)
 *   first_bad_step       cumulative step index (sum of the earlier spans' n_steps + the local index); first failure wins
 *   p_wave_end/_max      as psa_rk4_sweep_waves_* (both NULL, or both given and traj NULL)
 *   traj_or_null         [N][n_saved_total][n_waves][2], n_saved_total = sum_s (n_steps[s]/save_every + 1)
 * S == 1 is psa_rk4_sweep_* / psa_rk4_sweep_waves_* exactly (bit-identical outputs).  The host-buffer form sets
 * PSA_OPT_LOSSLESS for every span whose alpha is 0 (a broadcast 0, or, when S > 1, a per-point row that is 0 everywhere).
 * Argument errors reuse the codes above (n_segments < 1:
 * PSA_E_NSTEPS); a trajectory that does not fit the device gets PSA_E_TOO_LARGE before any allocation.
 */
int psa_rk4_chain_f64(int device, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                      const double *seg_len, int32_t save_every, const double *dbeta, const double *dbeta2,
                      const double *gamma, const double *alpha, const double *a0_re_im, const double *transfer_re_im,
                      uint32_t flags, double *a_end_re_im, double *p_sig_end, double *p_sig_max, int64_t *first_bad_step,
                      double *traj_or_null, double *elapsed_ms_or_null, double *p_wave_end, double *p_wave_max);
int psa_rk4_chain_f32(int device, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                      const double *seg_len, int32_t save_every, const float *dbeta, const float *dbeta2,
                      const float *gamma, const float *alpha, const float *a0_re_im, const float *transfer_re_im,
                      uint32_t flags, float *a_end_re_im, float *p_sig_end, float *p_sig_max, int64_t *first_bad_step,
                      float *traj_or_null, double *elapsed_ms_or_null, float *p_wave_end, float *p_wave_max);
/* _dev forms: SoA HBM buffers as psa_rk4_sweep_*_dev (a0 [2*n_waves][N | 1], a_end [2*n_waves][N], p_wave_* [n_waves][N],
 * traj [n_saved_total][n_waves][ld][2]); d_transfer_soa is [S-1][2*n_waves][N] (or [S-1][2*n_waves] with
 * PSA_BCAST_TRANSFER); n_steps / seg_len stay HOST arrays.  d_workspace: >= psa_rk4_chain_workspace_bytes(...) bytes of
 * device memory (may be NULL when S == 1).  Asynchronous on `stream`, no allocation: graph-capturable. */
int psa_rk4_chain_f64_dev(void *stream, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                          const double *seg_len, int32_t save_every, const double *d_dbeta, const double *d_dbeta2,
                          const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                          const double *d_transfer_soa, uint32_t flags, double *d_a_end_soa, double *d_p_sig_end,
                          double *d_p_sig_max, int64_t *d_first_bad_step, double *d_traj_soa, double *d_p_wave_end_soa,
                          double *d_p_wave_max_soa, void *d_workspace);
int psa_rk4_chain_f32_dev(void *stream, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                          const double *seg_len, int32_t save_every, const float *d_dbeta, const float *d_dbeta2,
                          const float *d_gamma, const float *d_alpha, const float *d_a0_soa, const float *d_transfer_soa,
                          uint32_t flags, float *d_a_end_soa, float *d_p_sig_end, float *d_p_sig_max,
                          int64_t *d_first_bad_step, float *d_traj_soa, float *d_p_wave_end_soa, float *d_p_wave_max_soa,
                          void *d_workspace);
/* bytes of d_workspace for a chain (elem_size 4 | 8, wave_summary 0 | 1); -1 for invalid arguments */
int64_t psa_rk4_chain_workspace_bytes(int n_waves, int64_t n_points, int32_t elem_size, int wave_summary);

/* ---- B1': one RHS evaluation per point (host buffers, blocking) --------------------
 * Replaces yaman_model.rhs_yaman_simplified (yaman_model.py:10-52) for a batch:
 *   z [N], a_re_im [N][4][2], gamma/alpha/dbeta [N]  ->  out_re_im [N][4][2]
 * and, when non-NULL, the three terms of yaman_model.py:123-132 / :135-156 / :159-186.
 */
int psa_yaman_rhs_f64(int device, int64_t n_points, const double *z, const double *a_re_im,
                      const double *gamma, const double *alpha, const double *dbeta, double *out_re_im,
                      double *out_linear, double *out_kerr, double *out_fwm);

/* ---- gain summary over a finished sweep (host buffers, blocking) -------------------
 * Per-point reduction of scan_mismtach.py:376-389 / :723-734 and the argmax-over-sweep summary of the
 * (dead) scan_mismatch_seeded_signal (scan_mismtach.py:183-186), as one wavefront/block reduction:
 *   gain[i] = p_metric[i] / p0_sig  (linear) or 10*log10 of it (gain_db != 0);
 *             NaN if p_metric is not finite, gain <= 0, or first_bad_step[i] >= 0
 *   *best_index = argmax over finite gains (-1 if none), *best_gain its value, *n_finite their count.
 */
int psa_gain_summary_f64(int device, int64_t n_points, const double *p_metric, const int64_t *first_bad_step,
                         double p0_sig, int gain_db, double *gain_out, int64_t *best_index, double *best_gain,
                         int64_t *n_finite);

int psa_gain_summary_f64_dev(void *stream, int64_t n_points, const double *d_p_metric,
                             const int64_t *d_first_bad_step, double p0_sig, int gain_db, double *d_gain_out,
                             int64_t *d_best_index, double *d_best_gain, int64_t *d_n_finite,
                             void *d_workspace /* >= psa_gain_summary_workspace_bytes(n_points) */);
int64_t psa_gain_summary_workspace_bytes(int64_t n_points);

/* float32 sweeps (psa_rk4_sweep_f32): p_metric and the per-point gain are float, the ratio p/p0 and log10 are formed in
 * float64; best_gain stays double. */
int psa_gain_summary_f32(int device, int64_t n_points, const float *p_metric, const int64_t *first_bad_step,
                         double p0_sig, int gain_db, float *gain_out, int64_t *best_index, double *best_gain,
                         int64_t *n_finite);
int psa_gain_summary_f32_dev(void *stream, int64_t n_points, const float *d_p_metric, const int64_t *d_first_bad_step,
                             double p0_sig, int gain_db, float *d_gain_out, int64_t *d_best_index, double *d_best_gain,
                             int64_t *d_n_finite, void *d_workspace);

/* ---- the phase mismatch of a whole grid, produced on the device ------------------------------------------------
 * A multi-GPU shard generates its own dbeta slice from the grid definition instead of receiving it:
 * point i of the flattened grid lambda_p2[n2] x lambda_signal[n3] (row-major: i2 = i / n3, i3 = i % n3) gets
 *   w_j = two_pi_c / lambda_j,  w4 = (w1 + w2) - w3                     frequency_plan.plan_from_wavelengths  :291-327
 *   method PSA_DBETA_SYMMETRIC_EVEN: omega_c, omega_d, Omega as frequency_plan.infer_symmetry_from_omegas :215-255, then
 *       dbeta = sum over even_orders of beta_n (Omega^n - omega_d^n) 2/n!   dispersion.delta_beta_symmetric  :321-372
 *   method PSA_DBETA_GENERAL_TAYLOR: (beta(w3) + beta(w4)) - (beta(w1) + beta(w2)), beta(w) = sum_{n <= max_order}
 *       beta_n (w - omega_ref)^n / n!                                        dispersion.delta_beta_from_omegas :282-318
 * and dbeta = NaN (valid = 0) wherever the reference would raise for that point (wavelength <= 0, w4 <= 0, energy
 * conservation beyond atol/rtol, inconsistent symmetric plan, non-finite result) -- what its sweep drivers turn into a
 * NaN gain (scan_mismtach.py:391-392).  float64 arithmetic in the reference's operation order; the _f32 variants round
 * the float64 result to float.
 *   beta[n_beta]   beta_0 .. beta_{n_beta-1} per length unit (host pointer, n_beta <= 9; DispersionParams.get_beta_n)
 *   two_pi_c       the caller's 2*pi*c (constants.c), passed so host and device divide the same double
 *   lambda axes    device pointers (_dev) or host pointers (blocking variant); [first_index, first_index + n_points)
 *                  is the caller's block of the flattened grid.
 */
#define PSA_DBETA_SYMMETRIC_EVEN 0
#define PSA_DBETA_GENERAL_TAYLOR 1
int psa_dbeta_grid_f64_dev(void *stream, int method, const int32_t *even_orders, int n_even_orders, int max_order,
                           const double *beta, int n_beta, double omega_ref, double two_pi_c, double atol, double rtol,
                           double lambda1_m, const double *d_lambda2_axis, int64_t n2, const double *d_lambda3_axis,
                           int64_t n3, int64_t first_index, int64_t n_points, double *d_dbeta, uint8_t *d_valid_or_null);
int psa_dbeta_grid_f32_dev(void *stream, int method, const int32_t *even_orders, int n_even_orders, int max_order,
                           const double *beta, int n_beta, double omega_ref, double two_pi_c, double atol, double rtol,
                           double lambda1_m, const double *d_lambda2_axis, int64_t n2, const double *d_lambda3_axis,
                           int64_t n3, int64_t first_index, int64_t n_points, float *d_dbeta, uint8_t *d_valid_or_null);
int psa_dbeta_grid_f64(int device, int method, const int32_t *even_orders, int n_even_orders, int max_order,
                       const double *beta, int n_beta, double omega_ref, double two_pi_c, double atol, double rtol,
                       double lambda1_m, const double *lambda2_axis, int64_t n2, const double *lambda3_axis, int64_t n3,
                       int64_t first_index, int64_t n_points, double *dbeta, uint8_t *valid_or_null);

/* Six-wave grid (build-defined, scan_six_wave_grid): pair k sits at omega_c +- Omega_k and has
 * dbeta_k = delta_beta_symmetric(omega_d, Omega_k); point i of the flattened Omega1[n1] x Omega2[n2] grid gets
 * (dbeta1, dbeta2) = (dbeta(Omega1[i / n2]), dbeta(Omega2[i % n2])). */
int psa_dbeta_pairs_f64_dev(void *stream, const int32_t *even_orders, int n_even_orders, const double *beta, int n_beta,
                            double omega_d, const double *d_Omega1_axis, int64_t n1, const double *d_Omega2_axis,
                            int64_t n2, int64_t first_index, int64_t n_points, double *d_dbeta1, double *d_dbeta2);
int psa_dbeta_pairs_f32_dev(void *stream, const int32_t *even_orders, int n_even_orders, const double *beta, int n_beta,
                            double omega_d, const double *d_Omega1_axis, int64_t n1, const double *d_Omega2_axis,
                            int64_t n2, int64_t first_index, int64_t n_points, float *d_dbeta1, float *d_dbeta2);
int psa_dbeta_pairs_f64(int device, const int32_t *even_orders, int n_even_orders, const double *beta, int n_beta,
                        double omega_d, const double *Omega1_axis, int64_t n1, const double *Omega2_axis, int64_t n2,
                        int64_t first_index, int64_t n_points, double *dbeta1, double *dbeta2);

/* ---- the adaptive sweep: embedded Dormand-Prince 5(4) with per-point step-size control ------------------------
 * The same N independent propagations as psa_rk4_sweep_f64, integrated to a tolerance instead of on a fixed grid:
 * scipy.integrate.RK45 (scipy 1.15) step for step on the complex state A[n_waves], one sweep point per lane, each point
 * with its own step size and step count.  float64 only, 4 and 6 waves.
 *   rtol, atol   error norm = RMS over the n_waves complex components of err_j / (atol + rtol * max(|y_j|, |y_new_j|))
 *   h_max        cap of every step (INFINITY: none)
 *   first_step   0: scipy's select_initial_step (two RHS evaluations); otherwise the first step.  Unlike scipy, which
 *                raises for first_step > z_max, a larger value is accepted and behaves as first_step = z_max (the
 *                first step's end is clamped onto z_max, and the next step grows from that step)
 *   max_steps    attempts (accepted + rejected) per point; the hard bound of every lane's loop
 *   n_out        dense-output rows at z_k = k * (z_max / n_out), k = 0..n_out (np.linspace(0, z_max, n_out + 1)), from
 *                RK45's quartic interpolant; row 0 is a0; rows past z_end are NaN.  Only with traj_or_null.
 *   flags        PSA_BCAST_GAMMA / ALPHA / A0 and PSA_OPT_LOSSLESS (set automatically for a broadcast alpha == 0 by the
 *                host form); anything else is PSA_E_FLAGS
 * Per point:
 *   a_end_re_im [N][n_waves][2]  the state at z_end;  p_sig_end [N]  |A_sig|^2 there
 *   p_sig_max   [N]  max of |A_sig|^2 over z = 0 and every accepted step end (NaN-propagating)
 *   status      [N]  0 reached z_max; 1 the step fell below 10 * ulp(z) (a non-finite state ends here; a non-finite a0
 *                    at z = 0 with no step); 2 max_steps attempts used up
 *   z_end       [N]  the z reached (z_max when status == 0);  n_accepted / n_rejected [N]  attempts of each kind
 *   traj_or_null [N][n_out + 1][n_waves][2]  the dense-output rows, or NULL; subject to the trajectory limits
 * The other argument rules and error codes are those of psa_rk4_sweep_f64.
 */
int psa_rk45_sweep_f64(int device, int n_waves, int64_t n_points, double z_max, double rtol, double atol, double h_max,
                       double first_step, int64_t max_steps, int64_t n_out, const double *dbeta, const double *dbeta2,
                       const double *gamma, const double *alpha, const double *a0_re_im, uint32_t flags,
                       double *a_end_re_im, double *p_sig_end, double *p_sig_max, int32_t *status, double *z_end,
                       int64_t *n_accepted, int64_t *n_rejected, double *traj_or_null, double *elapsed_ms_or_null);
/* On device buffers, asynchronous on `stream`, no allocation (graph-capturable): SoA as psa_rk4_sweep_f64_dev;
 * d_traj_soa [n_out + 1][n_waves][N][2] or NULL. */
int psa_rk45_sweep_f64_dev(void *stream, int n_waves, int64_t n_points, double z_max, double rtol, double atol,
                           double h_max, double first_step, int64_t max_steps, int64_t n_out, const double *d_dbeta,
                           const double *d_dbeta2, const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                           uint32_t flags, double *d_a_end_soa, double *d_p_sig_end, double *d_p_sig_max,
                           int32_t *d_status, double *d_z_end, int64_t *d_n_accepted, int64_t *d_n_rejected,
                           double *d_traj_soa);

/* ---- the multi-channel sweep: two pumps and K = n_pairs signal/idler pairs (1 <= K <= PSA_MAX_PAIRS) ---------------
 * Build-defined like the 6-wave model, which it extends: waves [p1, p2, s_1, i_1, ..., s_K, i_K],
 * NW = 2 + 2K, pair k with its own mismatch dbeta_k.  With P_j = |A_j|^2, S = sum_j P_j, E_k(z) = 2 gamma exp(i dbeta_k z):
 *   dA_p1/dz = (-alpha/2 + i gamma (2S - P_p1)) A_p1 + i conj(A_p2) sum_k E_k A_sk A_ik        (p2: p1 <-> p2)
 *   dA_sk/dz = (-alpha/2 + i gamma (2S - P_sk)) A_sk + i conj(A_ik) conj(E_k) A_p1 A_p2        (ik: sk <-> ik)
 * K = 1 is the reference's system (yaman_model.py:123-186), K = 2 the 6-wave model of psa_rk4_sweep_f64.  The channels
 * couple through pump depletion and SPM/XPM only: FWM products between channels (signal-signal mixing) are NOT modelled
 * here, where the detunings are arbitrary; on a uniform frequency grid psa_rk4_comb_f64 below models every one of them.
 * Classic fixed-step RK4 on z_i = i * z_max / n_steps with the save and NaN semantics of psa_rk4_sweep_f64; float64 only.
 * One lane per pair, L = the power of two >= K (at least 2) lanes per point: K = 5 pays for 8 lanes.
 *   dbeta       [N][n_pairs]            mismatch of every pair, 1/length
 *   gamma, alpha  [N] | [1]
 *   a0_re_im    [N][NW][2] | [1][NW][2]
 *   a_end_re_im [N][NW][2]   state at the last saved row
 *   p_wave_end  [N][NW]      |A_j|^2 at that row
 *   p_wave_max  [N][NW]      max of |A_j|^2 over the saved rows incl. z = 0, NaN-propagating like np.max
 *   first_bad_step [N]       as psa_rk4_sweep_f64 (PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP)
 * All four outputs are always written.  flags: PSA_BCAST_GAMMA / ALPHA / A0, PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP,
 * PSA_OPT_LOSSLESS (set by the host form itself for a broadcast alpha == 0) and PSA_OPT_BLOCK64; anything else (a layout,
 * float32 or LDS flag) is PSA_E_FLAGS.  n_pairs outside 1..PSA_MAX_PAIRS: PSA_E_NPAIRS; L * n_points beyond the launch
 * grid (2 * PSA_MAX_POINTS lanes): PSA_E_TOO_LARGE; the other codes as psa_rk4_sweep_f64.  All of it is checked before
 * any device call; n_points == 0 is a successful no-op.  Saved rows and chains of spans are psa_rk4_pairs_chain_f64 below
 * (one span with a trajectory is this sweep's trajectory form); there is no adaptive form.
 */
int psa_rk4_sweep_pairs_f64(int device, int n_pairs, int64_t n_points, int64_t n_steps, double z_max,
                            int32_t save_every, const double *dbeta, const double *gamma, const double *alpha,
                            const double *a0_re_im, uint32_t flags, double *a_end_re_im, double *p_wave_end,
                            double *p_wave_max, int64_t *first_bad_step, double *elapsed_ms_or_null);
/* On device buffers, asynchronous on `stream`, no allocation and no synchronisation: d_dbeta_soa [n_pairs][N],
 * d_a0_soa [2*NW][N | 1], d_a_end_soa [2*NW][N], d_p_wave_end_soa / d_p_wave_max_soa [NW][N], d_first_bad_step [N]. */
int psa_rk4_sweep_pairs_f64_dev(void *stream, int n_pairs, int64_t n_points, int64_t n_steps, double z_max,
                                int32_t save_every, const double *d_dbeta_soa, const double *d_gamma,
                                const double *d_alpha, const double *d_a0_soa, uint32_t flags, double *d_a_end_soa,
                                double *d_p_wave_end_soa, double *d_p_wave_max_soa, int64_t *d_first_bad_step);

/* ---- the single-pump (degenerate) sweep: one pump, a signal and an idler at w_i = 2 w_p - w_s ----------------------------
 * Build-defined, no reference counterpart: waves [p, s, i], NW = 3.  With P_j = |A_j|^2,
 * S = P_p + P_s + P_i, E(z) = 2 gamma exp(i dbeta z), dbeta = beta(w_s) + beta(w_i) - 2 beta(w_p):
 *   dA_p/dz = (-alpha/2 + i gamma (2S - P_p)) A_p + i conj(A_p) E A_s A_i
 *   dA_s/dz = (-alpha/2 + i gamma (2S - P_s)) A_s + i conj(A_i) (conj(E)/2) A_p^2              (i: s <-> i)
 * This is not psa_rk4_sweep_f64 with A1 == A2: there the pump's self-phase term is 1.5 gamma |A_p|^2 (A_p = sqrt(2) A1), so
 * the phase matching is off by gamma P_p / 2.  For alpha = 0 the model conserves P_p + P_s + P_i, P_s - P_i and P_p + 2 P_s.
 * Classic fixed-step RK4 on z_i = i * z_max / n_steps with the save and NaN semantics of psa_rk4_sweep_f64; float64 with
 * one sweep point per lane (the float32 forms follow below).
 *   dbeta       [N]                     mismatch per point, 1/length
 *   gamma, alpha  [N] | [1]
 *   a0_re_im    [N][3][2] | [1][3][2]
 *   a_end_re_im [N][3][2]   state at the last saved row
 *   p_wave_end  [N][3]      |A_j|^2 at that row
 *   p_wave_max  [N][3]      max of |A_j|^2 over the saved rows incl. z = 0, NaN-propagating like np.max
 *   first_bad_step [N]      as psa_rk4_sweep_f64 (PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP)
 *   traj_or_null [N][n_saved][3][2]  every saved row, or NULL
 * The four summary outputs are always written.  flags: PSA_BCAST_GAMMA / ALPHA / A0, PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP,
 * PSA_OPT_LOSSLESS (set by the host form itself for a broadcast alpha == 0), PSA_OPT_BLOCK64 and, on the `_dev` form only,
 * PSA_OPT_TRAJ_LD; anything else is PSA_E_FLAGS.  n_points above PSA_MAX_POINTS, a trajectory whose leading dimension ld
 * (n_points, or psa_traj_ld(n_points, 8)) has ld * 16 >= 2^32 (rows are addressed with a 32-bit lane offset) or that does not
 * fit the device's free memory: PSA_E_TOO_LARGE; the other codes as psa_rk4_sweep_f64.  All of it is checked before any
 * device call, in the order of psa_rk4_sweep_f64; n_points == 0 is a successful no-op.
 */
int psa_rk4_single_pump_f64(int device, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                            const double *dbeta, const double *gamma, const double *alpha, const double *a0_re_im,
                            uint32_t flags, double *a_end_re_im, double *p_wave_end, double *p_wave_max,
                            int64_t *first_bad_step, double *traj_or_null, double *elapsed_ms_or_null);
/* On device buffers, asynchronous on `stream`, no allocation and no synchronisation: d_dbeta [N], d_a0_soa [6][N | 1],
 * d_a_end_soa [6][N], d_p_wave_end_soa / d_p_wave_max_soa [3][N], d_first_bad_step [N], d_traj_soa_or_null
 * [n_saved][3][ld][2] with ld = N, or psa_traj_ld(N, 8) with PSA_OPT_TRAJ_LD. */
int psa_rk4_single_pump_f64_dev(void *stream, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                                const double *d_dbeta, const double *d_gamma, const double *d_alpha,
                                const double *d_a0_soa, uint32_t flags, double *d_a_end_soa, double *d_p_wave_end_soa,
                                double *d_p_wave_max_soa, int64_t *d_first_bad_step, double *d_traj_soa_or_null);
/* The same sweep in float32: every buffer float, z_max and elapsed_ms double, first_bad_step int64.  Two sweep
 * points per lane in packed math (points 2i and 2i+1 share lane i; any N, N = 1 included); classic RK4 on the un-fused
 * right-hand side with a compensated state, the phase factor re-seeded from a float64-reduced phase every 16 steps.  It is
 * the one float32 layout of this model: PSA_OPT_F32_SCALAR and PSA_OPT_F32_PACKED are PSA_E_FLAGS like every other layout
 * flag, the accepted flags are those of the _f64 forms, and PSA_OPT_LOSSLESS is a promise that selects no other kernel.
 * PSA_OPT_EXACT_STEP tests after every step; without it first_bad_step names the last step of the failing save block.  A
 * trajectory whose leading dimension ld (n_points, or psa_traj_ld(n_points, 4)) has ld * 8 >= 2^31 is PSA_E_TOO_LARGE, the
 * bound of psa_rk4_sweep_f32; every other rule, code and their order are those of psa_rk4_single_pump_f64. */
int psa_rk4_single_pump_f32(int device, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                            const float *dbeta, const float *gamma, const float *alpha, const float *a0_re_im,
                            uint32_t flags, float *a_end_re_im, float *p_wave_end, float *p_wave_max,
                            int64_t *first_bad_step, float *traj_or_null, double *elapsed_ms_or_null);
/* d_traj_soa_or_null [n_saved][3][ld][2] with ld = N, or psa_traj_ld(N, 4) with PSA_OPT_TRAJ_LD. */
int psa_rk4_single_pump_f32_dev(void *stream, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                                const float *d_dbeta, const float *d_gamma, const float *d_alpha,
                                const float *d_a0_soa, uint32_t flags, float *d_a_end_soa, float *d_p_wave_end_soa,
                                float *d_p_wave_max_soa, int64_t *d_first_bad_step, float *d_traj_soa_or_null);

/* ---- the multi-line ("frequency comb") sweep: M = n_lines equally spaced lines and EVERY FWM product among them ----------
 * Build-defined, no reference counterpart: lines m = 0..M-1 at w_0 + m dw, ascending in frequency,
 * 3 <= M <= PSA_MAX_LINES, the field of line m being A_m e^{i kappa_m z}.  With u_m(z) = exp(i kappa_m z), B_m = A_m u_m,
 *   C_d = sum_n B_{n+d} conj(B_n)      (both indices inside 0..M-1; C_{-d} = conj(C_d), C_0 = sum |B|^2)
 *   S_m = sum_l B_l C_{m-l}            (= sum over every ordered triple k + l - n = m of B_k B_l conj(B_n))
 *   dA_m/dz = -alpha/2 A_m + i gamma conj(u_m) S_m
 * S_m holds SPM/XPM ((2 sum_j P_j - P_m) B_m), pump-pump, pump-signal and signal-signal mixing; products that fall outside
 * the grid are dropped.  kappa_m is the line's propagation constant in any gauge: kappa_m + a + b m is the same system, only
 * kappa_k + kappa_l - kappa_n - kappa_m ever acts.  For alpha = 0 the model conserves sum P_m and sum m P_m.  M = 3 is
 * psa_rk4_single_pump_f64 with lines [0, 1, 2] = waves [s, p, i] and kappa_0 + kappa_2 - 2 kappa_1 = dbeta.
 * Classic fixed-step RK4 on z_i = i * z_max / n_steps with the save semantics of psa_rk4_sweep_f64; float64, one sweep
 * point per lane.
 *   kappa       [N][M]                  propagation constant of every line, 1/length
 *   gamma, alpha  [N] | [1]
 *   a0_re_im    [N][M][2] | [1][M][2]
 *   a_end_re_im [N][M][2]   state at the last saved row
 *   p_wave_end  [N][M]      |A_m|^2 at that row
 *   p_wave_max  [N][M]      max of |A_m|^2 over the saved rows incl. z = 0, NaN-propagating like np.max
 *   first_bad_step [N]      with PSA_OPT_CHECK_NAN the EXACT index of the first step that left the point non-finite (the
 *                           point is tested after every step; PSA_OPT_EXACT_STEP is accepted and changes nothing), else -1
 *   traj_or_null [N][n_saved][M][2]  every saved row, or NULL
 * The four summary outputs are always written.  flags: PSA_BCAST_GAMMA / ALPHA / A0, PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP,
 * PSA_OPT_LOSSLESS (set by the host form itself for a broadcast alpha == 0), PSA_OPT_BLOCK64 and, on the `_dev` form only,
 * PSA_OPT_TRAJ_LD; anything else (a layout, float32 or LDS flag) is PSA_E_FLAGS.  n_lines outside 3..PSA_MAX_LINES:
 * PSA_E_NLINES, checked first; then the rules, codes and order of psa_rk4_single_pump_f64 with M in place of 3 (a trajectory
 * whose leading dimension ld has ld * 16 >= 2^32, or that does not fit the device's free memory: PSA_E_TOO_LARGE).  All of it
 * is checked before any device call; n_points == 0 is a successful no-op.  Chains of spans are psa_rk4_comb_chain_f64 below
 * (float64 only); psa_rk4_comb_f32 is the float32 form; there is no adaptive form.
 */
int psa_rk4_comb_f64(int device, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                     const double *kappa, const double *gamma, const double *alpha, const double *a0_re_im,
                     uint32_t flags, double *a_end_re_im, double *p_wave_end, double *p_wave_max,
                     int64_t *first_bad_step, double *traj_or_null, double *elapsed_ms_or_null);
/* On device buffers, asynchronous on `stream`, no allocation and no synchronisation: d_kappa_soa [M][N], d_a0_soa
 * [2M][N | 1], d_a_end_soa [2M][N], d_p_wave_end_soa / d_p_wave_max_soa [M][N], d_first_bad_step [N], d_traj_soa_or_null
 * [n_saved][M][ld][2] with ld = N, or psa_traj_ld(N, 8) with PSA_OPT_TRAJ_LD. */
int psa_rk4_comb_f64_dev(void *stream, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                         const double *d_kappa_soa, const double *d_gamma, const double *d_alpha,
                         const double *d_a0_soa, uint32_t flags, double *d_a_end_soa, double *d_p_wave_end_soa,
                         double *d_p_wave_max_soa, int64_t *d_first_bad_step, double *d_traj_soa_or_null);
/* The same sweep in float32: every buffer float, z_max and elapsed_ms double, first_bad_step int64.  Two sweep
 * points per lane in packed math (points 2i and 2i+1 share lane i; any N, N = 1 included), every M = 3..PSA_MAX_LINES; classic
 * RK4 on the un-fused right-hand side with a compensated state, u_m re-seeded from a float64-reduced phase every 16 steps
 * (kappa is widened to double there, z is formed in double).  It is the one float32 layout of this model: PSA_OPT_F32_SCALAR
 * and PSA_OPT_F32_PACKED are PSA_E_FLAGS like every other layout flag, the accepted flags are those of the _f64 forms, and
 * PSA_OPT_LOSSLESS is a promise that selects no other kernel.  With PSA_OPT_CHECK_NAN first_bad_step is exact per point, as in
 * float64.  A trajectory whose leading dimension ld (n_points, or psa_traj_ld(n_points, 4)) has ld * 8 >= 2^31 is
 * PSA_E_TOO_LARGE, the bound of psa_rk4_sweep_f32; every other rule, code and their order are those of psa_rk4_comb_f64.
 * Float32 pays from sweeps that fill the chip with two points per lane (DESIGN.md 3.3f has the measured rates per M). */
int psa_rk4_comb_f32(int device, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                     const float *kappa, const float *gamma, const float *alpha, const float *a0_re_im,
                     uint32_t flags, float *a_end_re_im, float *p_wave_end, float *p_wave_max,
                     int64_t *first_bad_step, float *traj_or_null, double *elapsed_ms_or_null);
/* d_traj_soa_or_null [n_saved][M][ld][2] with ld = N, or psa_traj_ld(N, 4) with PSA_OPT_TRAJ_LD. */
int psa_rk4_comb_f32_dev(void *stream, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                         const float *d_kappa_soa, const float *d_gamma, const float *d_alpha,
                         const float *d_a0_soa, uint32_t flags, float *d_a_end_soa, float *d_p_wave_end_soa,
                         float *d_p_wave_max_soa, int64_t *d_first_bad_step, float *d_traj_soa_or_null);

/* ---- a chain of single-pump spans with mid-stage transfers (copier - mid-stage - PSA on one pump) ------------------------
 * psa_rk4_chain_* for the three-wave model above: S = n_segments >= 1 spans, each ONE launch of the
 * unchanged single-pump kernel, joined on the device by the chain's epilogue kernel (no host synchronisation between spans).
 * The kernel assumes nothing about which wave is strong, so the same entry point is the signal-degenerate dual-pump PSA
 * with the roles relabelled: the degenerate signal in slot 0, the two pumps in slots 1 and 2, dbeta = beta_1 + beta_2 -
 * 2 beta_s.  Span s has
 *   n_steps[s], seg_len[s]   host arrays [S]; each n_steps[s] in [1, 2^31) and a multiple of save_every (else
 *                            PSA_E_SAVE_EVERY), each seg_len[s] positive and finite
 *   dbeta [S][N];  gamma, alpha  [S][N], or [S] with PSA_BCAST_GAMMA / PSA_BCAST_ALPHA
 *   a0_re_im  [N][3][2] | [1][3][2] (PSA_BCAST_A0)
 * and between span s and s+1 the per-wave complex transfer T_s[j] (amplitude gain times e^{i phase}):
 *   transfer_re_im  [S-1][N][3][2], or [S-1][3][2] with PSA_BCAST_TRANSFER; NULL = identity
 * Gauge.  The physical FWM factor is e^{+-i Theta(z)}, Theta = Theta_s + dbeta_s zeta, Theta_s = sum_{k<s} dbeta_k L_k (zeta:
 * the span's local coordinate).  With B_s = A_s e^{+i Theta_s} for the signal (wave 1) and B = A for the pump and the idler,
 * all three equations hold in B with the plain factor e^{+-i dbeta_s zeta} (the Kerr terms are phase-blind): the kernel runs
 * each span unchanged, a boundary is B' = T_s B with the signal also multiplied by e^{+i dbeta_s L_s}, and reported
 * amplitudes and rows are rotated back by e^{-i Theta_s} on wave 1.  Theta is kept per point in float64.
 * Outputs, all in the physical (A) frame:
 *   a_end_re_im [N][3][2], p_wave_end [N][3]   the last saved row of the last span
 *   p_wave_max  [N][3]    max over every saved row of every span (each span's z = 0 row is the post-transfer state),
 *                         NaN-propagating
 *   first_bad_step [N]    cumulative step index (the earlier spans' n_steps + the local index); the first failure wins
 *   traj_or_null  [N][rows_total][3][2], rows_total = sum_s (n_steps[s]/save_every + 1); the host form pads the device
 *                 buffer itself and brings it home in the sweep's chunks
 * S == 1 is psa_rk4_single_pump_f64(_dev) itself, bit for bit: no workspace, no epilogue.  The host form sets
 * PSA_OPT_LOSSLESS per span: for a broadcast alpha of 0, or (S > 1) a per-point row that is 0 everywhere.
 * flags: the four PSA_BCAST_* bits, PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP, PSA_OPT_LOSSLESS, PSA_OPT_BLOCK64 and, on the
 * `_dev` form only, PSA_OPT_TRAJ_LD; anything else is PSA_E_FLAGS.  Every rule is checked before any device call, in the
 * order n_segments < 1 (PSA_E_NSTEPS), n_steps / seg_len NULL, the single-pump rules on the first span's grid (n_points,
 * n_steps, seg_len, save_every, flags, pointers, a trajectory's ld * 16 < 2^32 else PSA_E_TOO_LARGE), then every span's
 * n_steps, seg_len and save_every multiple; a trajectory that does not fit the device is PSA_E_TOO_LARGE (host form).
 * n_points == 0 is a successful no-op.  No new error code.
 */
int psa_rk4_single_pump_chain_f64(int device, int64_t n_points, int n_segments, const int64_t *n_steps,
                                  const double *seg_len, int32_t save_every, const double *dbeta, const double *gamma,
                                  const double *alpha, const double *a0_re_im, const double *transfer_re_im, uint32_t flags,
                                  double *a_end_re_im, double *p_wave_end, double *p_wave_max, int64_t *first_bad_step,
                                  double *traj_or_null, double *elapsed_ms_or_null);
/* On SoA device buffers, asynchronous on `stream`, no allocation and no synchronisation: d_dbeta [S][N], d_gamma / d_alpha
 * [S][N] | [S], d_a0_soa [6][N | 1], d_transfer_soa [S-1][6][N] (or [S-1][6] with PSA_BCAST_TRANSFER), d_a_end_soa [6][N],
 * d_p_wave_end_soa / d_p_wave_max_soa [3][N], d_first_bad_step [N], d_traj_soa_or_null [rows_total][3][ld][2] with ld = N, or
 * psa_traj_ld(N, 8) with PSA_OPT_TRAJ_LD; n_steps / seg_len stay HOST arrays.  d_workspace: at least
 * psa_rk4_single_pump_chain_workspace_bytes(n_points) bytes of device memory; NULL with S > 1 is PSA_E_NULLPTR, S == 1 needs
 * none.  `_dev` callers pass PSA_OPT_LOSSLESS for the whole chain. */
int psa_rk4_single_pump_chain_f64_dev(void *stream, int64_t n_points, int n_segments, const int64_t *n_steps,
                                      const double *seg_len, int32_t save_every, const double *d_dbeta,
                                      const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                                      const double *d_transfer_soa, uint32_t flags, double *d_a_end_soa,
                                      double *d_p_wave_end_soa, double *d_p_wave_max_soa, int64_t *d_first_bad_step,
                                      double *d_traj_soa_or_null, void *d_workspace);
/* bytes of d_workspace for a single-pump chain; -1 for n_points < 0 */
int64_t psa_rk4_single_pump_chain_workspace_bytes(int64_t n_points);

/* ---- a chain of multi-channel spans with mid-stage transfers (the WDM copier - mid-stage - PSA link) ----------------------
 * psa_rk4_single_pump_chain_f64 for the multi-channel model above: S = n_segments >= 1 spans of two pumps
 * and K = n_pairs signal/idler pairs, NW = 2 + 2K, each span ONE launch of the multi-channel kernel, joined on the device by
 * the chain's epilogue kernel (no host synchronisation between spans).  Span s has
 *   n_steps[s], seg_len[s]   host arrays [S]; each n_steps[s] in [1, 2^31) and a multiple of save_every (else
 *                            PSA_E_SAVE_EVERY), each seg_len[s] positive and finite
 *   dbeta [S][N][K];  gamma, alpha  [S][N], or [S] with PSA_BCAST_GAMMA / PSA_BCAST_ALPHA
 *   a0_re_im  [N][NW][2] | [1][NW][2] (PSA_BCAST_A0)
 * and between span s and s+1 the per-wave complex transfer T_s[j] (amplitude gain times e^{i phase}):
 *   transfer_re_im  [S-1][N][NW][2], or [S-1][NW][2] with PSA_BCAST_TRANSFER; NULL = identity
 * Gauge.  Pair k's physical FWM factor is e^{+-i Theta_k(z)}, Theta_k = Theta_{s,k} + dbeta_{s,k} zeta, Theta_{s,k} =
 * sum_{j<s} dbeta_{j,k} L_j.  With B_sk = A_sk e^{+i Theta_{s,k}} for the signal of every pair (wave 2 + 2k) and B = A for the
 * pumps and the idlers, every equation holds in B with the plain factor e^{+-i dbeta_{s,k} zeta}: in the pumps' sum over the
 * pairs each pair's phase cancels in its own term, and the Kerr terms are phase-blind.  The kernel runs each span unchanged,
 * a boundary is B' = T_s B with signal k also multiplied by e^{+i dbeta_{s,k} L_s}, and reported amplitudes and rows are
 * rotated back by e^{-i Theta_{s,k}} on wave 2 + 2k.  Theta is kept per point and pair in float64.
 * Outputs, all in the physical (A) frame:
 *   a_end_re_im [N][NW][2], p_wave_end [N][NW]   the last saved row of the last span
 *   p_wave_max  [N][NW]   max over every saved row of every span (each span's z = 0 row is the post-transfer state),
 *                         NaN-propagating
 *   first_bad_step [N]    cumulative step index (the earlier spans' n_steps + the local index); the first failure wins
 *   traj_or_null  [N][rows_total][NW][2], rows_total = sum_s (n_steps[s]/save_every + 1); the host form pads the device
 *                 buffer itself and brings it home in the sweep's chunks
 * S == 1 without a trajectory is psa_rk4_sweep_pairs_f64(_dev) itself, bit for bit: no workspace, no epilogue; S == 1 with
 * one is that sweep's trajectory form, its summaries the same bits.
 * One deliberate difference from psa_rk4_single_pump_chain_f64: a chain of ONE span keeps the sweep's rule for save_every,
 * not the chain's.  n_steps[0] need not be a multiple of save_every; a_end is the last saved row and the trajectory has
 * n_steps[0] / save_every + 1 rows, as for psa_rk4_sweep_pairs_f64.  With S > 1 every span's n_steps must be a multiple.
 * The host form sets PSA_OPT_LOSSLESS per span: for a broadcast alpha of 0, or (S > 1) a per-point row that is 0 everywhere.
 * flags: the four PSA_BCAST_* bits, PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP, PSA_OPT_LOSSLESS, PSA_OPT_BLOCK64 (rows are
 * written by 256-thread workgroups whatever it says) and, on the `_dev` form only, PSA_OPT_TRAJ_LD; anything else is
 * PSA_E_FLAGS.  Every rule is checked before any device call, in the order n_segments < 1 (PSA_E_NSTEPS), n_steps / seg_len
 * NULL, the multi-channel rules on the first span's grid (n_pairs: PSA_E_NPAIRS; n_points and the launch grid, n_steps,
 * seg_len, save_every, flags, pointers, a trajectory's ld * 16 < 2^32 else PSA_E_TOO_LARGE), then every span's n_steps,
 * seg_len and save_every multiple; a trajectory that does not fit the device is PSA_E_TOO_LARGE (host form).
 * n_points == 0 is a successful no-op.  No new error code.
 */
int psa_rk4_pairs_chain_f64(int device, int n_pairs, int64_t n_points, int n_segments, const int64_t *n_steps,
                            const double *seg_len, int32_t save_every, const double *dbeta, const double *gamma,
                            const double *alpha, const double *a0_re_im, const double *transfer_re_im, uint32_t flags,
                            double *a_end_re_im, double *p_wave_end, double *p_wave_max, int64_t *first_bad_step,
                            double *traj_or_null, double *elapsed_ms_or_null);
/* On SoA device buffers, asynchronous on `stream`, no allocation and no synchronisation: d_dbeta_soa [S][K][N], d_gamma /
 * d_alpha [S][N] | [S], d_a0_soa [2*NW][N | 1], d_transfer_soa [S-1][2*NW][N] (or [S-1][2*NW] with PSA_BCAST_TRANSFER),
 * d_a_end_soa [2*NW][N], d_p_wave_end_soa / d_p_wave_max_soa [NW][N], d_first_bad_step [N], d_traj_soa_or_null
 * [rows_total][NW][ld][2] with ld = N, or psa_traj_ld(N, 8) with PSA_OPT_TRAJ_LD; n_steps / seg_len stay HOST arrays.
 * d_workspace: at least psa_rk4_pairs_chain_workspace_bytes(n_pairs, n_points) bytes of device memory; NULL with S > 1 is
 * PSA_E_NULLPTR, S == 1 needs none.  `_dev` callers pass PSA_OPT_LOSSLESS for the whole chain. */
int psa_rk4_pairs_chain_f64_dev(void *stream, int n_pairs, int64_t n_points, int n_segments, const int64_t *n_steps,
                                const double *seg_len, int32_t save_every, const double *d_dbeta_soa,
                                const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                                const double *d_transfer_soa, uint32_t flags, double *d_a_end_soa,
                                double *d_p_wave_end_soa, double *d_p_wave_max_soa, int64_t *d_first_bad_step,
                                double *d_traj_soa_or_null, void *d_workspace);
/* bytes of d_workspace for a multi-channel chain; -1 for n_pairs outside 1..PSA_MAX_PAIRS or n_points < 0 */
int64_t psa_rk4_pairs_chain_workspace_bytes(int n_pairs, int64_t n_points);

/* ---- a chain of multi-line ("frequency comb") spans with mid-stage transfers (copier - mid-stage - PSA with every product) --
 * psa_rk4_single_pump_chain_f64 for the multi-line model above: S = n_segments >= 1 spans of M = n_lines
 * equally spaced lines, each span ONE launch of the unchanged multi-line kernel, joined on the device by the chain's epilogue
 * kernel (no host synchronisation between spans).  Span s has
 *   n_steps[s], seg_len[s]   host arrays [S]; each n_steps[s] in [1, 2^31) and a multiple of save_every (else
 *                            PSA_E_SAVE_EVERY), each seg_len[s] positive and finite
 *   kappa [S][N][M];  gamma, alpha  [S][N], or [S] with PSA_BCAST_GAMMA / PSA_BCAST_ALPHA
 *   a0_re_im  [N][M][2] | [1][M][2] (PSA_BCAST_A0)
 * and between span s and s+1 the per-line complex transfer T_s[m] (amplitude gain times e^{i phase}):
 *   transfer_re_im  [S-1][N][M][2], or [S-1][M][2] with PSA_BCAST_TRANSFER; NULL = identity
 * Gauge.  The field of line m is A_m e^{i Phi_m(z)}, Phi_m = Phi_{s,m} + kappa_{s,m} zeta on the span's local coordinate zeta,
 * Phi_{s,m} = sum_{j<s} kappa_{j,m} L_j.  With B_m = A_m e^{+i Phi_{s,m}} for EVERY line, A_m e^{i Phi_m} = B_m e^{i kappa_{s,m}
 * zeta}: the equations hold in B with the plain factors e^{+-i kappa_{s,m} zeta}, which is what the kernel integrates.  The kernel
 * runs each span unchanged, a boundary is B'_m = T_s[m] B_m e^{+i kappa_{s,m} L_s}, and reported amplitudes and rows are rotated
 * back by e^{-i Phi_{s,m}} on every line; powers need nothing.  Phi is kept per point and line in float64.  A span's kappa may
 * be given in any gauge kappa + a_s + b_s m (another one per span): only kappa_k + kappa_l - kappa_n - kappa_m acts on A, so
 * neither the powers nor the reported amplitudes depend on it.
 * Outputs, all in the physical (A) frame:
 *   a_end_re_im [N][M][2], p_wave_end [N][M]   the last saved row of the last span
 *   p_wave_max  [N][M]    max over every saved row of every span (each span's z = 0 row is the post-transfer state),
 *                         NaN-propagating
 *   first_bad_step [N]    cumulative step index (the earlier spans' n_steps + the local index); the first failure wins
 *   traj_or_null  [N][rows_total][M][2], rows_total = sum_s (n_steps[s]/save_every + 1); the host form pads the device
 *                 buffer itself and brings it home in the sweep's chunks
 * S == 1 is psa_rk4_comb_f64(_dev) itself, bit for bit: no workspace, no epilogue.  The host form sets PSA_OPT_LOSSLESS per
 * span: for a broadcast alpha of 0, or (S > 1) a per-point row that is 0 everywhere.
 * flags: the four PSA_BCAST_* bits, PSA_OPT_CHECK_NAN, PSA_OPT_EXACT_STEP, PSA_OPT_LOSSLESS, PSA_OPT_BLOCK64 and, on the
 * `_dev` form only, PSA_OPT_TRAJ_LD; anything else (a layout, float32 or LDS flag) is PSA_E_FLAGS.  Every rule is checked
 * before any device call, in the order n_segments < 1 (PSA_E_NSTEPS), n_steps / seg_len NULL, the multi-line rules on the
 * first span's grid (n_lines: PSA_E_NLINES, the first of them; n_points, n_steps, seg_len, save_every, flags, pointers, a
 * trajectory's ld * 16 < 2^32 else PSA_E_TOO_LARGE), then every span's n_steps, seg_len and save_every multiple; a trajectory
 * that does not fit the device is PSA_E_TOO_LARGE (host form).  n_points == 0 is a successful no-op.  No new error code.
 * There is no float32 or adaptive form.
 */
int psa_rk4_comb_chain_f64(int device, int n_lines, int64_t n_points, int n_segments, const int64_t *n_steps,
                           const double *seg_len, int32_t save_every, const double *kappa, const double *gamma,
                           const double *alpha, const double *a0_re_im, const double *transfer_re_im, uint32_t flags,
                           double *a_end_re_im, double *p_wave_end, double *p_wave_max, int64_t *first_bad_step,
                           double *traj_or_null, double *elapsed_ms_or_null);
/* On SoA device buffers, asynchronous on `stream`, no allocation and no synchronisation: d_kappa_soa [S][M][N], d_gamma /
 * d_alpha [S][N] | [S], d_a0_soa [2M][N | 1], d_transfer_soa [S-1][2M][N] (or [S-1][2M] with PSA_BCAST_TRANSFER),
 * d_a_end_soa [2M][N], d_p_wave_end_soa / d_p_wave_max_soa [M][N], d_first_bad_step [N], d_traj_soa_or_null
 * [rows_total][M][ld][2] with ld = N, or psa_traj_ld(N, 8) with PSA_OPT_TRAJ_LD; n_steps / seg_len stay HOST arrays.
 * d_workspace: at least psa_rk4_comb_chain_workspace_bytes(n_lines, n_points) bytes of device memory (Phi 8 M N, the span's
 * first_bad_step 8 N, the next a0 and the span's a_end 16 M N each, the span's two summaries 8 M N each, every slice rounded
 * up to 256 B); NULL with S > 1 is PSA_E_NULLPTR, S == 1 needs none.  `_dev` callers pass PSA_OPT_LOSSLESS for the whole
 * chain. */
int psa_rk4_comb_chain_f64_dev(void *stream, int n_lines, int64_t n_points, int n_segments, const int64_t *n_steps,
                               const double *seg_len, int32_t save_every, const double *d_kappa_soa,
                               const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                               const double *d_transfer_soa, uint32_t flags, double *d_a_end_soa,
                               double *d_p_wave_end_soa, double *d_p_wave_max_soa, int64_t *d_first_bad_step,
                               double *d_traj_soa_or_null, void *d_workspace);
/* bytes of d_workspace for a multi-line chain; -1 for n_lines outside 3..PSA_MAX_LINES or n_points < 0 */
int64_t psa_rk4_comb_chain_workspace_bytes(int n_lines, int64_t n_points);

#ifdef __cplusplus
}
#endif
#endif /* PSA_RK4_H */
