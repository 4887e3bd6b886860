// psa_capi.hip -- the extern "C" surface of libpsa_hip.so, fibre chains (psa_rk4_chain_*) included (see include/psa_rk4.h for the contract and the
// reference file:line each entry point replaces).  Host code only: argument validation, HBM staging for the
// host-buffer variants, launches.  No CPU compute path exists here on purpose: without a gfx950 device the
// host-buffer calls fail with PSA_E_DEVICE / a hipError_t -- they never fall back.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "psa_internal.h"
#include "psa_rk4.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    return (int)e;
}

#define HIP_RET(expr)                                                \
    do {                                                             \
        hipError_t _e = (expr);                                      \
        if (_e != hipSuccess) return hip_fail(_e, #expr);            \
    } while (0)

// Leading dimension of the trajectory buffer [n_saved][n_waves][ld][2].  The four (six) wave regions of a row, and
// consecutive rows, are ld * pair bytes apart; when that is a multiple of 2 MiB the streams of the resident waves collide in
// the memory system's address hash and the store rate drops (store-only probe, tools/hbm_write_peak: 5.7 / 5.6 / 4.9 TB/s at
// 262 144 / 524 288 / 1 048 576 points against 6.3 / 6.5 / 6.6 with the regions 4 352 B further apart; sizes that are not
// such multiples, and strides of 1 MiB or less, are best left alone: profiles/r03_store_layout_probe.log).
int64_t traj_ld_of(int64_t n_points, size_t elem_size) {
    const int64_t pair = 2 * (int64_t)elem_size;
    const int64_t bytes = n_points * pair;
    if (n_points <= 0 || bytes % (2ll << 20) != 0) return n_points;
    return n_points + 4352 / pair;          // 17 x 256 B: 272 float64 points, 544 float32 points
}

// ---- call records ------------------------------------------------------------------------------------------------------
// What one call of a sweep family asks for, fields in the order of its C arguments.  The extern "C" function builds the record
// once; validation, the `_dev` path and the host path take it by reference.  The host path copies it, has its layout function
// put device pointers (Staging) in place of the copy's buffer pointers and hands the copy to the same `_dev` function.  A new
// family with the wave summary (a_end, p_wave_end, p_wave_max, first_bad_step, optional rows) brings its record and its
// Family<> and is served by validate_wave, wave_dev, wave_host and the chain functions; a family with other outputs or rules
// (SweepCall, Rk45Call) brings its own validator, `_dev` function and layout on top of the shared rules (validate_grid,
// fill_shared_args, lossless_bit).
template <typename T>
struct SweepCall {   // psa_rk4_sweep_*, psa_rk4_sweep_waves_* and one span of a chain
    using Real = T;
    int n_waves;
    int64_t n_points, n_steps;
    double z_max;
    int32_t save_every;
    const T *dbeta, *dbeta2, *gamma, *alpha, *a0;
    uint32_t flags;
    T *a_end, *p_end, *p_max;
    int64_t *first_bad;
    T *traj;
    T *wave_end = nullptr, *wave_max = nullptr;   // the per-wave summary (on the device SoA [n_waves][N]); launched where set
    bool waves = false;                           // psa_rk4_sweep_waves_*: the summary is required, its rules are checked first
};
struct PairsCall {   // psa_rk4_sweep_pairs_f64* and one span of a multi-channel chain
    using Real = double;
    int n_pairs;
    int64_t n_points, n_steps;
    double z_max;
    int32_t save_every;
    const double *dbeta, *gamma, *alpha, *a0;
    uint32_t flags;
    double *a_end, *wave_end, *wave_max;
    int64_t *first_bad;
    double *traj = nullptr;   // a chain's rows (psa_rk4_pairs_chain_f64*); the sweep's entry points have none
};
template <typename T>
struct SinglePumpCall {   // psa_rk4_single_pump_f64*, psa_rk4_single_pump_f32* and one span of a single-pump chain
    using Real = T;
    int64_t n_points, n_steps;
    double z_max;
    int32_t save_every;
    const T *dbeta, *gamma, *alpha, *a0;
    uint32_t flags;
    T *a_end, *wave_end, *wave_max;
    int64_t *first_bad;
    T *traj;
};
template <typename T>
struct CombCall {    // psa_rk4_comb_f64*, psa_rk4_comb_f32* and one span of a multi-line chain
    using Real = T;
    int n_lines;
    int64_t n_points, n_steps;
    double z_max;
    int32_t save_every;
    const T *kappa, *gamma, *alpha, *a0;
    uint32_t flags;
    T *a_end, *wave_end, *wave_max;
    int64_t *first_bad;
    T *traj;
};
struct Rk45Call {    // psa_rk45_sweep_f64*
    int n_waves;
    int64_t n_points;
    double z_max, rtol, atol, h_max, first_step;
    int64_t max_steps, n_out;
    const double *dbeta, *dbeta2, *gamma, *alpha, *a0;
    uint32_t flags;
    double *a_end, *p_end, *p_max;
    int32_t *status;
    double *z_end;
    int64_t *n_acc, *n_rej;
    double *traj;
    int64_t traj_ld;   // leading dimension of the device rows: n_points (`_dev`), traj_ld_of (the host form's staging)
};
template <typename Span>
struct ChainCall {   // psa_rk4_chain_* (Span = SweepCall<T>), psa_rk4_single_pump_chain_f64* (SinglePumpCall<double>),
                     // psa_rk4_pairs_chain_f64* (PairsCall), psa_rk4_comb_chain_f64* (CombCall<double>)
    Span s;                     // what the spans share; its n_steps and z_max are set span by span from the arrays below
    int n_segments;
    const int64_t *n_steps;     // host [S]
    const double *seg_len;      // host [S]
    const typename Span::Real *transfer;
    void *workspace;            // device scratch of more than one span (carve_chain)
    // host [S] or NULL: span s gets PSA_OPT_LOSSLESS where it is non-zero (the host-buffer entry points: a broadcast alpha
    // of 0); `_dev` callers pass PSA_OPT_LOSSLESS for the whole chain instead
    const unsigned char *lossless = nullptr;
};

// The grid rules of every fixed-step family.  lanes_per_point: named in the message when the launch limit depends on it (0: not).
int validate_grid(int64_t n_points, long long max_points, long long lanes_per_point, int64_t n_steps, double z_max,
                  int32_t save_every) {
    if (n_points < 0) return fail(PSA_E_NPOINTS, "n_points must be >= 0, got %lld", (long long)n_points);
    if (n_points > max_points)   // the wording without the lanes leaves the last argument unread
        return fail(PSA_E_TOO_LARGE,
                    lanes_per_point ? "n_points %lld exceeds the launch limit of %lld points at %lld lanes per point"
                                    : "n_points %lld exceeds the launch limit of %lld points",
                    (long long)n_points, max_points, lanes_per_point);
    if (n_steps <= 0 || n_steps > 2147483647LL)
        return fail(PSA_E_NSTEPS, "n_steps must be in [1, 2^31), got %lld", (long long)n_steps);
    if (!(z_max > 0.0) || !std::isfinite(z_max)) return fail(PSA_E_ZMAX, "z_max must be positive");
    if (save_every <= 0) return fail(PSA_E_SAVE_EVERY, "save_every must be a positive integer");
    return PSA_OK;
}

// The per-wave summary entry points (psa_rk4_sweep_waves_*) are offered for the register layouts without trajectory
// and with the automatic block sizes only.
template <typename T>
int validate_waves(const SweepCall<T> &c) {
    if (c.traj) return fail(PSA_E_FLAGS, "the per-wave summary takes no trajectory (traj_or_null must be NULL)");
    if (c.flags & PSA_OPT_LDS_STAGING) return fail(PSA_E_FLAGS, "the per-wave summary does not exist with PSA_OPT_LDS_STAGING");
    if (c.flags & PSA_OPT_BLOCK64) return fail(PSA_E_FLAGS, "the per-wave summary does not exist with PSA_OPT_BLOCK64");
    if (c.n_points > 0 && (!c.wave_end || !c.wave_max)) return fail(PSA_E_NULLPTR, "p_wave_end / p_wave_max is NULL");
    return PSA_OK;
}

template <typename T>
int validate_common(const SweepCall<T> &c) {
    int rc;
    if (c.waves && (rc = validate_waves(c)) != PSA_OK) return rc;
    if (c.n_waves != 4 && c.n_waves != 6) return fail(PSA_E_NWAVES, "n_waves must be 4 or 6, got %d", c.n_waves);
    // a launch is at most 2^32 - 1 threads in x, and the two-lane float64 layout spends two of them per point
    rc = validate_grid(c.n_points, PSA_MAX_POINTS, 0, c.n_steps, c.z_max, c.save_every);
    if (rc != PSA_OK) return rc;
    if (c.n_waves == 6 && !c.dbeta2 && c.n_points > 0) return fail(PSA_E_DBETA2, "n_waves == 6 requires dbeta2");
    if (c.n_waves == 4 && c.dbeta2) return fail(PSA_E_DBETA2, "dbeta2 must be NULL for n_waves == 4");
    const uint32_t flags = c.flags;
    {
        const int layouts = !!(flags & PSA_OPT_SPLIT_POINT) + !!(flags & PSA_OPT_ONE_LANE) + !!(flags & PSA_OPT_QUAD_POINT);
        if (layouts > 1)
            return fail(PSA_E_FLAGS, "PSA_OPT_SPLIT_POINT, PSA_OPT_ONE_LANE and PSA_OPT_QUAD_POINT exclude each other");
        if ((flags & PSA_OPT_QUAD_POINT) && c.n_waves != 4)
            return fail(PSA_E_FLAGS, "PSA_OPT_QUAD_POINT (four lanes per point) exists for the 4-wave model only");
    }
    if ((flags & PSA_OPT_F32_SCALAR) && (flags & PSA_OPT_F32_PACKED))
        return fail(PSA_E_FLAGS, "PSA_OPT_F32_SCALAR and PSA_OPT_F32_PACKED exclude each other");
    if (c.n_points > 0 && (!c.dbeta || !c.gamma || !c.alpha || !c.a0 || !c.a_end || !c.p_end || !c.p_max || !c.first_bad))
        return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    if (c.traj) {
        // trajectory rows are addressed as a wave-uniform (row, wave) base + a 32-bit byte offset per lane, kept below 2^31
        const unsigned long long pair = 2ull * sizeof(T);
        if ((unsigned long long)c.n_points * pair >= (1ull << 31))
            return fail(PSA_E_TOO_LARGE, "a trajectory launch takes at most %llu points", (1ull << 31) / pair - 1);
        // the two-lane layout folds the lane's wave offset into that 32-bit offset
        const unsigned long long ld = (flags & PSA_OPT_TRAJ_LD) ? (unsigned long long)traj_ld_of(c.n_points, sizeof(T)) : (unsigned long long)c.n_points;
        if ((flags & (PSA_OPT_SPLIT_POINT | PSA_OPT_QUAD_POINT)) && ld * c.n_waves * pair >= (1ull << 32))
            return fail(PSA_E_TOO_LARGE, "a two-lane trajectory launch takes at most %llu points",
                        (1ull << 32) / (c.n_waves * pair) - 1);
    }
    return PSA_OK;
}

// What the argument structs of every family share (they agree on the field names): gamma, alpha and a0 with the strides the
// PSA_BCAST_* bits select, a_end, n_points and z_max ...
template <typename Args, typename Call>
void fill_shared_args(Args &a, const Call &c) {
    a.gamma = c.gamma;
    a.alpha = c.alpha;
    a.a0 = c.a0;
    a.a_end = c.a_end;
    a.n_points = c.n_points;
    a.z_max = c.z_max;
    a.gamma_stride = (c.flags & PSA_BCAST_GAMMA) ? 0 : 1;
    a.alpha_stride = (c.flags & PSA_BCAST_ALPHA) ? 0 : 1;
    a.a0_stride = (c.flags & PSA_BCAST_A0) ? 0 : 1;
    a.a0_ld = (c.flags & PSA_BCAST_A0) ? 1 : c.n_points;
}
// ... and, for SweepArgs and AdaptiveArgs, the mismatch
template <typename Args, typename Call>
void fill_point_args(Args &a, const Call &c) {
    a.dbeta = c.dbeta;
    fill_shared_args(a, c);
}

// The reference's alpha == 0.0 branch: a broadcast alpha (host pointer) of 0 selects PSA_OPT_LOSSLESS.
template <typename T>
uint32_t lossless_bit(uint32_t flags, const T *alpha) {
    return ((flags & PSA_BCAST_ALPHA) && alpha[0] == T(0)) ? PSA_OPT_LOSSLESS : 0u;
}

template <typename T> struct Launch;
template <> struct Launch<double> {
    static constexpr auto sweep = psa::launch_sweep_f64;
    static hipError_t a2s(hipStream_t s, const double *a, double *b, long long n, int nc) { return psa::launch_aos_to_soa_f64(s, a, b, n, nc); }
    static hipError_t s2a(hipStream_t s, const double *a, double *b, long long n, int nc) { return psa::launch_soa_to_aos_f64(s, a, b, n, nc); }
    static hipError_t t2a(hipStream_t s, const double *a, double *b, long long n, long long ld, long long r, int nc) { return psa::launch_traj_to_aos_f64(s, a, b, n, ld, r, nc); }
};
template <> struct Launch<float> {
    static constexpr auto sweep = psa::launch_sweep_f32;
    static hipError_t a2s(hipStream_t s, const float *a, float *b, long long n, int nc) { return psa::launch_aos_to_soa_f32(s, a, b, n, nc); }
    static hipError_t s2a(hipStream_t s, const float *a, float *b, long long n, int nc) { return psa::launch_soa_to_aos_f32(s, a, b, n, nc); }
    static hipError_t t2a(hipStream_t s, const float *a, float *b, long long n, long long ld, long long r, int nc) { return psa::launch_traj_to_aos_f32(s, a, b, n, ld, r, nc); }
};

// every pointer of c is a device pointer (a0, a_end, traj and the wave summary SoA)
template <typename T>
int sweep_dev(void *stream, const SweepCall<T> &c) {
    int rc = validate_common(c);
    if (rc != PSA_OK) return rc;
    if (c.n_points == 0) return PSA_OK;
    psa::SweepArgs<T> a;
    fill_point_args(a, c);
    a.dbeta2 = c.dbeta2;
    a.p_end = c.p_end;
    a.p_max = c.p_max;
    a.first_bad = (long long *)c.first_bad;
    a.traj = c.traj;
    a.traj_ld = (c.flags & PSA_OPT_TRAJ_LD) ? traj_ld_of(c.n_points, sizeof(T)) : c.n_points;
    a.n_steps = (int)c.n_steps;
    a.save_every = c.save_every;
    a.p_wave_end = c.wave_end;
    a.p_wave_max = c.wave_max;
    hipError_t e = Launch<T>::sweep((hipStream_t)stream, c.n_waves, c.flags, a);
    if (e != hipSuccess) return hip_fail(e, "rk4_sweep launch");
    return PSA_OK;
}

// Device scratch that frees itself on every exit path of the host-buffer entry points.
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
};

// Makes `device` current for the scope of a host-buffer entry point and puts the caller's device back afterwards
// (a host-API call must not leave a side effect on a thread that also drives torch or another HIP library).
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t enter(int device) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) return e;
        if (prev == device) return hipSuccess;
        e = hipSetDevice(device);
        switched = (e == hipSuccess);
        return e;
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

int check_device(int device, const char *what) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PSA_E_DEVICE, "no HIP device visible: %s has no CPU fallback", what);
    if (device < 0 || device >= ndev) return fail(PSA_E_DEVICE, "device %d out of range [0, %d)", device, ndev);
    return PSA_OK;
}

// ---- host-call contexts ------------------------------------------------------------------------------------------
// What a host-buffer sweep needs besides its buffers -- a stream, two timing events, (for trajectories of more than one
// point) two copy streams and an event, device scratch and a page-locked mirror for small transfers -- is created once per
// concurrent caller and device and kept in a pool: the reference's own scenarios are sweeps of 1, 30 and 100 points
// (main.py), where creating and destroying these per call cost as much as a tenth of the kernel (0.5-0.75 ms of a 4-5 ms
// single run).  A context is leased to one call at a time (concurrent callers on one device each get their own), its
// streams are drained before it goes back, and psa_release_cache() destroys the idle ones.
constexpr size_t CTX_ARENA_KEEP = 64u << 20;     // device scratch larger than this is allocated per call, not kept
constexpr size_t CTX_PINNED_IN = 256u << 10;     // page-locked mirror: inputs ...
constexpr size_t CTX_PINNED_OUT = 768u << 10;    // ... and outputs of a small sweep travel in ONE copy each way

struct HostCtx {
    int device = -1;
    hipStream_t st = nullptr, st_copy[2] = {nullptr, nullptr};
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_kernel = nullptr;
    void *arena = nullptr;
    size_t arena_cap = 0;
    char *pinned = nullptr;

    hipError_t init(int dev) {
        device = dev;
        hipError_t e;
        if ((e = hipStreamCreate(&st)) != hipSuccess) return e;
        if ((e = hipEventCreate(&ev0)) != hipSuccess) return e;
        if ((e = hipEventCreate(&ev1)) != hipSuccess) return e;
        return hipHostMalloc((void **)&pinned, CTX_PINNED_IN + CTX_PINNED_OUT, hipHostMallocDefault);
    }
    hipError_t need_copy_streams() {
        hipError_t e;
        for (int b = 0; b < 2; ++b)
            if (!st_copy[b] && (e = hipStreamCreate(&st_copy[b])) != hipSuccess) return e;
        if (!ev_kernel && (e = hipEventCreateWithFlags(&ev_kernel, hipEventDisableTiming)) != hipSuccess) return e;
        return hipSuccess;
    }
    hipError_t need_arena(size_t bytes) {   // grow-only; the caller has checked bytes <= CTX_ARENA_KEEP
        if (bytes <= arena_cap) return hipSuccess;
        if (arena) { (void)hipFree(arena); arena = nullptr; arena_cap = 0; }
        size_t cap = 1u << 20;
        while (cap < bytes) cap <<= 1;
        hipError_t e = hipMalloc(&arena, cap);
        if (e == hipSuccess) arena_cap = cap;
        return e;
    }
    void drain() {
        for (int b = 0; b < 2; ++b) if (st_copy[b]) (void)hipStreamSynchronize(st_copy[b]);
        if (st) (void)hipStreamSynchronize(st);
    }
    void destroy() {   // its device must be current
        drain();
        for (int b = 0; b < 2; ++b) if (st_copy[b]) (void)hipStreamDestroy(st_copy[b]);
        if (ev_kernel) (void)hipEventDestroy(ev_kernel);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (st) (void)hipStreamDestroy(st);
        if (arena) (void)hipFree(arena);
        if (pinned) (void)hipHostFree(pinned);
    }
};

std::mutex g_ctx_mutex;
std::vector<HostCtx *> g_ctx_idle;

// Lease of one context for the scope of a call; the device must already be current (DeviceScope) and stays so until the
// lease has ended (declare the lease AFTER the scope and after any per-call DevBuf: it drains the streams first).
struct CtxLease {
    HostCtx *c = nullptr;
    hipError_t acquire(int device) {
        {
            std::lock_guard<std::mutex> lock(g_ctx_mutex);
            for (size_t i = 0; i < g_ctx_idle.size(); ++i)
                if (g_ctx_idle[i]->device == device) {
                    c = g_ctx_idle[i];
                    g_ctx_idle.erase(g_ctx_idle.begin() + (long)i);
                    return hipSuccess;
                }
        }
        c = new HostCtx();
        hipError_t e = c->init(device);
        if (e != hipSuccess) {
            c->destroy();
            delete c;
            c = nullptr;
        }
        return e;
    }
    ~CtxLease() {
        if (!c) return;
        c->drain();   // nothing of this call may still be in flight when the buffers are reused or freed
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        g_ctx_idle.push_back(c);
    }
};

// 256-B aligned slices of one allocation; without a base (the sizing pass of a host call) it only measures
struct Carver {
    char *base = nullptr;
    size_t used = 0;
    static size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    template <typename U> U *take(size_t count) {
        U *p = base ? (U *)(base + used) : nullptr;
        used += aligned(count * sizeof(U));
        return p;
    }
};

// staging for the trajectory transpose of the host-buffer API: two buffers of at most this many bytes each
constexpr size_t TRAJ_STAGE_BYTES = 256u << 20;

#ifdef PSA_FAULT_INJECTION
// Sanitizer builds only (tools/host_sanitize.sh): PSA_FAIL_CHUNK=k makes the k-th staged trajectory chunk of every call
// fail, so the error path OUT of the staging loop (streams drained, per-call buffers freed, context returned) runs under ASan.
static bool injected_chunk_failure(size_t chunk_index) {
    const char *e = getenv("PSA_FAIL_CHUNK");
    return e && (size_t)atoll(e) == chunk_index;
}
#endif

// ---- the one staging path of every host-buffer entry point ------------------------------------------------------
// A call declares its buffers in a layout function.  host_call() runs it twice: against unplaced Carvers to measure the
// scratch, then against the scratch itself, where the same declarations hand out the device pointers and record the
// copies and transposes.  Scratch: [inputs] [device-only] [outputs] [trajectory, two staging buffers].  The input and the
// output region are each contiguous, so a small call's inputs and outputs travel in ONE copy each way through the
// context's page-locked mirror.  A NULL host pointer declares no buffer and yields a NULL device pointer.
template <typename T>
struct Staging {
    struct Copy { void *host; void *dev; size_t bytes; };
    struct Transpose { const T *from; T *to; size_t rows; int nc, batches; };
    struct Traj { T *dev = nullptr, *host = nullptr, *stage[2] = {nullptr, nullptr}; size_t n = 0, rows = 0, ld = 0, chunk = 0; int nc = 0; };
    Carver in, mid, out, big;
    std::vector<Copy> ups, downs;
    std::vector<Transpose> to_soa, to_aos;
    Traj traj;
    bool has_traj = false, traj_too_large = false;

    template <typename U> U *input(const U *host, size_t count) {            // host -> device as it is
        if (!host) return nullptr;
        U *d = in.take<U>(count);
        ups.push_back({(void *)host, (void *)d, count * sizeof(U)});
        return d;
    }
    template <typename U> U *output(U *host, size_t count) {                  // device -> host as it is
        if (!host) return nullptr;
        U *d = out.take<U>(count);
        downs.push_back({(void *)host, (void *)d, count * sizeof(U)});
        return d;
    }
    template <typename U> U *scratch(size_t count) { return mid.take<U>(count); }
    T *input_soa(const T *host, size_t rows, int nc, int batches = 1) {      // host [batches][rows][nc] -> [batches][nc][rows]
        if (!host) return nullptr;
        const T *aos = input(host, (size_t)batches * rows * nc);
        T *soa = mid.take<T>((size_t)batches * rows * nc);
        to_soa.push_back({aos, soa, rows, nc, batches});
        return soa;
    }
    T *output_soa(T *host, size_t rows, int nc) {                            // device [nc][rows] -> host [rows][nc]
        if (!host) return nullptr;
        T *soa = mid.take<T>(rows * nc);
        to_aos.push_back({soa, output(host, rows * nc), rows, nc, 1});
        return soa;
    }
    // device [rows][nc/2][ld][2] -> host [n][rows][nc/2][2].  One point's layouts coincide: it leaves with the outputs.
    // More points leave in chunks of whole 32-point transpose tiles (very long single runs: one tile per chunk).
    T *trajectory(T *host, size_t n, size_t rows, int nc) {
        if (!host) return nullptr;
        has_traj = true;
        if (n == 1) return output(host, rows * nc);
        const size_t ld = (size_t)traj_ld_of((int64_t)n, sizeof(T)), point_bytes = rows * nc * sizeof(T);
        if ((long double)ld * rows * nc * sizeof(T) > 4.0e18L) { traj_too_large = true; return nullptr; }
        size_t chunk = (TRAJ_STAGE_BYTES / point_bytes) / 32 * 32;
        if (chunk < 32) chunk = 32;
        if (chunk > n) chunk = n;
        traj.dev = big.take<T>(ld * rows * nc);
        for (int b = 0; b < 2; ++b) traj.stage[b] = (T *)big.take<char>(chunk * point_bytes);
        traj.host = host;
        traj.n = n;
        traj.rows = rows;
        traj.ld = ld;
        traj.chunk = chunk;
        traj.nc = nc;
        return traj.dev;
    }
};

// Checks the device, leases a context, lays out and fills the scratch, runs compute(stream) (elapsed_ms: the compute alone,
// between the context's two timing events), brings the outputs home and returns once every stream of the call has finished.
template <typename T, typename Layout, typename Compute>
int host_call(int device, const char *what, double *elapsed_ms, Layout &&layout, Compute &&compute) {
    int rc = check_device(device, what);
    if (rc != PSA_OK) return rc;
    Staging<T> size;
    layout(size);
    if (size.traj_too_large) return fail(PSA_E_TOO_LARGE, "trajectory buffer too large");
    const size_t in_b = size.in.used, mid_b = size.mid.used, out_b = size.out.used;
    const size_t total = in_b + mid_b + out_b + size.big.used;

    DeviceScope scope;
    DevBuf own;          // scratch above CTX_ARENA_KEEP is allocated per call
    CtxLease lease;      // declared last: its streams are drained before `own` is freed and the device restored
    HIP_RET(scope.enter(device));
    if (size.has_traj && total > CTX_ARENA_KEEP) {   // say "too large" before hipMalloc says "out of memory"
        size_t free_b = 0, total_b = 0;
        HIP_RET(hipMemGetInfo(&free_b, &total_b));
        if (total > free_b)
            return fail(PSA_E_TOO_LARGE, "trajectory of %.3g GB does not fit the %.3g GB free on device %d",
                        (double)total / 1e9, (double)free_b / 1e9, device);
    }
    HIP_RET(lease.acquire(device));
    HostCtx &cx = *lease.c;
    hipStream_t st = cx.st;
    char *base;
    if (total <= CTX_ARENA_KEEP) {
        HIP_RET(cx.need_arena(total));
        base = (char *)cx.arena;
    } else {
        HIP_RET(own.alloc(total));
        base = (char *)own.p;
    }
    Staging<T> sg;
    sg.in.base = base;
    sg.mid.base = base + in_b;
    sg.out.base = sg.mid.base + mid_b;
    sg.big.base = sg.out.base + out_b;
    layout(sg);

    const bool mirror = in_b <= CTX_PINNED_IN && out_b <= CTX_PINNED_OUT;
    char *m_in = cx.pinned, *m_out = cx.pinned + CTX_PINNED_IN;   // same offsets as the device regions
    for (const auto &c : sg.ups) {
        if (!c.bytes) continue;
        if (mirror) std::memcpy(m_in + ((char *)c.dev - sg.in.base), c.host, c.bytes);
        else HIP_RET(hipMemcpyAsync(c.dev, c.host, c.bytes, hipMemcpyHostToDevice, st));
    }
    if (mirror && in_b) HIP_RET(hipMemcpyAsync(sg.in.base, m_in, in_b, hipMemcpyHostToDevice, st));
    for (const auto &t : sg.to_soa)
        for (int b = 0; b < t.batches; ++b)
            HIP_RET(Launch<T>::a2s(st, t.from + b * t.rows * t.nc, t.to + b * t.rows * t.nc, (long long)t.rows, t.nc));
    if (elapsed_ms) HIP_RET(hipEventRecord(cx.ev0, st));   // only on request: two records are measurable on a small call
    rc = compute(st);
    if (rc != PSA_OK) return rc;
    if (elapsed_ms) HIP_RET(hipEventRecord(cx.ev1, st));
    for (const auto &t : sg.to_aos) HIP_RET(Launch<T>::s2a(st, t.from, t.to, (long long)t.rows, t.nc));
    if (mirror) {
        if (out_b) HIP_RET(hipMemcpyAsync(m_out, sg.out.base, out_b, hipMemcpyDeviceToHost, st));
    } else {
        for (const auto &c : sg.downs)
            if (c.bytes) HIP_RET(hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, st));
    }
    if (const auto &tr = sg.traj; tr.dev) {
        // [rows][nw][ld] -> chunk [pts][rows][nw] in one staging buffer while the other one's chunk is being copied home
        HIP_RET(cx.need_copy_streams());
        HIP_RET(hipEventRecord(cx.ev_kernel, st));
        for (int b = 0; b < 2; ++b) HIP_RET(hipStreamWaitEvent(cx.st_copy[b], cx.ev_kernel, 0));
        const size_t point_elems = tr.rows * tr.nc;
        int b = 0;
        for (size_t p0 = 0; p0 < tr.n; p0 += tr.chunk, b ^= 1) {
            const size_t pts = (tr.n - p0 < tr.chunk) ? tr.n - p0 : tr.chunk;
#ifdef PSA_FAULT_INJECTION
            if (injected_chunk_failure(p0 / tr.chunk)) return hip_fail(hipErrorUnknown, "injected failure in the staging loop");
#endif
            // stream order on st_copy[b] keeps the staging buffer busy until its previous copy has finished
            HIP_RET(Launch<T>::t2a(cx.st_copy[b], tr.dev + 2 * p0, tr.stage[b], (long long)pts, (long long)tr.ld,
                                   (long long)tr.rows, tr.nc));
            HIP_RET(hipMemcpyAsync(tr.host + p0 * point_elems, tr.stage[b], pts * point_elems * sizeof(T),
                                   hipMemcpyDeviceToHost, cx.st_copy[b]));
        }
        HIP_RET(hipStreamSynchronize(cx.st_copy[0]));
        HIP_RET(hipStreamSynchronize(cx.st_copy[1]));
    }
    HIP_RET(hipStreamSynchronize(st));
    if (mirror)
        for (const auto &c : sg.downs) std::memcpy(c.host, m_out + ((char *)c.dev - sg.out.base), c.bytes);
    if (elapsed_ms) {
        float ms = 0.f;
        HIP_RET(hipEventElapsedTime(&ms, cx.ev0, cx.ev1));
        *elapsed_ms = (double)ms;
    }
    return PSA_OK;
}

template <typename T>
int sweep_host(int device, const SweepCall<T> &c, double *elapsed_ms) {
    int rc = validate_common(c);
    if (rc != PSA_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (c.n_points == 0) return PSA_OK;
    const int nc = 2 * c.n_waves;
    const size_t N = (size_t)c.n_points;
    SweepCall<T> d = c;                       // the call on device buffers: the layout fills in the pointers
    if (c.traj) d.flags |= PSA_OPT_TRAJ_LD;   // the device-side trajectory has its own leading dimension; the caller's is dense
    d.flags |= lossless_bit(c.flags, c.alpha);
    auto layout = [&](Staging<T> &sg) {
        d.dbeta = sg.input(c.dbeta, N);
        d.dbeta2 = sg.input(c.dbeta2, N);
        d.gamma = sg.input(c.gamma, (c.flags & PSA_BCAST_GAMMA) ? 1 : N);
        d.alpha = sg.input(c.alpha, (c.flags & PSA_BCAST_ALPHA) ? 1 : N);
        d.a0 = sg.input_soa(c.a0, (c.flags & PSA_BCAST_A0) ? 1 : N, nc);
        d.a_end = sg.output_soa(c.a_end, N, nc);
        d.p_end = sg.output(c.p_end, N);
        d.p_max = sg.output(c.p_max, N);
        d.first_bad = sg.output(c.first_bad, N);
        d.wave_end = sg.output_soa(c.wave_end, N, c.n_waves);
        d.wave_max = sg.output_soa(c.wave_max, N, c.n_waves);
        d.traj = sg.trajectory(c.traj, N, (size_t)(c.n_steps / c.save_every + 1), nc);
    };
    return host_call<T>(device, "the RK4 sweep", elapsed_ms, layout, [&](hipStream_t st) { return sweep_dev<T>(st, d); });
}

// ---- the wave-summary families: multi-channel (psa_rk4_sweep_pairs_f64*), single-pump (psa_rk4_single_pump_*) and multi-line
// ("comb", psa_rk4_comb_*) -----------------------------------------------------------------------------------------------
// Three models with one surface: a_end, the end and the maximum power of every wave, first_bad_step and optional rows.  One
// validator, one `_dev` function and one host function serve them, as sweeps and as the spans of their chains; what differs
// between them -- and between them and the 4/6-wave sweep as a chain's span -- is stated once per record, in Family<> below.
template <typename Span> struct Family;
// The array of a record whose values a chain's gauge accumulates: dbeta, or the multi-line model's kappa.
template <typename Span> auto mismatch_of(Span &c) -> decltype((c.dbeta)) { return c.dbeta; }
template <typename T> const T *&mismatch_of(CombCall<T> &c) { return c.kappa; }
template <typename T> const T *mismatch_of(const CombCall<T> &c) { return c.kappa; }

// host_form: the call as the host-buffer entry point received it (PSA_OPT_TRAJ_LD is the `_dev` form's; the host form's
// device-side trajectory always has the padded leading dimension); chain: the call is (a span of) the family's chain.  The
// order is validate_common's with the family's count in front; float32 has one layout (two points per lane), so
// PSA_OPT_F32_SCALAR / PSA_OPT_F32_PACKED are refused like every other layout flag.
template <typename Call>
int validate_wave(const Call &c, bool host_form, bool chain = false) {
    using F = Family<Call>;
    using T = typename Call::Real;
    int rc = F::check_count(c);
    if (rc != PSA_OK) return rc;
    // a launch is at most 2^32 - 1 threads in x, two of which the limit allows per point; a family that spends more says so
    const long long lanes = F::lanes_per_point(c);
    rc = validate_grid(c.n_points, lanes ? 2 * PSA_MAX_POINTS / lanes : PSA_MAX_POINTS, lanes, c.n_steps, c.z_max, c.save_every);
    if (rc != PSA_OK) return rc;
    const bool rows = F::sweep_rows || chain;   // a sweep without rows has them as one span of its chain, and says "chain" there
    const uint32_t accepted = PSA_BCAST_GAMMA | PSA_BCAST_ALPHA | PSA_BCAST_A0 | PSA_OPT_CHECK_NAN | PSA_OPT_EXACT_STEP |
                              PSA_OPT_LOSSLESS | PSA_OPT_BLOCK64 | ((rows && !host_form) ? PSA_OPT_TRAJ_LD : 0u);
    if (c.flags & ~accepted)
        return fail(PSA_E_FLAGS, rows ? "the %s %s takes the BCAST bits, CHECK_NAN, EXACT_STEP, LOSSLESS, BLOCK64 and (its _dev form) "
                                        "TRAJ_LD only (no layout, float32 or LDS flag): 0x%x"
                                      : "the %s %s takes the BCAST bits, CHECK_NAN, EXACT_STEP, LOSSLESS and BLOCK64 only (no layout, "
                                        "float32 or LDS flag): 0x%x",
                    F::name, (chain && !F::sweep_rows) ? "chain" : "sweep", (unsigned)(c.flags & ~accepted));
    if (c.n_points > 0 && (!mismatch_of(c) || !c.gamma || !c.alpha || !c.a0 || !c.a_end || !c.wave_end || !c.wave_max || !c.first_bad))
        return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    if (c.traj) {
        // trajectory rows are addressed as a wave-uniform (row, wave) base + the lane's 32-bit byte offset (the multi-channel
        // kernel addresses its rows with 64 bits per lane and keeps the bound for parity between the families)
        const bool padded = host_form || (c.flags & PSA_OPT_TRAJ_LD);
        const unsigned long long ld = (unsigned long long)(padded ? traj_ld_of(c.n_points, sizeof(T)) : c.n_points);
        // float64: one 16-byte pair per lane below 2^32; float32: the packed sweep's bound, 8-byte pairs below 2^31
        if (ld * 2ull * sizeof(T) >= (sizeof(T) == 8 ? 1ull << 32 : 1ull << 31))
            return fail(PSA_E_TOO_LARGE, "a %s trajectory launch takes a leading dimension below 2^28 points, got %llu", F::name, ld);
    }
    return PSA_OK;
}

// every pointer of c is a device pointer (SoA: a mismatch of several rows, a0, a_end, the summaries and the rows)
template <typename Call>
int wave_dev(void *stream, const Call &c, bool chain = false) {
    using F = Family<Call>;
    int rc = validate_wave(c, false, chain);
    if (rc != PSA_OK) return rc;
    if (c.n_points == 0) return PSA_OK;
    typename F::Args a;
    fill_shared_args(a, c);
    a.p_wave_end = c.wave_end;
    a.p_wave_max = c.wave_max;
    a.first_bad = (long long *)c.first_bad;
    a.traj = c.traj;
    a.traj_ld = (c.flags & PSA_OPT_TRAJ_LD) ? traj_ld_of(c.n_points, sizeof(typename Call::Real)) : c.n_points;
    a.n_steps = (int)c.n_steps;
    a.save_every = c.save_every;
    hipError_t e = F::launch((hipStream_t)stream, a, c);   // sets the mismatch and the family's count
    if (e != hipSuccess) return hip_fail(e, F::launch_what);
    return PSA_OK;
}

// The mismatch of S spans (a sweep: one) on the device: [S][N] as it is, or [S][N][rows] -> [S][rows][N]
template <typename Span>
auto stage_mismatch(Staging<typename Span::Real> &sg, const Span &c, int S, size_t N) {
    return Family<Span>::mismatch_soa ? sg.input_soa(mismatch_of(c), N, Family<Span>::dbeta_rows(c), S) : sg.input(mismatch_of(c), S * N);
}
// The summary of a wave-summary family, sweep or chain
template <typename Call>
void stage_wave_summary(Staging<typename Call::Real> &sg, Call &d, const Call &c, size_t N) {
    d.wave_end = sg.output_soa(c.wave_end, N, Family<Call>::n_waves(c));
    d.wave_max = sg.output_soa(c.wave_max, N, Family<Call>::n_waves(c));
    d.first_bad = sg.output(c.first_bad, N);
}

template <typename Call>
int wave_host(int device, const Call &c, double *elapsed_ms) {
    using F = Family<Call>;
    using T = typename Call::Real;
    int rc = validate_wave(c, true);
    if (rc != PSA_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (c.n_points == 0) return PSA_OK;
    const int nc = 2 * F::n_waves(c);
    const size_t N = (size_t)c.n_points;
    Call d = c;
    if (c.traj) d.flags |= PSA_OPT_TRAJ_LD;   // the device-side trajectory has its own leading dimension; the caller's is dense
    d.flags |= lossless_bit(c.flags, c.alpha);
    auto layout = [&](Staging<T> &sg) {
        mismatch_of(d) = stage_mismatch(sg, c, 1, N);
        d.gamma = sg.input(c.gamma, (c.flags & PSA_BCAST_GAMMA) ? 1 : N);
        d.alpha = sg.input(c.alpha, (c.flags & PSA_BCAST_ALPHA) ? 1 : N);
        d.a0 = sg.input_soa(c.a0, (c.flags & PSA_BCAST_A0) ? 1 : N, nc);
        d.a_end = sg.output_soa(c.a_end, N, nc);
        stage_wave_summary(sg, d, c, N);
        d.traj = sg.trajectory(c.traj, N, (size_t)(c.n_steps / c.save_every + 1), nc);   // a sweep without rows: NULL in, NULL out
    };
    return host_call<T>(device, F::sweep_what, elapsed_ms, layout, [&](hipStream_t st) { return wave_dev(st, d); });
}

// What differs between the families, stated once per family: the record decides.  As a chain's span every family states the
// index and stride of its signals (whose phase the gauge accumulates), its summary, and whether one span alone may end behind
// its last saved row; a wave-summary family adds what validate_wave, wave_dev and wave_host read.
template <typename T> struct Family<SweepCall<T>> {   // 4 and 6 waves [p1, p2, s, i, ...]
    static constexpr int sig_wave = 2, sig_stride = 2;
    static constexpr bool signal_summary = true;      // p_end / p_max
    static constexpr bool waves_optional = true;      // the per-wave summary where p_wave_end / p_wave_max are given
    static constexpr bool second_mismatch = true;     // dbeta2 / theta2 (6 waves)
    static constexpr bool sweep_tail = false;         // one span, too, must end on a saved row
    static constexpr bool mismatch_soa = false;
    static constexpr const char *what = "the fibre chain";
    static int n_waves(const SweepCall<T> &c) { return c.n_waves; }
    static int n_signals(const SweepCall<T> &c) { return c.n_waves == 6 ? 2 : 1; }
    static int dbeta_rows(const SweepCall<T> &) { return 1; }   // rows of [N] a span's dbeta holds
    static int validate_first(const SweepCall<T> &first, bool) { return validate_common(first); }
    static int span_dev(void *stream, const SweepCall<T> &c) { return sweep_dev<T>(stream, c); }
    static void stage_summary(Staging<T> &sg, SweepCall<T> &d, const SweepCall<T> &c, size_t N) {
        d.p_end = sg.output(c.p_end, N);
        d.p_max = sg.output(c.p_max, N);
        d.first_bad = sg.output(c.first_bad, N);
        d.wave_end = sg.output_soa(c.wave_end, N, c.n_waves);
        d.wave_max = sg.output_soa(c.wave_max, N, c.n_waves);
    }
};
// A wave-summary family as a chain's span: the per-wave columns are the summary, and the sweep's own functions run the span.
template <typename Call> struct WaveSpan {
    static constexpr bool signal_summary = false, waves_optional = false, second_mismatch = false;
    static int validate_first(Call first, bool host_form) {
        first.flags &= ~PSA_BCAST_TRANSFER;   // the chain's own bit
        return validate_wave(first, host_form, true);
    }
    static int span_dev(void *stream, const Call &c) { return wave_dev(stream, c, true); }
    static void stage_summary(Staging<typename Call::Real> &sg, Call &d, const Call &c, size_t N) { stage_wave_summary(sg, d, c, N); }
};
template <typename T> struct Family<SinglePumpCall<T>> : WaveSpan<SinglePumpCall<T>> {   // three waves [p, s, i]
    using Call = SinglePumpCall<T>;
    using Args = psa::SinglePumpArgs<T>;
    static constexpr int sig_wave = 1, sig_stride = 2;
    static constexpr bool sweep_tail = false, sweep_rows = true, mismatch_soa = false;
    static constexpr const char *name = "single-pump", *sweep_what = "the single-pump RK4 sweep", *what = "the single-pump fibre chain",
                                 *launch_what = "rk4_sweep_single_pump launch";
    static int n_waves(const Call &) { return 3; }
    static int n_signals(const Call &) { return 1; }
    static int dbeta_rows(const Call &) { return 1; }
    static int check_count(const Call &) { return PSA_OK; }
    static long long lanes_per_point(const Call &) { return 0; }   // one, or half a lane: PSA_MAX_POINTS holds, no lanes in the message
    static hipError_t launch(hipStream_t st, Args &a, const Call &c) {
        a.dbeta = c.dbeta;
        if constexpr (sizeof(T) == 8) return psa::launch_sweep_single_pump_f64(st, c.flags, a);
        else return psa::launch_sweep_single_pump_f32(st, c.flags, a);
    }
};
template <> struct Family<PairsCall> : WaveSpan<PairsCall> {   // two pumps and K pairs [p1, p2, s_1, i_1, ..., s_K, i_K]: K signals, K mismatches
    using Call = PairsCall;
    using Args = psa::PairsArgs;
    static constexpr int sig_wave = 2, sig_stride = 2;
    // one span is the sweep's trajectory form and keeps the sweep's rule: A[-1] is the last SAVED row, a tail may follow it
    static constexpr bool sweep_tail = true;
    static constexpr bool sweep_rows = false;    // psa_rk4_sweep_pairs_f64* stages no rows and takes no PSA_OPT_TRAJ_LD: the chain does
    static constexpr bool mismatch_soa = true;   // a span's dbeta is SoA [K][N]
    static constexpr const char *name = "multi-channel", *sweep_what = "the multi-channel RK4 sweep", *what = "the multi-channel fibre chain",
                                 *launch_what = "rk4_sweep_pairs launch";
    static int n_waves(const Call &c) { return 2 + 2 * c.n_pairs; }
    static int n_signals(const Call &c) { return c.n_pairs; }
    static int dbeta_rows(const Call &c) { return c.n_pairs; }
    static int check_count(const Call &c) {
        if (c.n_pairs >= 1 && c.n_pairs <= PSA_MAX_PAIRS) return PSA_OK;
        return fail(PSA_E_NPAIRS, "n_pairs must be in [1, %d], got %d", PSA_MAX_PAIRS, c.n_pairs);
    }
    // a point takes L lanes: the power of two >= n_pairs (at least 2)
    static long long lanes_per_point(const Call &c) { return psa::pairs_lanes_per_point(c.n_pairs); }
    static hipError_t launch(hipStream_t st, Args &a, const Call &c) {
        a.dbeta = c.dbeta;
        a.n_pairs = c.n_pairs;
        return psa::launch_sweep_pairs_f64(st, c.flags, a);
    }
};
template <typename T> struct Family<CombCall<T>> : WaveSpan<CombCall<T>> {   // M lines, every one with its own accumulated phase: M "signals" at waves 0..M-1
    using Call = CombCall<T>;
    using Args = psa::CombArgs<T>;
    static constexpr int sig_wave = 0, sig_stride = 1;
    static constexpr bool sweep_tail = false, sweep_rows = true;
    static constexpr bool mismatch_soa = true;   // a span's kappa is SoA [M][N]
    static constexpr const char *name = "multi-line", *sweep_what = "the multi-line RK4 sweep", *what = "the multi-line fibre chain",
                                 *launch_what = "rk4_sweep_comb launch";
    static int n_waves(const Call &c) { return c.n_lines; }
    static int n_signals(const Call &c) { return c.n_lines; }
    static int dbeta_rows(const Call &c) { return c.n_lines; }
    static int check_count(const Call &c) {
        if (c.n_lines >= 3 && c.n_lines <= PSA_MAX_LINES) return PSA_OK;
        return fail(PSA_E_NLINES, "n_lines must be in [3, %d], got %d", PSA_MAX_LINES, c.n_lines);
    }
    static long long lanes_per_point(const Call &) { return 0; }
    static hipError_t launch(hipStream_t st, Args &a, const Call &c) {
        a.kappa = c.kappa;
        a.n_lines = c.n_lines;
        if constexpr (sizeof(T) == 8) return psa::launch_sweep_comb_f64(st, c.flags, a);
        else return psa::launch_sweep_comb_f32(st, c.flags, a);
    }
};

// ---- fibre chains: S spans, one sweep launch + one epilogue (psa_chain.hip) each ------------------------------------
template <typename T> struct EpilogueLaunch;
template <> struct EpilogueLaunch<double> { static constexpr auto fn = psa::launch_chain_epilogue_f64; };
template <> struct EpilogueLaunch<float> { static constexpr auto fn = psa::launch_chain_epilogue_f32; };

// Device scratch of a chain of more than one span: Theta (float64, one per signal), the next span's a0, and the span's own
// outputs before they are folded into the running ones.  Without a base it only measures (`bytes`).
template <typename T>
struct ChainScratch {
    double *theta, *theta2;
    T *a0_next, *a_end_s, *p_end_s, *p_max_s;
    int64_t *bad_s;
    T *wend_s, *wmax_s;
    size_t bytes;
    // theta_rows: the Theta of that many signals in ONE block [theta_rows][N] (the multi-channel model's K; theta2 is its
    // second row); two_thetas: a second signal's Theta in a block of its own (6 waves)
    ChainScratch(void *base, size_t N, int n_waves, bool two_thetas, bool signal_summary, bool waves, int theta_rows = 1) {
        Carver ws;
        ws.base = (char *)base;
        theta = ws.take<double>((size_t)theta_rows * N);
        theta2 = two_thetas ? ws.take<double>(N) : (theta_rows > 1 && theta ? theta + N : nullptr);
        a0_next = ws.take<T>(2 * (size_t)n_waves * N);
        a_end_s = ws.take<T>(2 * (size_t)n_waves * N);
        p_end_s = signal_summary ? ws.take<T>(N) : nullptr;
        p_max_s = signal_summary ? ws.take<T>(N) : nullptr;
        bad_s = ws.take<int64_t>(N);
        wend_s = waves ? ws.take<T>((size_t)n_waves * N) : nullptr;
        wmax_s = waves ? ws.take<T>((size_t)n_waves * N) : nullptr;
        bytes = ws.used;
    }
    template <typename Span>
    static ChainScratch of(void *base, const Span &c) {
        using F = Family<Span>;
        const int n_waves = F::n_waves(c);
        return ChainScratch(base, (size_t)c.n_points, n_waves, F::second_mismatch && n_waves == 6, F::signal_summary,
                            !F::waves_optional || c.wave_end != nullptr, F::second_mismatch ? 1 : F::n_signals(c));
    }
};

// The part of span s's epilogue record that every chain family fills alike: the frame (Theta, the rows to rotate, the
// A-frame a_end of the last span), first_bad_step with its step offset, and the boundary to span s + 1.  The family adds its
// wave count, the index of its signal and its summary buffers.
template <typename T>
struct SpanJoin {
    int64_t n_points;
    int n_segments;
    uint32_t flags;          // PSA_BCAST_TRANSFER is read here
    const T *transfer;       // the chain's [S-1] transfers or nullptr
    size_t transfer_step;    // elements from one boundary's transfer to the next
    T *a_end, *a0_next, *a_end_s;
    int64_t *first_bad, *first_bad_s;
    double *theta;
    size_t traj_ld;
    psa::ChainEpilogue<T> record(int s, int64_t step_offset, T *span_traj, int64_t rows, const T *dbeta, double seg_len) const {
        const bool first = s == 0, last = s == n_segments - 1;
        psa::ChainEpilogue<T> e;
        e.n = n_points;
        e.first = first;
        e.fold = !first;
        e.a_end_s = a_end_s;
        e.first_bad_s = (const long long *)first_bad_s;
        e.first_bad = (long long *)first_bad;
        e.step_offset = step_offset;
        e.theta = theta;
        e.traj = span_traj;
        e.traj_ld = (long long)traj_ld;
        e.rows = rows;
        e.a_end_out = last ? a_end : nullptr;
        e.transfer = (!last && transfer) ? transfer + s * transfer_step : nullptr;
        e.transfer_stride = (flags & PSA_BCAST_TRANSFER) ? 0 : 1;
        e.dbeta = dbeta;
        e.seg_len = seg_len;
        e.a0_next = a0_next;
        return e;
    }
};

// The grid rules of a chain's spans (every chain family); *rows_total = sum over spans of n_steps[s] / save_every + 1.
// tail_ok: this span count may end behind its last saved row, as a sweep may (Family::sweep_tail: one span alone)
int validate_spans(int n_segments, const int64_t *n_steps, const double *seg_len, int32_t save_every, int64_t *rows_total,
                   bool tail_ok = false) {
    int64_t rows = 0;
    for (int s = 0; s < n_segments; ++s) {
        if (n_steps[s] <= 0 || n_steps[s] > 2147483647LL)
            return fail(PSA_E_NSTEPS, "n_steps[%d] must be in [1, 2^31), got %lld", s, (long long)n_steps[s]);
        if (!(seg_len[s] > 0.0) || !std::isfinite(seg_len[s])) return fail(PSA_E_ZMAX, "seg_len[%d] must be positive", s);
        // a_end is the last saved row: a tail after it would silently shorten the span
        if (n_steps[s] % save_every != 0 && !tail_ok)
            return fail(PSA_E_SAVE_EVERY, "n_steps[%d] = %lld is not a multiple of save_every = %d", s,
                        (long long)n_steps[s], (int)save_every);
        rows += n_steps[s] / save_every + 1;
    }
    *rows_total = rows;
    return PSA_OK;
}

// The reference's alpha == 0.0 branch, span by span, for the host-buffer chains: a broadcast 0, or (S > 1, where a lossy span
// elsewhere makes the alpha array per point) a span whose row is 0 everywhere.  One span keeps the sweep's rule: bit-identical.
template <typename T>
std::vector<unsigned char> lossless_spans(uint32_t flags, const T *alpha, int S, size_t N) {
    std::vector<unsigned char> lossless((size_t)S, 0);
    for (int s = 0; s < S; ++s) {
        bool zero = lossless_bit(flags, alpha + s) != 0;
        if (!(flags & PSA_BCAST_ALPHA) && S > 1) {
            const T *a = alpha + (size_t)s * N;
            zero = true;
            for (size_t i = 0; i < N && zero; ++i) zero = a[i] == T(0);
        }
        lossless[(size_t)s] = zero;
    }
    return lossless;
}

// argument rules of every chain: the span count, the first span's grid through the family's sweep validator, the later spans
template <typename Span>
int validate_chain(const ChainCall<Span> &c, bool host_form, int64_t *rows_total) {
    using F = Family<Span>;
    if (c.n_segments < 1) return fail(PSA_E_NSTEPS, "n_segments must be >= 1, got %d", c.n_segments);
    if (!c.n_steps || !c.seg_len) return fail(PSA_E_NULLPTR, "n_steps / seg_len is NULL");
    Span first = c.s;   // the sweep's rules, on the first span's grid
    first.n_steps = c.n_steps[0];
    first.z_max = c.seg_len[0];
    int rc = F::validate_first(first, host_form);
    if (rc != PSA_OK) return rc;
    int64_t rows = 0;
    if ((rc = validate_spans(c.n_segments, c.n_steps, c.seg_len, c.s.save_every, &rows, F::sweep_tail && c.n_segments == 1)) != PSA_OK)
        return rc;
    if constexpr (F::waves_optional) {
        if ((c.s.wave_end != nullptr) != (c.s.wave_max != nullptr))
            return fail(PSA_E_NULLPTR, "p_wave_end and p_wave_max are given together or not at all");
        if (c.s.wave_end && (rc = validate_waves(c.s)) != PSA_OK) return rc;
    }
    if (c.s.traj && (long double)rows * 2 * F::n_waves(c.s) * (long double)traj_ld_of(c.s.n_points, sizeof(typename Span::Real)) > 4.0e18L)
        return fail(PSA_E_TOO_LARGE, "trajectory buffer too large");
    *rows_total = rows;
    return PSA_OK;
}

template <typename Span>
int chain_dev(void *stream, const ChainCall<Span> &c) {
    using F = Family<Span>;
    using T = typename Span::Real;
    int64_t rows_total = 0;
    int rc = validate_chain(c, false, &rows_total);
    if (rc != PSA_OK) return rc;
    if (c.s.n_points == 0) return PSA_OK;
    const int S = c.n_segments, n_waves = F::n_waves(c.s);
    const uint32_t flags = c.s.flags;
    Span sp = c.s;   // the span being run
    auto set_span = [&](int s) {
        sp.n_steps = c.n_steps[s];
        sp.z_max = c.seg_len[s];
        sp.flags = flags & ~PSA_BCAST_TRANSFER;
        if (s > 0) sp.flags &= ~PSA_BCAST_A0;                  // the next span starts from a per-point state
        if (c.lossless && c.lossless[s]) sp.flags |= PSA_OPT_LOSSLESS;
    };
    if (S == 1) {   // one span IS the sweep: same launch, same outputs, bit for bit
        set_span(0);
        return F::span_dev(stream, sp);
    }
    if (!c.workspace) return fail(PSA_E_NULLPTR, "a chain of more than one span needs d_workspace");

    const size_t N = (size_t)c.s.n_points;
    const int nc = 2 * n_waves;
    const auto w = ChainScratch<T>::of(c.workspace, c.s);
    const size_t ld = (flags & PSA_OPT_TRAJ_LD) ? (size_t)traj_ld_of(c.s.n_points, sizeof(T)) : N;
    const size_t g_step = (flags & PSA_BCAST_GAMMA) ? 1 : N, a_step = (flags & PSA_BCAST_ALPHA) ? 1 : N;
    const size_t t_step = (flags & PSA_BCAST_TRANSFER) ? (size_t)nc : nc * N;
    const SpanJoin<T> join{c.s.n_points, S, flags, c.transfer, t_step, c.s.a_end, w.a0_next, w.a_end_s, c.s.first_bad, w.bad_s, w.theta, ld};
    int64_t row = 0, step_off = 0;
    for (int s = 0; s < S; ++s) {
        const bool first = s == 0;
        set_span(s);
        const T *const dbeta = mismatch_of(c.s) + s * (F::dbeta_rows(c.s) * N);
        mismatch_of(sp) = dbeta;
        sp.gamma = c.s.gamma + s * g_step;
        sp.alpha = c.s.alpha + s * a_step;
        sp.a0 = first ? c.s.a0 : w.a0_next;
        sp.a_end = w.a_end_s;
        sp.first_bad = first ? c.s.first_bad : w.bad_s;
        sp.traj = c.s.traj ? c.s.traj + (size_t)row * n_waves * ld * 2 : nullptr;
        sp.wave_end = w.wend_s ? (first ? c.s.wave_end : w.wend_s) : nullptr;
        sp.wave_max = w.wmax_s ? (first ? c.s.wave_max : w.wmax_s) : nullptr;
        if constexpr (F::signal_summary) {
            sp.p_end = first ? c.s.p_end : w.p_end_s;
            sp.p_max = first ? c.s.p_max : w.p_max_s;
        }
        if constexpr (F::second_mismatch) sp.dbeta2 = c.s.dbeta2 ? c.s.dbeta2 + s * N : nullptr;
        rc = F::span_dev(stream, sp);
        if (rc != PSA_OK) return rc;
        psa::ChainEpilogue<T> e = join.record(s, step_off, sp.traj, sp.n_steps / sp.save_every + 1, dbeta, sp.z_max);
        e.n_waves = n_waves;
        e.sig_wave = F::sig_wave;
        e.sig_stride = F::sig_stride;
        e.p_end_s = w.p_end_s;
        e.p_max_s = w.p_max_s;
        e.wave_end_s = w.wend_s;
        e.wave_max_s = w.wmax_s;
        e.wave_end = c.s.wave_end;
        e.wave_max = c.s.wave_max;
        e.n_sig = F::n_signals(c.s);
        e.theta2 = w.theta2;
        e.sig_ld = (long long)N;
        e.p_end = e.p_max = nullptr;   // a family without the signal summary
        e.dbeta2 = e.n_sig > 1 ? dbeta + N : nullptr;   // the rows of one [K][N] block, or ...
        if constexpr (F::signal_summary) {
            e.p_end = c.s.p_end;
            e.p_max = c.s.p_max;
        }
        if constexpr (F::second_mismatch) e.dbeta2 = sp.dbeta2;   // ... the second mismatch's own array
        hipError_t he = EpilogueLaunch<T>::fn((hipStream_t)stream, e);
        if (he != hipSuccess) return hip_fail(he, "chain epilogue launch");
        row += e.rows;
        step_off += sp.n_steps;
    }
    return PSA_OK;
}

template <typename Span>
int chain_host(int device, const ChainCall<Span> &c, double *elapsed_ms) {
    using F = Family<Span>;
    using T = typename Span::Real;
    int64_t rows_total = 0;
    int rc = validate_chain(c, true, &rows_total);
    if (rc != PSA_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (c.s.n_points == 0) return PSA_OK;

    const int S = c.n_segments, nc = 2 * F::n_waves(c.s);
    const size_t N = (size_t)c.s.n_points;
    const uint32_t flags = c.s.flags;
    const std::vector<unsigned char> lossless = lossless_spans(flags, c.s.alpha, S, N);
    ChainCall<Span> d = c;
    if (c.s.traj) d.s.flags |= PSA_OPT_TRAJ_LD;   // the device-side trajectory has its own leading dimension; the caller's is dense
    d.lossless = lossless.data();
    const T *tr = S > 1 ? c.transfer : nullptr;
    auto layout = [&](Staging<T> &sg) {
        mismatch_of(d.s) = stage_mismatch(sg, c.s, S, N);
        if constexpr (F::second_mismatch) d.s.dbeta2 = sg.input(c.s.dbeta2, S * N);
        d.s.gamma = sg.input(c.s.gamma, (flags & PSA_BCAST_GAMMA) ? (size_t)S : S * N);
        d.s.alpha = sg.input(c.s.alpha, (flags & PSA_BCAST_ALPHA) ? (size_t)S : S * N);
        d.s.a0 = sg.input_soa(c.s.a0, (flags & PSA_BCAST_A0) ? 1 : N, nc);
        // [S-1][n_waves][2] is already [S-1][2*n_waves]; [S-1][N][n_waves][2] -> [S-1][2*n_waves][N]
        d.transfer = (flags & PSA_BCAST_TRANSFER) ? sg.input(tr, (size_t)(S - 1) * nc) : sg.input_soa(tr, N, nc, S - 1);
        d.workspace = S > 1 ? sg.template scratch<char>(ChainScratch<T>::of(nullptr, c.s).bytes) : nullptr;
        d.s.a_end = sg.output_soa(c.s.a_end, N, nc);
        F::stage_summary(sg, d.s, c.s, N);
        d.s.traj = sg.trajectory(c.s.traj, N, (size_t)rows_total, nc);
    };
    return host_call<T>(device, F::what, elapsed_ms, layout, [&](hipStream_t st) { return chain_dev(st, d); });
}

// the two exported sizes: the same carve, measured; -1 for a call no chain takes
int64_t chain_workspace_bytes(int n_waves, int64_t n_points, size_t elem, bool waves) {
    if ((n_waves != 4 && n_waves != 6) || n_points < 0 || (elem != 4 && elem != 8)) return -1;
    const size_t N = (size_t)n_points;
    return (int64_t)(elem == 8 ? ChainScratch<double>(nullptr, N, n_waves, n_waves == 6, true, waves).bytes
                               : ChainScratch<float>(nullptr, N, n_waves, n_waves == 6, true, waves).bytes);
}
int64_t single_pump_chain_workspace_bytes(int64_t n_points) {
    return n_points < 0 ? -1 : (int64_t)ChainScratch<double>(nullptr, (size_t)n_points, 3, false, false, true).bytes;
}
int64_t pairs_chain_workspace_bytes(int n_pairs, int64_t n_points) {
    if (n_pairs < 1 || n_pairs > PSA_MAX_PAIRS || n_points < 0) return -1;
    return (int64_t)ChainScratch<double>(nullptr, (size_t)n_points, 2 + 2 * n_pairs, false, false, true, n_pairs).bytes;
}
int64_t comb_chain_workspace_bytes(int n_lines, int64_t n_points) {
    if (n_lines < 3 || n_lines > PSA_MAX_LINES || n_points < 0) return -1;
    return (int64_t)ChainScratch<double>(nullptr, (size_t)n_points, n_lines, false, false, true, n_lines).bytes;
}

template <typename T> struct GainLaunch;
template <> struct GainLaunch<double> { static constexpr auto fn = psa::launch_gain_summary_f64; };
template <> struct GainLaunch<float> { static constexpr auto fn = psa::launch_gain_summary_f32; };

template <typename T>
int gain_summary_dev(void *stream, int64_t n, const T *d_p, const int64_t *d_bad, double p0_sig, int gain_db, T *d_gain,
                     int64_t *d_best_i, double *d_best_g, int64_t *d_nfin, void *d_ws) {
    if (n < 0) return fail(PSA_E_NPOINTS, "n_points must be >= 0");
    if (!d_best_i || !d_best_g || !d_nfin || !d_ws || (n > 0 && !d_p))
        return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    hipError_t e = GainLaunch<T>::fn((hipStream_t)stream, n, d_p, (const long long *)d_bad, p0_sig, gain_db, d_gain,
                                     (long long *)d_best_i, d_best_g, (long long *)d_nfin, d_ws);
    if (e != hipSuccess) return hip_fail(e, "gain_summary launch");
    return PSA_OK;
}

template <typename T>
int gain_summary_host(int device, int64_t n, const T *p_metric, const int64_t *first_bad, double p0_sig, int gain_db,
                      T *gain_out, int64_t *best_index, double *best_gain, int64_t *n_finite) {
    if (n < 0) return fail(PSA_E_NPOINTS, "n_points must be >= 0");
    if (!best_index || !best_gain || !n_finite || (n > 0 && !p_metric))
        return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    const size_t N = (size_t)n;
    int64_t scal[3];   // best_index | best_gain (double) | n_finite
    const T *d_p;
    const int64_t *d_bad;
    T *d_gain;
    int64_t *d_scal;
    void *d_ws;
    int rc = host_call<T>(device, "the gain summary", nullptr, [&](Staging<T> &sg) {
        d_p = sg.input(p_metric, N);
        d_bad = sg.input(first_bad, N);
        d_ws = sg.template scratch<char>((size_t)psa::gain_summary_workspace_bytes(n));
        d_gain = sg.output(gain_out, N);
        d_scal = sg.output(scal, 3);
    }, [&](hipStream_t st) {
        return gain_summary_dev<T>(st, n, d_p, d_bad, p0_sig, gain_db, d_gain, d_scal, (double *)(d_scal + 1), d_scal + 2, d_ws);
    });
    if (rc != PSA_OK) return rc;
    *best_index = scal[0];
    std::memcpy(best_gain, &scal[1], 8);
    *n_finite = scal[2];
    return PSA_OK;
}

// dbeta producer: argument checks + the model struct shared by both kernels
int make_dbeta_model(psa::DbetaModel &m, int method, const int32_t *orders, int n_orders, int max_order,
                     const double *beta, int n_beta, double omega_ref, double two_pi_c, double atol, double rtol) {
    if (method != PSA_DBETA_SYMMETRIC_EVEN && method != PSA_DBETA_GENERAL_TAYLOR)
        return fail(PSA_E_DBETA_MODEL, "method must be PSA_DBETA_SYMMETRIC_EVEN or PSA_DBETA_GENERAL_TAYLOR");
    if (!beta || n_beta < 1 || n_beta > psa::DBETA_MAX_ORDER + 1)
        return fail(PSA_E_DBETA_MODEL, "beta must hold 1..%d coefficients", psa::DBETA_MAX_ORDER + 1);
    for (int n = 0; n <= psa::DBETA_MAX_ORDER; ++n) m.beta[n] = n < n_beta ? beta[n] : 0.0;
    m.omega_ref = omega_ref; m.two_pi_c = two_pi_c; m.atol = atol; m.rtol = rtol;
    m.method = method; m.n_orders = 0; m.max_order = 0;
    for (int k = 0; k < 4; ++k) m.orders[k] = 0;
    if (method == PSA_DBETA_SYMMETRIC_EVEN) {
        if (!orders || n_orders < 1 || n_orders > 4) return fail(PSA_E_DBETA_MODEL, "1..4 even orders expected");
        for (int k = 0; k < n_orders; ++k) {
            if (orders[k] < 2 || orders[k] % 2 || orders[k] > psa::DBETA_MAX_ORDER)
                return fail(PSA_E_DBETA_MODEL, "even_orders must be even ints in [2, %d], got %d", psa::DBETA_MAX_ORDER, orders[k]);
            m.orders[k] = orders[k];
        }
        m.n_orders = n_orders;
    } else {
        if (max_order < 0 || max_order > psa::DBETA_MAX_ORDER)
            return fail(PSA_E_DBETA_MODEL, "max_order must be in [0, %d]", psa::DBETA_MAX_ORDER);
        m.max_order = max_order;
    }
    return PSA_OK;
}

template <typename T> struct DbetaLaunch;
template <> struct DbetaLaunch<double> {
    static constexpr auto grid = psa::launch_dbeta_grid_f64;
    static constexpr auto pairs = psa::launch_dbeta_pairs_f64;
};
template <> struct DbetaLaunch<float> {
    static constexpr auto grid = psa::launch_dbeta_grid_f32;
    static constexpr auto pairs = psa::launch_dbeta_pairs_f32;
};

template <typename T>
int dbeta_grid_dev(void *stream, int method, const int32_t *orders, int n_orders, int max_order, const double *beta,
                   int n_beta, double omega_ref, double two_pi_c, double atol, double rtol, double lambda1_m,
                   const double *d_ax2, int64_t n2, const double *d_ax3, int64_t n3, int64_t first, int64_t n, T *d_out,
                   uint8_t *d_valid) {
    psa::DbetaModel m;
    int rc = make_dbeta_model(m, method, orders, n_orders, max_order, beta, n_beta, omega_ref, two_pi_c, atol, rtol);
    if (rc != PSA_OK) return rc;
    if (n < 0 || n2 <= 0 || n3 <= 0 || first < 0) return fail(PSA_E_NPOINTS, "n_points / axes / first_index out of range");
    if ((long double)first + (long double)n > (long double)n2 * (long double)n3)
        return fail(PSA_E_NPOINTS, "[first_index, first_index + n_points) leaves the %lld x %lld grid", (long long)n2, (long long)n3);
    if (n == 0) return PSA_OK;
    if (!d_ax2 || !d_ax3 || !d_out) return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    hipError_t e = DbetaLaunch<T>::grid((hipStream_t)stream, m, lambda1_m, d_ax2, n2, d_ax3, n3, first, n, d_out, d_valid);
    if (e != hipSuccess) return hip_fail(e, "dbeta_grid launch");
    return PSA_OK;
}

template <typename T>
int dbeta_pairs_dev(void *stream, const int32_t *orders, int n_orders, const double *beta, int n_beta, double omega_d,
                    const double *d_ax1, int64_t n1, const double *d_ax2, int64_t n2, int64_t first, int64_t n,
                    T *d_out1, T *d_out2) {
    psa::DbetaModel m;
    int rc = make_dbeta_model(m, PSA_DBETA_SYMMETRIC_EVEN, orders, n_orders, 0, beta, n_beta, 1.0, 0.0, 0.0, 0.0);
    if (rc != PSA_OK) return rc;
    if (n < 0 || n1 <= 0 || n2 <= 0 || first < 0) return fail(PSA_E_NPOINTS, "n_points / axes / first_index out of range");
    if ((long double)first + (long double)n > (long double)n1 * (long double)n2)
        return fail(PSA_E_NPOINTS, "[first_index, first_index + n_points) leaves the %lld x %lld grid", (long long)n1, (long long)n2);
    if (n == 0) return PSA_OK;
    if (!d_ax1 || !d_ax2 || !d_out1 || !d_out2) return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    hipError_t e = DbetaLaunch<T>::pairs((hipStream_t)stream, m, omega_d, d_ax1, n1, d_ax2, n2, first, n, d_out1, d_out2);
    if (e != hipSuccess) return hip_fail(e, "dbeta_pairs launch");
    return PSA_OK;
}

// ---- the adaptive (RK45) sweep ----------------------------------------------------------------------------------
// Argument rules of psa_rk45_sweep_*: those of the sweep (validate_common, with one step and a stride of one standing in
// for the grid an adaptive run does not have), the flags it takes, the tolerances, the extra outputs and the row count.
int validate_rk45(const Rk45Call &c) {
    // status stands in for first_bad_step: the sweep's rules only ask whether it is NULL
    const SweepCall<double> as_sweep{c.n_waves, c.n_points, 1, c.z_max, 1, c.dbeta, c.dbeta2, c.gamma, c.alpha, c.a0, 0u,
                                     c.a_end, c.p_end, c.p_max, reinterpret_cast<int64_t *>(c.status), c.traj};
    int rc = validate_common(as_sweep);
    if (rc != PSA_OK) return rc;
    const uint32_t allowed = PSA_BCAST_GAMMA | PSA_BCAST_ALPHA | PSA_BCAST_A0 | PSA_OPT_LOSSLESS;
    if (c.flags & ~allowed)
        return fail(PSA_E_FLAGS, "the adaptive sweep takes PSA_BCAST_GAMMA/ALPHA/A0 and PSA_OPT_LOSSLESS only, got 0x%x",
                    c.flags);
    if (!(c.rtol >= 100.0 * 2.220446049250313e-16) || !std::isfinite(c.rtol))
        return fail(PSA_E_TOL, "rtol must be finite and >= 100 * DBL_EPSILON");
    if (!(c.atol > 0.0) || !std::isfinite(c.atol)) return fail(PSA_E_TOL, "atol must be positive and finite");
    if (!(c.h_max > 0.0)) return fail(PSA_E_TOL, "h_max must be positive");
    if (!(c.first_step >= 0.0) || !std::isfinite(c.first_step))
        return fail(PSA_E_TOL, "first_step must be >= 0 and finite (0: select it)");
    if (c.max_steps < 1) return fail(PSA_E_TOL, "max_steps must be >= 1, got %lld", (long long)c.max_steps);
    if (c.n_out < 0) return fail(PSA_E_TOL, "n_out must be >= 0, got %lld", (long long)c.n_out);
    if (c.n_points > 0 && (!c.z_end || !c.n_acc || !c.n_rej)) return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    if (c.traj && ((long double)c.n_out + 1.0L) * (long double)c.n_points * (2.0L * c.n_waves) * sizeof(double) > 4.0e18L)
        return fail(PSA_E_TOO_LARGE, "dense-output buffer too large");
    return PSA_OK;
}

int rk45_dev(void *stream, const Rk45Call &c) {
    int rc = validate_rk45(c);
    if (rc != PSA_OK) return rc;
    if (c.n_points == 0) return PSA_OK;
    psa::AdaptiveArgs<double> a;
    fill_point_args(a, c);
    a.dbeta2 = c.dbeta2;
    a.p_end = c.p_end;
    a.p_max = c.p_max;
    a.status = c.status;
    a.z_end = c.z_end;
    a.n_accepted = (long long *)c.n_acc;
    a.n_rejected = (long long *)c.n_rej;
    a.traj = c.traj;
    a.traj_ld = c.traj_ld;
    a.rtol = c.rtol;
    a.atol = c.atol;
    a.h_max = c.h_max;
    a.first_step = c.first_step;
    a.max_steps = c.max_steps;
    a.n_out = c.n_out;
    hipError_t e = psa::launch_rk45_sweep_f64((hipStream_t)stream, c.n_waves, c.flags, a);
    if (e != hipSuccess) return hip_fail(e, "rk45_sweep launch");
    return PSA_OK;
}

int rk45_host(int device, const Rk45Call &c, double *elapsed_ms) {
    int rc = validate_rk45(c);
    if (rc != PSA_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (c.n_points == 0) return PSA_OK;
    const int nc = 2 * c.n_waves;
    const size_t N = (size_t)c.n_points;
    Rk45Call d = c;
    d.flags |= lossless_bit(c.flags, c.alpha);
    d.traj_ld = traj_ld_of(c.n_points, sizeof(double));
    auto layout = [&](Staging<double> &sg) {
        d.dbeta = sg.input(c.dbeta, N);
        d.dbeta2 = sg.input(c.dbeta2, N);
        d.gamma = sg.input(c.gamma, (c.flags & PSA_BCAST_GAMMA) ? 1 : N);
        d.alpha = sg.input(c.alpha, (c.flags & PSA_BCAST_ALPHA) ? 1 : N);
        d.a0 = sg.input_soa(c.a0, (c.flags & PSA_BCAST_A0) ? 1 : N, nc);
        d.a_end = sg.output_soa(c.a_end, N, nc);
        d.p_end = sg.output(c.p_end, N);
        d.p_max = sg.output(c.p_max, N);
        d.status = sg.output(c.status, N);
        d.z_end = sg.output(c.z_end, N);
        d.n_acc = sg.output(c.n_acc, N);
        d.n_rej = sg.output(c.n_rej, N);
        d.traj = sg.trajectory(c.traj, N, (size_t)c.n_out + 1, nc);
    };
    return host_call<double>(device, "the RK45 sweep", elapsed_ms, layout, [&](hipStream_t st) { return rk45_dev(st, d); });
}

}  // namespace

extern "C" {

int psa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
const char *psa_last_error(void) { return g_err; }
const char *psa_version(void) { return "psa-hip 0.3.0 gfx950"; }
int64_t psa_n_saved(int64_t n_steps, int32_t save_every) {
    if (n_steps < 0 || save_every <= 0) return -1;
    return n_steps / save_every + 1;
}
int64_t psa_traj_ld(int64_t n_points, int32_t elem_size) {
    if (n_points < 0 || (elem_size != 4 && elem_size != 8)) return -1;
    return traj_ld_of(n_points, (size_t)elem_size);
}
int psa_release_cache(void) {
    std::vector<HostCtx *> idle;
    {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        idle.swap(g_ctx_idle);
    }
    int prev = -1;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    for (HostCtx *c : idle) {
        if (hipSetDevice(c->device) == hipSuccess) c->destroy();
        delete c;
    }
    if (have_prev) (void)hipSetDevice(prev);
    return (int)idle.size();
}

int psa_rk4_sweep_f64(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                      const double *dbeta, const double *dbeta2, const double *gamma, const double *alpha,
                      const double *a0, uint32_t flags, double *a_end, double *p_end, double *p_max,
                      int64_t *first_bad, double *traj, double *elapsed_ms) {
    return sweep_host<double>(device, {n_waves, n_points, n_steps, z_max, save_every, dbeta, dbeta2, gamma, alpha, a0, flags,
                                       a_end, p_end, p_max, first_bad, traj}, elapsed_ms);
}
int psa_rk4_sweep_f32(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                      const float *dbeta, const float *dbeta2, const float *gamma, const float *alpha, const float *a0,
                      uint32_t flags, float *a_end, float *p_end, float *p_max, int64_t *first_bad, float *traj,
                      double *elapsed_ms) {
    return sweep_host<float>(device, {n_waves, n_points, n_steps, z_max, save_every, dbeta, dbeta2, gamma, alpha, a0, flags,
                                      a_end, p_end, p_max, first_bad, traj}, elapsed_ms);
}
int psa_rk4_sweep_f64_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                          int32_t save_every, const double *d_dbeta, const double *d_dbeta2, const double *d_gamma,
                          const double *d_alpha, const double *d_a0_soa, uint32_t flags, double *d_a_end_soa,
                          double *d_p_end, double *d_p_max, int64_t *d_first_bad, double *d_traj_soa) {
    return sweep_dev<double>(stream, {n_waves, n_points, n_steps, z_max, save_every, d_dbeta, d_dbeta2, d_gamma, d_alpha,
                                      d_a0_soa, flags, d_a_end_soa, d_p_end, d_p_max, d_first_bad, d_traj_soa});
}
int psa_rk4_sweep_f32_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                          int32_t save_every, const float *d_dbeta, const float *d_dbeta2, const float *d_gamma,
                          const float *d_alpha, const float *d_a0_soa, uint32_t flags, float *d_a_end_soa,
                          float *d_p_end, float *d_p_max, int64_t *d_first_bad, float *d_traj_soa) {
    return sweep_dev<float>(stream, {n_waves, n_points, n_steps, z_max, save_every, d_dbeta, d_dbeta2, d_gamma, d_alpha,
                                     d_a0_soa, flags, d_a_end_soa, d_p_end, d_p_max, d_first_bad, d_traj_soa});
}

int psa_rk4_sweep_waves_f64(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                            const double *dbeta, const double *dbeta2, const double *gamma, const double *alpha,
                            const double *a0, uint32_t flags, double *a_end, double *p_end, double *p_max,
                            int64_t *first_bad, double *traj, double *elapsed_ms, double *p_wave_end, double *p_wave_max) {
    return sweep_host<double>(device, {n_waves, n_points, n_steps, z_max, save_every, dbeta, dbeta2, gamma, alpha, a0, flags,
                                       a_end, p_end, p_max, first_bad, traj, p_wave_end, p_wave_max, true}, elapsed_ms);
}
int psa_rk4_sweep_waves_f32(int device, int n_waves, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                            const float *dbeta, const float *dbeta2, const float *gamma, const float *alpha,
                            const float *a0, uint32_t flags, float *a_end, float *p_end, float *p_max,
                            int64_t *first_bad, float *traj, double *elapsed_ms, float *p_wave_end, float *p_wave_max) {
    return sweep_host<float>(device, {n_waves, n_points, n_steps, z_max, save_every, dbeta, dbeta2, gamma, alpha, a0, flags,
                                      a_end, p_end, p_max, first_bad, traj, p_wave_end, p_wave_max, true}, elapsed_ms);
}
int psa_rk4_sweep_waves_f64_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                                int32_t save_every, const double *d_dbeta, const double *d_dbeta2, const double *d_gamma,
                                const double *d_alpha, const double *d_a0_soa, uint32_t flags, double *d_a_end_soa,
                                double *d_p_end, double *d_p_max, int64_t *d_first_bad, double *d_traj_soa,
                                double *d_p_wave_end_soa, double *d_p_wave_max_soa) {
    return sweep_dev<double>(stream, {n_waves, n_points, n_steps, z_max, save_every, d_dbeta, d_dbeta2, d_gamma, d_alpha,
                                      d_a0_soa, flags, d_a_end_soa, d_p_end, d_p_max, d_first_bad, d_traj_soa, d_p_wave_end_soa,
                                      d_p_wave_max_soa, true});
}
int psa_rk4_sweep_waves_f32_dev(void *stream, int n_waves, int64_t n_points, int64_t n_steps, double z_max,
                                int32_t save_every, const float *d_dbeta, const float *d_dbeta2, const float *d_gamma,
                                const float *d_alpha, const float *d_a0_soa, uint32_t flags, float *d_a_end_soa,
                                float *d_p_end, float *d_p_max, int64_t *d_first_bad, float *d_traj_soa,
                                float *d_p_wave_end_soa, float *d_p_wave_max_soa) {
    return sweep_dev<float>(stream, {n_waves, n_points, n_steps, z_max, save_every, d_dbeta, d_dbeta2, d_gamma, d_alpha,
                                     d_a0_soa, flags, d_a_end_soa, d_p_end, d_p_max, d_first_bad, d_traj_soa, d_p_wave_end_soa,
                                     d_p_wave_max_soa, true});
}

int psa_yaman_rhs_f64(int device, int64_t n, const double *z, const double *a, const double *gamma,
                      const double *alpha, const double *dbeta, double *out, double *out_lin, double *out_kerr,
                      double *out_fwm) {
    if (n < 0) return fail(PSA_E_NPOINTS, "n_points must be >= 0");
    if (n == 0) return PSA_OK;
    if (!z || !a || !gamma || !alpha || !dbeta || !out) return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    const size_t N = (size_t)n;
    const double *d_z, *d_a, *d_gamma, *d_alpha, *d_dbeta;
    double *d_out, *d_lin, *d_kerr, *d_fwm;
    return host_call<double>(device, "the RHS kernel", nullptr, [&](Staging<double> &sg) {
        d_z = sg.input(z, N);
        d_a = sg.input(a, 8 * N);
        d_gamma = sg.input(gamma, N);
        d_alpha = sg.input(alpha, N);
        d_dbeta = sg.input(dbeta, N);
        d_out = sg.output(out, 8 * N);
        d_lin = sg.output(out_lin, 8 * N);
        d_kerr = sg.output(out_kerr, 8 * N);
        d_fwm = sg.output(out_fwm, 8 * N);
    }, [&](hipStream_t st) {
        hipError_t e = psa::launch_yaman_rhs_f64(st, n, d_z, d_a, d_gamma, d_alpha, d_dbeta, d_out, d_lin, d_kerr, d_fwm);
        return e == hipSuccess ? PSA_OK : hip_fail(e, "yaman_rhs launch");
    });
}

int64_t psa_gain_summary_workspace_bytes(int64_t n) { return psa::gain_summary_workspace_bytes(n); }

int psa_gain_summary_f64_dev(void *stream, int64_t n, const double *d_p, const int64_t *d_bad, double p0_sig,
                             int gain_db, double *d_gain, int64_t *d_best_i, double *d_best_g, int64_t *d_nfin,
                             void *d_ws) {
    return gain_summary_dev<double>(stream, n, d_p, d_bad, p0_sig, gain_db, d_gain, d_best_i, d_best_g, d_nfin, d_ws);
}
int psa_gain_summary_f32_dev(void *stream, int64_t n, const float *d_p, const int64_t *d_bad, double p0_sig,
                             int gain_db, float *d_gain, int64_t *d_best_i, double *d_best_g, int64_t *d_nfin,
                             void *d_ws) {
    return gain_summary_dev<float>(stream, n, d_p, d_bad, p0_sig, gain_db, d_gain, d_best_i, d_best_g, d_nfin, d_ws);
}
int psa_gain_summary_f64(int device, int64_t n, const double *p_metric, const int64_t *first_bad, double p0_sig,
                         int gain_db, double *gain_out, int64_t *best_index, double *best_gain, int64_t *n_finite) {
    return gain_summary_host<double>(device, n, p_metric, first_bad, p0_sig, gain_db, gain_out, best_index, best_gain, n_finite);
}
int psa_gain_summary_f32(int device, int64_t n, const float *p_metric, const int64_t *first_bad, double p0_sig,
                         int gain_db, float *gain_out, int64_t *best_index, double *best_gain, int64_t *n_finite) {
    return gain_summary_host<float>(device, n, p_metric, first_bad, p0_sig, gain_db, gain_out, best_index, best_gain, n_finite);
}

/* ---- device-side dbeta producer ---------------------------------------------------------------------------- */
int psa_dbeta_grid_f64_dev(void *stream, int method, const int32_t *orders, int n_orders, int max_order,
                           const double *beta, int n_beta, double omega_ref, double two_pi_c, double atol, double rtol,
                           double lambda1_m, const double *d_lambda2_axis, int64_t n2, const double *d_lambda3_axis,
                           int64_t n3, int64_t first_index, int64_t n_points, double *d_dbeta, uint8_t *d_valid) {
    return dbeta_grid_dev<double>(stream, method, orders, n_orders, max_order, beta, n_beta, omega_ref, two_pi_c, atol,
                                  rtol, lambda1_m, d_lambda2_axis, n2, d_lambda3_axis, n3, first_index, n_points, d_dbeta,
                                  d_valid);
}
int psa_dbeta_grid_f32_dev(void *stream, int method, const int32_t *orders, int n_orders, int max_order,
                           const double *beta, int n_beta, double omega_ref, double two_pi_c, double atol, double rtol,
                           double lambda1_m, const double *d_lambda2_axis, int64_t n2, const double *d_lambda3_axis,
                           int64_t n3, int64_t first_index, int64_t n_points, float *d_dbeta, uint8_t *d_valid) {
    return dbeta_grid_dev<float>(stream, method, orders, n_orders, max_order, beta, n_beta, omega_ref, two_pi_c, atol,
                                 rtol, lambda1_m, d_lambda2_axis, n2, d_lambda3_axis, n3, first_index, n_points, d_dbeta,
                                 d_valid);
}
int psa_dbeta_pairs_f64_dev(void *stream, const int32_t *orders, int n_orders, const double *beta, int n_beta,
                            double omega_d, const double *d_Omega1_axis, int64_t n1, const double *d_Omega2_axis,
                            int64_t n2, int64_t first_index, int64_t n_points, double *d_dbeta1, double *d_dbeta2) {
    return dbeta_pairs_dev<double>(stream, orders, n_orders, beta, n_beta, omega_d, d_Omega1_axis, n1, d_Omega2_axis, n2,
                                   first_index, n_points, d_dbeta1, d_dbeta2);
}
int psa_dbeta_pairs_f32_dev(void *stream, const int32_t *orders, int n_orders, const double *beta, int n_beta,
                            double omega_d, const double *d_Omega1_axis, int64_t n1, const double *d_Omega2_axis,
                            int64_t n2, int64_t first_index, int64_t n_points, float *d_dbeta1, float *d_dbeta2) {
    return dbeta_pairs_dev<float>(stream, orders, n_orders, beta, n_beta, omega_d, d_Omega1_axis, n1, d_Omega2_axis, n2,
                                  first_index, n_points, d_dbeta1, d_dbeta2);
}

int psa_dbeta_grid_f64(int device, int method, const int32_t *orders, int n_orders, int max_order, const double *beta,
                       int n_beta, double omega_ref, double two_pi_c, double atol, double rtol, double lambda1_m,
                       const double *lambda2_axis, int64_t n2, const double *lambda3_axis, int64_t n3,
                       int64_t first_index, int64_t n_points, double *dbeta, uint8_t *valid) {
    if (n_points < 0 || n2 <= 0 || n3 <= 0) return fail(PSA_E_NPOINTS, "n_points must be >= 0 and the axes non-empty");
    if (!lambda2_axis || !lambda3_axis || (n_points > 0 && !dbeta)) return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    if (n_points == 0) return check_device(device, "the dbeta producer");
    const size_t N = (size_t)n_points;
    const double *d_ax2, *d_ax3;
    double *d_out;
    uint8_t *d_valid;
    return host_call<double>(device, "the dbeta producer", nullptr, [&](Staging<double> &sg) {
        d_ax2 = sg.input(lambda2_axis, (size_t)n2);
        d_ax3 = sg.input(lambda3_axis, (size_t)n3);
        d_out = sg.output(dbeta, N);
        d_valid = sg.output(valid, N);
    }, [&](hipStream_t st) {
        return dbeta_grid_dev<double>(st, method, orders, n_orders, max_order, beta, n_beta, omega_ref, two_pi_c, atol, rtol,
                                      lambda1_m, d_ax2, n2, d_ax3, n3, first_index, n_points, d_out, d_valid);
    });
}

int psa_dbeta_pairs_f64(int device, const int32_t *orders, int n_orders, const double *beta, int n_beta, double omega_d,
                        const double *Omega1_axis, int64_t n1, const double *Omega2_axis, int64_t n2,
                        int64_t first_index, int64_t n_points, double *dbeta1, double *dbeta2) {
    if (n_points < 0 || n1 <= 0 || n2 <= 0) return fail(PSA_E_NPOINTS, "n_points must be >= 0 and the axes non-empty");
    if (!Omega1_axis || !Omega2_axis || (n_points > 0 && (!dbeta1 || !dbeta2))) return fail(PSA_E_NULLPTR, "a required buffer pointer is NULL");
    if (n_points == 0) return check_device(device, "the dbeta producer");
    const size_t N = (size_t)n_points;
    const double *d_ax1, *d_ax2;
    double *d_out1, *d_out2;
    return host_call<double>(device, "the dbeta producer", nullptr, [&](Staging<double> &sg) {
        d_ax1 = sg.input(Omega1_axis, (size_t)n1);
        d_ax2 = sg.input(Omega2_axis, (size_t)n2);
        d_out1 = sg.output(dbeta1, N);
        d_out2 = sg.output(dbeta2, N);
    }, [&](hipStream_t st) {
        return dbeta_pairs_dev<double>(st, orders, n_orders, beta, n_beta, omega_d, d_ax1, n1, d_ax2, n2, first_index,
                                       n_points, d_out1, d_out2);
    });
}

// the chain's record: the spans' shared part has no grid of its own (n_steps 0, z_max 0: set span by span)
int psa_rk4_chain_f64(int device, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                      const double *seg_len, int32_t save_every, const double *dbeta, const double *dbeta2, const double *gamma,
                      const double *alpha, const double *a0, const double *transfer, uint32_t flags, double *a_end, double *p_end,
                      double *p_max, int64_t *first_bad, double *traj, double *elapsed_ms, double *p_wave_end, double *p_wave_max) {
    return chain_host<SweepCall<double>>(device, {{n_waves, n_points, 0, 0.0, save_every, dbeta, dbeta2, gamma, alpha, a0, flags, a_end,
                                       p_end, p_max, first_bad, traj, p_wave_end, p_wave_max}, n_segments, n_steps, seg_len,
                                       transfer, nullptr}, elapsed_ms);
}

int psa_rk4_chain_f64_dev(void *stream, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                          const double *seg_len, int32_t save_every, const double *d_dbeta, const double *d_dbeta2,
                          const double *d_gamma, const double *d_alpha, const double *d_a0_soa, const double *d_transfer_soa,
                          uint32_t flags, double *d_a_end_soa, double *d_p_end, double *d_p_max, int64_t *d_first_bad,
                          double *d_traj_soa, double *d_p_wave_end_soa, double *d_p_wave_max_soa, void *d_workspace) {
    return chain_dev<SweepCall<double>>(stream, {{n_waves, n_points, 0, 0.0, save_every, d_dbeta, d_dbeta2, d_gamma, d_alpha, d_a0_soa,
                                      flags, d_a_end_soa, d_p_end, d_p_max, d_first_bad, d_traj_soa, d_p_wave_end_soa,
                                      d_p_wave_max_soa}, n_segments, n_steps, seg_len, d_transfer_soa, d_workspace});
}

int psa_rk4_chain_f32(int device, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                      const double *seg_len, int32_t save_every, const float *dbeta, const float *dbeta2, const float *gamma,
                      const float *alpha, const float *a0, const float *transfer, uint32_t flags, float *a_end, float *p_end,
                      float *p_max, int64_t *first_bad, float *traj, double *elapsed_ms, float *p_wave_end, float *p_wave_max) {
    return chain_host<SweepCall<float>>(device, {{n_waves, n_points, 0, 0.0, save_every, dbeta, dbeta2, gamma, alpha, a0, flags, a_end,
                                      p_end, p_max, first_bad, traj, p_wave_end, p_wave_max}, n_segments, n_steps, seg_len,
                                      transfer, nullptr}, elapsed_ms);
}

int psa_rk4_chain_f32_dev(void *stream, int n_waves, int64_t n_points, int n_segments, const int64_t *n_steps,
                          const double *seg_len, int32_t save_every, const float *d_dbeta, const float *d_dbeta2,
                          const float *d_gamma, const float *d_alpha, const float *d_a0_soa, const float *d_transfer_soa,
                          uint32_t flags, float *d_a_end_soa, float *d_p_end, float *d_p_max, int64_t *d_first_bad,
                          float *d_traj_soa, float *d_p_wave_end_soa, float *d_p_wave_max_soa, void *d_workspace) {
    return chain_dev<SweepCall<float>>(stream, {{n_waves, n_points, 0, 0.0, save_every, d_dbeta, d_dbeta2, d_gamma, d_alpha, d_a0_soa,
                                     flags, d_a_end_soa, d_p_end, d_p_max, d_first_bad, d_traj_soa, d_p_wave_end_soa,
                                     d_p_wave_max_soa}, n_segments, n_steps, seg_len, d_transfer_soa, d_workspace});
}

int64_t psa_rk4_chain_workspace_bytes(int n_waves, int64_t n_points, int32_t elem_size, int wave_summary) {
    return chain_workspace_bytes(n_waves, n_points, (size_t)(elem_size > 0 ? elem_size : 0), wave_summary != 0);
}

int psa_rk45_sweep_f64(int device, int n_waves, int64_t n_points, double z_max, double rtol, double atol, double h_max,
                       double first_step, int64_t max_steps, int64_t n_out, const double *dbeta, const double *dbeta2,
                       const double *gamma, const double *alpha, const double *a0_re_im, uint32_t flags,
                       double *a_end_re_im, double *p_sig_end, double *p_sig_max, int32_t *status, double *z_end,
                       int64_t *n_accepted, int64_t *n_rejected, double *traj_or_null, double *elapsed_ms_or_null) {
    return rk45_host(device, {n_waves, n_points, z_max, rtol, atol, h_max, first_step, max_steps, n_out, dbeta, dbeta2, gamma,
                              alpha, a0_re_im, flags, a_end_re_im, p_sig_end, p_sig_max, status, z_end, n_accepted, n_rejected,
                              traj_or_null, n_points}, elapsed_ms_or_null);
}
int psa_rk45_sweep_f64_dev(void *stream, int n_waves, int64_t n_points, double z_max, double rtol, double atol,
                           double h_max, double first_step, int64_t max_steps, int64_t n_out, const double *d_dbeta,
                           const double *d_dbeta2, const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                           uint32_t flags, double *d_a_end_soa, double *d_p_sig_end, double *d_p_sig_max,
                           int32_t *d_status, double *d_z_end, int64_t *d_n_accepted, int64_t *d_n_rejected,
                           double *d_traj_soa) {
    return rk45_dev(stream, {n_waves, n_points, z_max, rtol, atol, h_max, first_step, max_steps, n_out, d_dbeta, d_dbeta2,
                             d_gamma, d_alpha, d_a0_soa, flags, d_a_end_soa, d_p_sig_end, d_p_sig_max, d_status, d_z_end,
                             d_n_accepted, d_n_rejected, d_traj_soa, n_points});
}

int psa_rk4_sweep_pairs_f64(int device, int n_pairs, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                            const double *dbeta, const double *gamma, const double *alpha, const double *a0_re_im,
                            uint32_t flags, double *a_end_re_im, double *p_wave_end, double *p_wave_max,
                            int64_t *first_bad_step, double *elapsed_ms_or_null) {
    return wave_host(device, PairsCall{n_pairs, n_points, n_steps, z_max, save_every, dbeta, gamma, alpha, a0_re_im, flags, a_end_re_im,
                               p_wave_end, p_wave_max, first_bad_step}, elapsed_ms_or_null);
}
int psa_rk4_sweep_pairs_f64_dev(void *stream, int n_pairs, int64_t n_points, int64_t n_steps, double z_max,
                                int32_t save_every, const double *d_dbeta_soa, const double *d_gamma, const double *d_alpha,
                                const double *d_a0_soa, uint32_t flags, double *d_a_end_soa, double *d_p_wave_end_soa,
                                double *d_p_wave_max_soa, int64_t *d_first_bad_step) {
    return wave_dev(stream, PairsCall{n_pairs, n_points, n_steps, z_max, save_every, d_dbeta_soa, d_gamma, d_alpha, d_a0_soa, flags,
                              d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step});
}


int psa_rk4_single_pump_f64(int device, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                            const double *dbeta, const double *gamma, const double *alpha, const double *a0_re_im,
                            uint32_t flags, double *a_end_re_im, double *p_wave_end, double *p_wave_max,
                            int64_t *first_bad_step, double *traj_or_null, double *elapsed_ms_or_null) {
    return wave_host(device, SinglePumpCall<double>{n_points, n_steps, z_max, save_every, dbeta, gamma, alpha, a0_re_im, flags,
                                                            a_end_re_im, p_wave_end, p_wave_max, first_bad_step, traj_or_null},
                            elapsed_ms_or_null);
}
int psa_rk4_single_pump_f64_dev(void *stream, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                                const double *d_dbeta, const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                                uint32_t flags, double *d_a_end_soa, double *d_p_wave_end_soa, double *d_p_wave_max_soa,
                                int64_t *d_first_bad_step, double *d_traj_soa_or_null) {
    return wave_dev(stream, SinglePumpCall<double>{n_points, n_steps, z_max, save_every, d_dbeta, d_gamma, d_alpha, d_a0_soa,
                                                          flags, d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step,
                                                          d_traj_soa_or_null});
}
int psa_rk4_single_pump_f32(int device, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                            const float *dbeta, const float *gamma, const float *alpha, const float *a0_re_im,
                            uint32_t flags, float *a_end_re_im, float *p_wave_end, float *p_wave_max,
                            int64_t *first_bad_step, float *traj_or_null, double *elapsed_ms_or_null) {
    return wave_host(device, SinglePumpCall<float>{n_points, n_steps, z_max, save_every, dbeta, gamma, alpha, a0_re_im, flags,
                                                           a_end_re_im, p_wave_end, p_wave_max, first_bad_step, traj_or_null},
                            elapsed_ms_or_null);
}
int psa_rk4_single_pump_f32_dev(void *stream, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                                const float *d_dbeta, const float *d_gamma, const float *d_alpha, const float *d_a0_soa,
                                uint32_t flags, float *d_a_end_soa, float *d_p_wave_end_soa, float *d_p_wave_max_soa,
                                int64_t *d_first_bad_step, float *d_traj_soa_or_null) {
    return wave_dev(stream, SinglePumpCall<float>{n_points, n_steps, z_max, save_every, d_dbeta, d_gamma, d_alpha, d_a0_soa,
                                                         flags, d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step,
                                                         d_traj_soa_or_null});
}

// the chain's record: the spans' shared part has no grid of its own (n_steps 0, z_max 0: set span by span)
int psa_rk4_single_pump_chain_f64(int device, int64_t n_points, int n_segments, const int64_t *n_steps, const double *seg_len,
                                  int32_t save_every, const double *dbeta, const double *gamma, const double *alpha,
                                  const double *a0_re_im, const double *transfer_re_im, uint32_t flags, double *a_end_re_im,
                                  double *p_wave_end, double *p_wave_max, int64_t *first_bad_step, double *traj_or_null,
                                  double *elapsed_ms_or_null) {
    return chain_host<SinglePumpCall<double>>(device, {{n_points, 0, 0.0, save_every, dbeta, gamma, alpha, a0_re_im, flags, a_end_re_im,
                                            p_wave_end, p_wave_max, first_bad_step, traj_or_null}, n_segments, n_steps,
                                           seg_len, transfer_re_im, nullptr}, elapsed_ms_or_null);
}
int psa_rk4_single_pump_chain_f64_dev(void *stream, int64_t n_points, int n_segments, const int64_t *n_steps,
                                      const double *seg_len, int32_t save_every, const double *d_dbeta, const double *d_gamma,
                                      const double *d_alpha, const double *d_a0_soa, const double *d_transfer_soa,
                                      uint32_t flags, double *d_a_end_soa, double *d_p_wave_end_soa, double *d_p_wave_max_soa,
                                      int64_t *d_first_bad_step, double *d_traj_soa_or_null, void *d_workspace) {
    return chain_dev<SinglePumpCall<double>>(stream, {{n_points, 0, 0.0, save_every, d_dbeta, d_gamma, d_alpha, d_a0_soa, flags,
                                           d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step,
                                           d_traj_soa_or_null}, n_segments, n_steps, seg_len, d_transfer_soa, d_workspace});
}
int64_t psa_rk4_single_pump_chain_workspace_bytes(int64_t n_points) { return single_pump_chain_workspace_bytes(n_points); }

int psa_rk4_pairs_chain_f64(int device, int n_pairs, int64_t n_points, int n_segments, const int64_t *n_steps, const double *seg_len,
                            int32_t save_every, const double *dbeta, const double *gamma, const double *alpha,
                            const double *a0_re_im, const double *transfer_re_im, uint32_t flags, double *a_end_re_im,
                            double *p_wave_end, double *p_wave_max, int64_t *first_bad_step, double *traj_or_null,
                            double *elapsed_ms_or_null) {
    return chain_host<PairsCall>(device, {{n_pairs, n_points, 0, 0.0, save_every, dbeta, gamma, alpha, a0_re_im, flags, a_end_re_im,
                                          p_wave_end, p_wave_max, first_bad_step, traj_or_null},
                                         n_segments, n_steps, seg_len, transfer_re_im, nullptr}, elapsed_ms_or_null);
}
int psa_rk4_pairs_chain_f64_dev(void *stream, int n_pairs, int64_t n_points, int n_segments, const int64_t *n_steps,
                                const double *seg_len, int32_t save_every, const double *d_dbeta_soa, const double *d_gamma,
                                const double *d_alpha, const double *d_a0_soa, const double *d_transfer_soa, uint32_t flags,
                                double *d_a_end_soa, double *d_p_wave_end_soa, double *d_p_wave_max_soa,
                                int64_t *d_first_bad_step, double *d_traj_soa_or_null, void *d_workspace) {
    return chain_dev<PairsCall>(stream, {{n_pairs, n_points, 0, 0.0, save_every, d_dbeta_soa, d_gamma, d_alpha, d_a0_soa, flags,
                                         d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step, d_traj_soa_or_null},
                                        n_segments, n_steps, seg_len, d_transfer_soa, d_workspace});
}
int64_t psa_rk4_pairs_chain_workspace_bytes(int n_pairs, int64_t n_points) { return pairs_chain_workspace_bytes(n_pairs, n_points); }

int psa_rk4_comb_f64(int device, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                     const double *kappa, const double *gamma, const double *alpha, const double *a0_re_im, uint32_t flags,
                     double *a_end_re_im, double *p_wave_end, double *p_wave_max, int64_t *first_bad_step, double *traj_or_null,
                     double *elapsed_ms_or_null) {
    return wave_host(device, CombCall<double>{n_lines, n_points, n_steps, z_max, save_every, kappa, gamma, alpha, a0_re_im, flags,
                                              a_end_re_im, p_wave_end, p_wave_max, first_bad_step, traj_or_null}, elapsed_ms_or_null);
}
int psa_rk4_comb_f64_dev(void *stream, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                         const double *d_kappa_soa, const double *d_gamma, const double *d_alpha, const double *d_a0_soa,
                         uint32_t flags, double *d_a_end_soa, double *d_p_wave_end_soa, double *d_p_wave_max_soa,
                         int64_t *d_first_bad_step, double *d_traj_soa_or_null) {
    return wave_dev(stream, CombCall<double>{n_lines, n_points, n_steps, z_max, save_every, d_kappa_soa, d_gamma, d_alpha, d_a0_soa,
                                             flags, d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step,
                                             d_traj_soa_or_null});
}
int psa_rk4_comb_f32(int device, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                     const float *kappa, const float *gamma, const float *alpha, const float *a0_re_im, uint32_t flags,
                     float *a_end_re_im, float *p_wave_end, float *p_wave_max, int64_t *first_bad_step, float *traj_or_null,
                     double *elapsed_ms_or_null) {
    return wave_host(device, CombCall<float>{n_lines, n_points, n_steps, z_max, save_every, kappa, gamma, alpha, a0_re_im, flags,
                                             a_end_re_im, p_wave_end, p_wave_max, first_bad_step, traj_or_null}, elapsed_ms_or_null);
}
int psa_rk4_comb_f32_dev(void *stream, int n_lines, int64_t n_points, int64_t n_steps, double z_max, int32_t save_every,
                         const float *d_kappa_soa, const float *d_gamma, const float *d_alpha, const float *d_a0_soa,
                         uint32_t flags, float *d_a_end_soa, float *d_p_wave_end_soa, float *d_p_wave_max_soa,
                         int64_t *d_first_bad_step, float *d_traj_soa_or_null) {
    return wave_dev(stream, CombCall<float>{n_lines, n_points, n_steps, z_max, save_every, d_kappa_soa, d_gamma, d_alpha, d_a0_soa,
                                            flags, d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step,
                                            d_traj_soa_or_null});
}

int psa_rk4_comb_chain_f64(int device, int n_lines, int64_t n_points, int n_segments, const int64_t *n_steps, const double *seg_len,
                           int32_t save_every, const double *kappa, const double *gamma, const double *alpha,
                           const double *a0_re_im, const double *transfer_re_im, uint32_t flags, double *a_end_re_im,
                           double *p_wave_end, double *p_wave_max, int64_t *first_bad_step, double *traj_or_null,
                           double *elapsed_ms_or_null) {
    return chain_host<CombCall<double>>(device, {{n_lines, n_points, 0, 0.0, save_every, kappa, gamma, alpha, a0_re_im, flags, a_end_re_im,
                                         p_wave_end, p_wave_max, first_bad_step, traj_or_null},
                                        n_segments, n_steps, seg_len, transfer_re_im, nullptr}, elapsed_ms_or_null);
}
int psa_rk4_comb_chain_f64_dev(void *stream, int n_lines, int64_t n_points, int n_segments, const int64_t *n_steps,
                               const double *seg_len, int32_t save_every, const double *d_kappa_soa, const double *d_gamma,
                               const double *d_alpha, const double *d_a0_soa, const double *d_transfer_soa, uint32_t flags,
                               double *d_a_end_soa, double *d_p_wave_end_soa, double *d_p_wave_max_soa,
                               int64_t *d_first_bad_step, double *d_traj_soa_or_null, void *d_workspace) {
    return chain_dev<CombCall<double>>(stream, {{n_lines, n_points, 0, 0.0, save_every, d_kappa_soa, d_gamma, d_alpha, d_a0_soa, flags,
                                        d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad_step, d_traj_soa_or_null},
                                       n_segments, n_steps, seg_len, d_transfer_soa, d_workspace});
}
int64_t psa_rk4_comb_chain_workspace_bytes(int n_lines, int64_t n_points) { return comb_chain_workspace_bytes(n_lines, n_points); }

}  // extern "C"
