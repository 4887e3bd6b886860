// psa_rk4_f64.hip -- float64 instantiations of the RK4 sweep kernels (gfx950): one point per lane, and one point per
// lane PAIR (psa_rk4_split_kernel.inc.h) for sweeps smaller than the chip.
#include <atomic>

#include "psa_rk4_quad_kernel.inc.h"

namespace psa {

// SIMDs (4 per CU) of the device the launch goes to -- the stream's device, which need not be the thread's current one
// (the _dev entry points take the caller's stream); cached per device ordinal.  Every sweep launcher sizes its workgroups by it.
int simd_count(hipStream_t s) {
    static std::atomic<int> cache[64];
    int dev = -1;
    if (s == nullptr || hipStreamGetDevice(s, &dev) != hipSuccess) {
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    }
    if (dev < 0 || dev >= 64) return 1024;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        v = 4 * cus;
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

// ---- which lane layout?  A cost model from measured instruction counts (profiles/kernels.json, SQ_INSTS_VALU per wave
// per z-step): one lane per point issues I1 = 300.7 (4 waves) / 471.9 (6 waves) instructions per step, two lanes per point
// I2 = 183.6 / 296.8 per lane, four lanes per point (4 waves only, psa_rk4_quad_kernel.inc.h) I4 ~ 157.  The z-loop is issue-bound and sequential, so a launch takes as long as its busiest SIMD:
//     T(layout) ~ I(layout) * k / eff(k),      k = ceil(waves(layout) / SIMDs)  waves sharing a SIMD,
// eff(k) = sustained DP issue rate with k resident waves (tools/dp_peak.hip: 0.896, 0.94, 0.96 of nominal for 1, 2, >= 3).
// Two lanes per point win whenever the doubled wave count still rounds to the same k (N <= 32 768 on MI355X: k = 1 either
// way, 0.61-0.65 of the time) and again in windows like 65 536 < N <= 98 304 (three half-length waves per SIMD beat two
// full-length ones); in between (32 768 < N <= 65 536) every SIMD that holds 64 points needs I1 whatever the layout, so one
// lane per point is the floor there -- a hybrid launch cannot beat its slowest wave (profiles/r03_split_cliff.log).
// I1 is the general loop's count.  For mirrored inputs (A2 == A1, A4 == A3: psa_rk4_kernel.inc.h) the one-lane kernel issues
// about half of it, which this choice -- made on the host, where a0 cannot be seen -- does not know: in the second window
// above the two-lane layout it picks is then the slower one, although a mirrored wave of the two-lane
// kernel runs that same mirrored loop on its even lanes.
// -> lanes per point: 1, 2 or (4 waves only) 4
static int best_lanes_per_point(int n_waves, long long n_points, int simds) {
    const double i1 = (n_waves == 4) ? 300.7 : 471.9, i2 = (n_waves == 4) ? 183.6 : 296.8, i4 = 157.0;
    auto eff = [](long long k) { return k <= 1 ? 0.896 : (k == 2 ? 0.94 : 0.96); };
    auto cost = [&](double instr, long long lanes) {
        const long long k = ((lanes + 63) / 64 + simds - 1) / simds;
        return instr * (double)k / eff(k);
    };
    const double t1 = cost(i1, n_points), t2 = cost(i2, 2 * n_points);
    int best = t2 < t1 ? 2 : 1;
    if (n_waves == 4 && cost(i4, 4 * n_points) < (best == 2 ? t2 : t1)) best = 4;
    return best;
}

// Layout precedence: PSA_OPT_QUAD_POINT (4 waves only; one lane otherwise), PSA_OPT_SPLIT_POINT, PSA_OPT_ONE_LANE, then
// the cost model above.  Multi-lane layouts exist for the register layout only, and a multi-lane trajectory launch folds
// the lane's wave offset into the 32-bit store offset (NW * ld * 16 B < 2^32): otherwise one lane per point, forced or not.
hipError_t launch_sweep_f64(hipStream_t s, int n_waves, uint32_t flags, const SweepArgs<double> &a) {
    Pick p = pick_one_lane(n_waves, flags, a);
    const int simds = simd_count(s);
    const bool multi_ok = !p.lds && (!p.traj || (unsigned long long)a.traj_ld * n_waves * 16ull < (1ull << 32));
    int lanes = 1;
    if (multi_ok && !(flags & PSA_OPT_ONE_LANE)) {
        if (flags & PSA_OPT_QUAD_POINT) lanes = n_waves == 4 ? 4 : 1;
        else if (flags & PSA_OPT_SPLIT_POINT) lanes = 2;
        else lanes = best_lanes_per_point(n_waves, a.n_points, simds);
    }
    if (lanes == 1) {
        // the row-driven z-loop (4 waves, register layout, no trajectory) compiled for the row length, where a row exists
        if (n_waves == 4 && !p.traj && !p.lds && a.save_every == PSA_FIXED_ROW && a.n_steps >= PSA_FIXED_ROW) p.row = PSA_FIXED_ROW;
        return launch_family<OneLane<double>>(s, p, a);
    }
    p.block = workgroup_size(flags, (long long)lanes * a.n_points, simds);
    p.lossless = (flags & PSA_OPT_LOSSLESS) != 0;
    return lanes == 2 ? launch_family<SplitLanes>(s, p, a) : launch_family<QuadLanes>(s, p, a);
}
}  // namespace psa
