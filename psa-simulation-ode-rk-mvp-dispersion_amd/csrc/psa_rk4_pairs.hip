// psa_rk4_pairs.hip -- float64 instantiations of the multi-channel RK4 sweep kernel (gfx950): two pumps and 1..16
// signal/idler pairs, one lane per pair (psa_rk4_pairs_kernel.inc.h).
#include "psa_rk4_pairs_kernel.inc.h"

namespace psa {

// SIMDs (4 per CU) of the device the launch goes to: the stream's device, which need not be the thread's current one.
// (psa_rk4_f64.hip keeps a cached copy of this query private to its own launcher.)
static int pairs_simd_count(hipStream_t s) {
    int dev = -1, cus = 0;
    if (s == nullptr || hipStreamGetDevice(s, &dev) != hipSuccess) {
        if (hipGetDevice(&dev) != hipSuccess) return 1024;
    }
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return 4 * cus;
}

// L: the power of two >= n_pairs, at least 2 (a single pair runs beside one dark lane)
int pairs_lanes_per_point(int n_pairs) {
    int l = 2;
    while (l < n_pairs) l <<= 1;
    return l;
}

hipError_t launch_sweep_pairs_f64(hipStream_t s, uint32_t flags, const PairsArgs &a) {
    if (a.n_points == 0) return hipSuccess;
    const int lanes_per_point = pairs_lanes_per_point(a.n_pairs);
    const long long lanes = (long long)lanes_per_point * a.n_points;
    const int check = !(flags & PSA_OPT_CHECK_NAN) ? CHECK_NONE : ((flags & PSA_OPT_EXACT_STEP) ? CHECK_EXACT : CHECK_BLOCK);
    // the rule of launch_sweep_f64: 64-thread workgroups while the launch's waves fit half the SIMDs, 256 beyond.  Rows exist
    // with 256-thread workgroups only: the block size changes the speed and no number, and a launch that saves rows is bound
    // by its stores (PSA_OPT_BLOCK64 selects nothing there).
    const long long waves = (lanes + 63) / 64;
    const bool traj = a.traj != nullptr;
    const int block = (!traj && ((flags & PSA_OPT_BLOCK64) || 2 * waves <= (long long)pairs_simd_count(s))) ? 64 : 256;
    const bool lossless = (flags & PSA_OPT_LOSSLESS) != 0;
    const dim3 grid((unsigned)((lanes + block - 1) / block)), blk(block);
    return with_int<2, 4, 8, 16>(lanes_per_point, [&](auto l) {
    return with_int<CHECK_NONE, CHECK_BLOCK, CHECK_EXACT>(check, [&](auto chk) {
    return with_bool(lossless, [&](auto ll) {
        void *args[] = {const_cast<PairsArgs *>(&a)};
        const void *k = block == 64 ? reinterpret_cast<const void *>(&rk4_sweep_pairs_kernel<l, chk, 64, !ll, false>)
                        : traj      ? reinterpret_cast<const void *>(&rk4_sweep_pairs_kernel<l, chk, 256, !ll, true>)
                                    : reinterpret_cast<const void *>(&rk4_sweep_pairs_kernel<l, chk, 256, !ll, false>);
        (void)hipLaunchKernel(k, grid, blk, args, 0, s);
        return hipGetLastError();
    }); }); });
}

}  // namespace psa
