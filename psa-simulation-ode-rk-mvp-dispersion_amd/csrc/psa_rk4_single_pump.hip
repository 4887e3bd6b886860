// psa_rk4_single_pump.hip -- float64 instantiations of the single-pump three-wave RK4 sweep kernel (gfx950): one pump, a
// signal and an idler, one sweep point per lane (psa_rk4_single_pump_kernel.inc.h).
#include "psa_rk4_single_pump_kernel.inc.h"

namespace psa {

// SIMDs (4 per CU) of the device the launch goes to: the stream's device, which need not be the thread's current one.
int single_pump_simd_count(hipStream_t s) {
    int dev = -1, cus = 0;
    if (s == nullptr || hipStreamGetDevice(s, &dev) != hipSuccess) {
        if (hipGetDevice(&dev) != hipSuccess) return 1024;
    }
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return 4 * cus;
}

hipError_t launch_sweep_single_pump_f64(hipStream_t s, uint32_t flags, const SinglePumpArgs<double> &a) {
    if (a.n_points == 0) return hipSuccess;
    const int check = !(flags & PSA_OPT_CHECK_NAN) ? CHECK_NONE : ((flags & PSA_OPT_EXACT_STEP) ? CHECK_EXACT : CHECK_BLOCK);
    // the rule of launch_sweep_f64: 64-thread workgroups while the launch's waves fit half the SIMDs, 256 beyond
    const long long waves = (a.n_points + 63) / 64;
    const int block = ((flags & PSA_OPT_BLOCK64) || 2 * waves <= (long long)single_pump_simd_count(s)) ? 64 : 256;
    const bool lossless = (flags & PSA_OPT_LOSSLESS) != 0;
    const dim3 grid((unsigned)((a.n_points + block - 1) / block)), blk(block);
    return with_int<CHECK_NONE, CHECK_BLOCK, CHECK_EXACT>(check, [&](auto chk) {
    return with_bool(a.traj != nullptr, [&](auto traj) {
    return with_int<64, 256>(block, [&](auto b) {
    return with_bool(lossless, [&](auto ll) {
        void *args[] = {const_cast<SinglePumpArgs<double> *>(&a)};
        (void)hipLaunchKernel(reinterpret_cast<const void *>(&rk4_sweep_single_pump_kernel<chk, traj, b, !ll>), grid, blk, args, 0, s);
        return hipGetLastError();
    }); }); }); });
}

}  // namespace psa
