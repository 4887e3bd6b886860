// psa_rk4_single_pump_f32.hip -- float32 instantiations of the single-pump three-wave RK4 sweep kernel (gfx950): two sweep
// points per lane, packed math (psa_rk4_single_pump_pk_kernel.inc.h).
#include "psa_rk4_single_pump_pk_kernel.inc.h"

namespace psa {

hipError_t launch_sweep_single_pump_f32(hipStream_t s, uint32_t flags, const SinglePumpArgs<float> &a) {
    if (a.n_points == 0) return hipSuccess;
    const int check = !(flags & PSA_OPT_CHECK_NAN) ? CHECK_NONE : ((flags & PSA_OPT_EXACT_STEP) ? CHECK_EXACT : CHECK_BLOCK);
    // the rule of the float64 launcher, counted over lanes (two points each): 64-thread workgroups while the launch's waves fit
    // half the SIMDs, 256 beyond.  PSA_OPT_LOSSLESS is a promise about alpha and selects nothing: one register layout.
    const long long lanes = PackedPoints::lanes(a.n_points);
    const long long waves = (lanes + 63) / 64;
    const int block = ((flags & PSA_OPT_BLOCK64) || 2 * waves <= (long long)single_pump_simd_count(s)) ? 64 : 256;
    const dim3 grid((unsigned)((lanes + block - 1) / block)), blk(block);
    return with_int<CHECK_NONE, CHECK_BLOCK, CHECK_EXACT>(check, [&](auto chk) {
    return with_bool(a.traj != nullptr, [&](auto traj) {
    return with_int<64, 256>(block, [&](auto b) {
        void *args[] = {const_cast<SinglePumpArgs<float> *>(&a)};
        (void)hipLaunchKernel(reinterpret_cast<const void *>(&rk4_sweep_single_pump_pk_kernel<chk, traj, b>), grid, blk, args, 0, s);
        return hipGetLastError();
    }); }); });
}

}  // namespace psa
