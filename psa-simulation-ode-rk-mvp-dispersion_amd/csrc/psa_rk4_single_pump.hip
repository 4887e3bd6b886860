// psa_rk4_single_pump.hip -- float64 instantiations of the single-pump three-wave RK4 sweep kernel (gfx950): one pump, a
// signal and an idler, one sweep point per lane (psa_rk4_single_pump_kernel.inc.h).
#include "psa_rk4_single_pump_kernel.inc.h"

namespace psa {

hipError_t launch_sweep_single_pump_f64(hipStream_t s, uint32_t flags, const SinglePumpArgs<double> &a) {
    const int block = workgroup_size(flags, a.n_points, simd_count(s));
    return with_int<CHECK_NONE, CHECK_BLOCK, CHECK_EXACT>(check_mode(flags), [&](auto chk) {
    return with_bool(a.traj != nullptr, [&](auto traj) {
    return with_int<64, 256>(block, [&](auto b) {
    return with_bool((flags & PSA_OPT_LOSSLESS) != 0, [&](auto ll) {
        return launch_lanes(reinterpret_cast<const void *>(&rk4_sweep_single_pump_kernel<chk, traj, b, !ll>), a.n_points, block, 0, a, s);
    }); }); }); });
}

}  // namespace psa
