// psa_rk4_single_pump_f32.hip -- float32 instantiations of the single-pump three-wave RK4 sweep kernel (gfx950): two sweep
// points per lane, packed math (psa_rk4_single_pump_pk_kernel.inc.h).
#include "psa_rk4_single_pump_pk_kernel.inc.h"

namespace psa {

hipError_t launch_sweep_single_pump_f32(hipStream_t s, uint32_t flags, const SinglePumpArgs<float> &a) {
    // Its own: two points per lane.  PSA_OPT_LOSSLESS is a promise about alpha and selects nothing: one register layout.
    const long long lanes = packed_lanes(a.n_points);
    const int block = workgroup_size(flags, lanes, simd_count(s));
    return with_int<CHECK_NONE, CHECK_BLOCK, CHECK_EXACT>(check_mode(flags), [&](auto chk) {
    return with_bool(a.traj != nullptr, [&](auto traj) {
    return with_int<64, 256>(block, [&](auto b) {
        return launch_lanes(reinterpret_cast<const void *>(&rk4_sweep_single_pump_pk_kernel<chk, traj, b>), lanes, block, 0, a, s);
    }); }); });
}

}  // namespace psa
