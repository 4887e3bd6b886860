// psa_rk4_pairs.hip -- float64 instantiations of the multi-channel RK4 sweep kernel (gfx950): two pumps and 1..16
// signal/idler pairs, one lane per pair (psa_rk4_pairs_kernel.inc.h).
#include "psa_rk4_pairs_kernel.inc.h"

namespace psa {

// Its own: L lanes per point, and rows exist with 256-thread workgroups only (pairs_workgroup_size)
hipError_t launch_sweep_pairs_f64(hipStream_t s, uint32_t flags, const PairsArgs &a) {
    const int lanes_per_point = pairs_lanes_per_point(a.n_pairs);
    const long long lanes = (long long)lanes_per_point * a.n_points;
    const bool traj = a.traj != nullptr;
    const int block = pairs_workgroup_size(flags, lanes, simd_count(s), traj);
    return with_int<2, 4, 8, 16>(lanes_per_point, [&](auto l) {
    return with_int<CHECK_NONE, CHECK_BLOCK, CHECK_EXACT>(check_mode(flags), [&](auto chk) {
    return with_bool((flags & PSA_OPT_LOSSLESS) != 0, [&](auto ll) {
        const void *k = block == 64 ? reinterpret_cast<const void *>(&rk4_sweep_pairs_kernel<l, chk, 64, !ll, false>)
                        : traj      ? reinterpret_cast<const void *>(&rk4_sweep_pairs_kernel<l, chk, 256, !ll, true>)
                                    : reinterpret_cast<const void *>(&rk4_sweep_pairs_kernel<l, chk, 256, !ll, false>);
        return launch_lanes(k, lanes, block, 0, a, s);
    }); }); });
}

}  // namespace psa
