// psa_rk4_comb.hip -- float64 instantiations of the multi-line ("frequency comb") RK4 sweep kernel (gfx950): M = 3 ..
// PSA_MAX_LINES equally spaced lines with every FWM product among them, one sweep point per lane
// (psa_rk4_comb_kernel.inc.h).
#include "psa_rk4_comb_kernel.inc.h"

namespace psa {

static_assert(PSA_MAX_LINES == 12, "the instantiation list below ends at PSA_MAX_LINES");

hipError_t launch_sweep_comb_f64(hipStream_t s, uint32_t flags, const CombArgs<double> &a) {
    // Its own: the check is a bool (the test runs after every step), and M >= 10 keeps its rotators in dynamic LDS
    const int block = workgroup_size(flags, a.n_points, simd_count(s));
    return with_int<3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(a.n_lines, [&](auto m) {
    return with_bool((flags & PSA_OPT_CHECK_NAN) != 0, [&](auto chk) {
    return with_bool((flags & PSA_OPT_LOSSLESS) != 0, [&](auto ll) {
        return launch_lanes(reinterpret_cast<const void *>(&rk4_sweep_comb_kernel<m, chk, !ll>), a.n_points, block,
                            comb_lds_bytes(m, block), a, s);
    }); }); });
}

}  // namespace psa
