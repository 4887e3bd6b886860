// psa_rk4_comb_f32.hip -- float32 instantiations of the multi-line ("frequency comb") RK4 sweep kernel (gfx950): M = 3 ..
// PSA_MAX_LINES equally spaced lines with every FWM product among them, two sweep points per lane, packed math
// (psa_rk4_comb_pk_kernel.inc.h).
#include "psa_rk4_comb_pk_kernel.inc.h"

namespace psa {

static_assert(PSA_MAX_LINES == 12, "the instantiation list below ends at PSA_MAX_LINES");

hipError_t launch_sweep_comb_f32(hipStream_t s, uint32_t flags, const CombArgs<float> &a) {
    // Its own: two points per lane, the check is a bool, the lane's LDS column from M = 8 (launch_lanes raises the limit where
    // it must).  PSA_OPT_LOSSLESS is a promise about alpha and selects nothing: one register layout.
    const long long lanes = packed_lanes(a.n_points);
    const int block = workgroup_size(flags, lanes, simd_count(s));
    return with_int<3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(a.n_lines, [&](auto m) {
    return with_bool((flags & PSA_OPT_CHECK_NAN) != 0, [&](auto chk) {
        return launch_lanes(reinterpret_cast<const void *>(&rk4_sweep_comb_pk_kernel<m, chk>), lanes, block,
                            comb_pk_lds_bytes(m, block), a, s);
    }); });
}

}  // namespace psa
