// psa_rk4_f32.hip -- float32 instantiations of the RK4 sweep (gfx950): one point per lane, and two points per lane
// with packed math (PSA_OPT_F32_PACKED forces it, PSA_OPT_F32_SCALAR forbids it).  Measured on MI355X the packed form is
// never slower (1.14x at 65 536 points, 1.85x at 131 072, 1.94x at 2^20: non-packed and packed float32 VALU ops both
// occupy a SIMD for 4 cycles per wave64 -- tools/sp_peak.hip, profiles/r02_sp_peak.log -- so packing is the only way to
// the float32 vector peak), hence the default is packed for every sweep of at least two points without LDS staging.
#include "psa_rk4_pk_kernel.inc.h"

namespace psa {
hipError_t launch_sweep_f32(hipStream_t s, int n_waves, uint32_t flags, const SweepArgs<float> &a) {
    Pick p = pick_one_lane(n_waves, flags, a);
    // the packed kernel has no lossless form, and with the promise given one lane is preferred only when it was forced
    if (!(flags & PSA_OPT_F32_SCALAR)) p.lossless = false;
    if (!p.lds && ((flags & PSA_OPT_F32_PACKED) || (!(flags & PSA_OPT_F32_SCALAR) && a.n_points >= 2)))
        return launch_family<PackedPoints>(s, p, a);
    return launch_family<OneLane<float>>(s, p, a);
}
}  // namespace psa
