// psa_rk4_comb.hip -- float64 instantiations of the multi-line ("frequency comb") RK4 sweep kernel (gfx950): M = 3 ..
// PSA_MAX_LINES equally spaced lines with every FWM product among them, one sweep point per lane
// (psa_rk4_comb_kernel.inc.h).
#include "psa_rk4_comb_kernel.inc.h"

namespace psa {

static_assert(PSA_MAX_LINES == 12, "the instantiation list below ends at PSA_MAX_LINES");

hipError_t launch_sweep_comb_f64(hipStream_t s, uint32_t flags, const CombArgs<double> &a) {
    if (a.n_points == 0) return hipSuccess;
    // the rule of launch_sweep_single_pump_f64: 64-thread workgroups while the launch's waves fit half the SIMDs, 256 beyond
    const long long waves = (a.n_points + 63) / 64;
    const int block = ((flags & PSA_OPT_BLOCK64) || 2 * waves <= (long long)single_pump_simd_count(s)) ? 64 : 256;
    const dim3 grid((unsigned)((a.n_points + block - 1) / block)), blk(block);
    return with_int<3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(a.n_lines, [&](auto m) {
    return with_bool((flags & PSA_OPT_CHECK_NAN) != 0, [&](auto chk) {
    return with_bool((flags & PSA_OPT_LOSSLESS) != 0, [&](auto ll) {
        void *args[] = {const_cast<CombArgs<double> *>(&a)};
        const size_t lds = comb_rotators_in_lds(m) ? (size_t)16 * m * block : 0;   // at most 48 KiB: 12 lines, 256 threads
        (void)hipLaunchKernel(reinterpret_cast<const void *>(&rk4_sweep_comb_kernel<m, chk, !ll>), grid, blk, args, lds, s);
        return hipGetLastError();
    }); }); });
}

}  // namespace psa
