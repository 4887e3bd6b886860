// psa_rk4_comb_f32.hip -- float32 instantiations of the multi-line ("frequency comb") RK4 sweep kernel (gfx950): M = 3 ..
// PSA_MAX_LINES equally spaced lines with every FWM product among them, two sweep points per lane, packed math
// (psa_rk4_comb_pk_kernel.inc.h).
#include "psa_rk4_comb_pk_kernel.inc.h"

namespace psa {

static_assert(PSA_MAX_LINES == 12, "the instantiation list below ends at PSA_MAX_LINES");

hipError_t launch_sweep_comb_f32(hipStream_t s, uint32_t flags, const CombArgs<float> &a) {
    if (a.n_points == 0) return hipSuccess;
    // the rule of launch_sweep_comb_f64, counted over lanes (two points each): 64-thread workgroups while the launch's waves
    // fit half the SIMDs, 256 beyond.  PSA_OPT_LOSSLESS is a promise about alpha and selects nothing: one register layout.
    const long long lanes = PackedPoints::lanes(a.n_points);
    const long long waves = (lanes + 63) / 64;
    const int block = ((flags & PSA_OPT_BLOCK64) || 2 * waves <= (long long)single_pump_simd_count(s)) ? 64 : 256;
    const dim3 grid((unsigned)((lanes + block - 1) / block)), blk(block);
    return with_int<3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(a.n_lines, [&](auto m) {
    return with_bool((flags & PSA_OPT_CHECK_NAN) != 0, [&](auto chk) {
        const void *kernel = reinterpret_cast<const void *>(&rk4_sweep_comb_pk_kernel<m, chk>);
        // the lane's LDS column: at most 144 KiB of the CU's 160 (12 lines, 256 threads, three vectors); above the 64 KiB a
        // launch gets by default the kernel's limit is raised first.  The attribute belongs to the function ON THE CURRENT
        // DEVICE, and a sweep split over devices launches from one thread per device: it is set at every such launch (a host
        // call without a device round trip) rather than remembered per kernel and device
        const size_t lds = (size_t)16 * m * comb_pk_lds_vectors(m) * block;
        if (lds > 65536) {
            const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        void *args[] = {const_cast<CombArgs<float> *>(&a)};
        (void)hipLaunchKernel(kernel, grid, blk, args, lds, s);
        return hipGetLastError();
    }); });
}

}  // namespace psa
