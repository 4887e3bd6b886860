// psa_launch_rules.h -- the launch rules of every sweep kernel family as plain C++: no HIP, nothing of the device.  What a
// launcher decides from the flags and the size of a launch is decided here, once (psa_launch.inc.h turns it into the launch);
// tests/c/launch_rules_client.cpp pins every rule on the CPU.  The kernels read the two comb predicates as well.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "psa_rk4.h"

namespace psa {

enum CheckMode : int { CHECK_NONE = 0, CHECK_BLOCK = 1, CHECK_EXACT = 2 };
// PSA_OPT_EXACT_STEP asks for the exact index of a check that PSA_OPT_CHECK_NAN turns on: alone it selects nothing
inline CheckMode check_mode(uint32_t flags) {
    return !(flags & PSA_OPT_CHECK_NAN) ? CHECK_NONE : ((flags & PSA_OPT_EXACT_STEP) ? CHECK_EXACT : CHECK_BLOCK);
}

// Workgroup size of a launch of `lanes` lanes on a device of `simds` SIMDs (4 per CU).  64-thread workgroups while the
// launch's waves fit half the SIMDs (a sweep of few waves is spread over as many CUs as it has waves), 256 beyond (four waves
// per workgroup land on the four SIMDs of one CU: the placement that gives every wave its own SIMD when the sweep fills the
// chip -- 1 024 single-wave workgroups measured 12 % slower at N = 32 768 because some SIMDs received two).  PSA_OPT_BLOCK64
// forces 64.  The block size changes the speed and no number.
inline int workgroup_size(uint32_t flags, long long lanes, int simds) {
    const long long waves = (lanes + 63) / 64;
    return ((flags & PSA_OPT_BLOCK64) || 2 * waves <= (long long)simds) ? 64 : 256;
}
inline unsigned grid_blocks(long long lanes, int block) { return (unsigned)((lanes + block - 1) / block); }

// Two float32 points per lane (every packed kernel): the odd tail has a lane to itself
inline long long packed_lanes(long long n_points) { return (n_points + 1) / 2; }

// Multi-channel model, L lanes per point: the power of two >= n_pairs, at least 2 (a single pair runs beside one dark lane).
// Its rows exist with 256-thread workgroups only: a launch that saves rows is bound by its stores (BLOCK64 selects nothing).
inline int pairs_lanes_per_point(int n_pairs) {
    int l = 2;
    while (l < n_pairs) l <<= 1;
    return l;
}
inline int pairs_workgroup_size(uint32_t flags, long long lanes, int simds, bool traj) {
    return traj ? 256 : workgroup_size(flags, lanes, simds);
}

// Float64 comb: where the registers (256 VGPRs + 256 AGPRs at one wave per SIMD) do not hold the whole state without scratch
// memory, the rotators live in LDS: 16 M bytes per lane of dynamic LDS (at most 48 KiB: 12 lines, 256 threads).
constexpr bool comb_rotators_in_lds(const int m) { return m >= 10; }
inline size_t comb_lds_bytes(int m, int block) { return comb_rotators_in_lds(m) ? (size_t)16 * m * block : 0; }
// Float32 comb: 2M-vectors of f32x2 the lane keeps in LDS instead of registers: 0 none, 1 the rotators, 2 and dl, 3 and yb.
// 16 M bytes per vector and lane; the lane's LDS column is at most 144 KiB of the CU's 160 (12 lines, 256 threads, 3 vectors).
constexpr int comb_pk_lds_vectors(const int m) { return m >= 10 ? 3 : (m >= 8 ? 1 : 0); }
inline size_t comb_pk_lds_bytes(int m, int block) { return (size_t)16 * m * comb_pk_lds_vectors(m) * block; }
// Above the 64 KiB a launch gets by default the kernel's dynamic LDS limit is raised first
inline bool lds_limit_raised(size_t lds_bytes) { return lds_bytes > 65536; }

}  // namespace psa
