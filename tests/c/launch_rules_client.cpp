// launch_rules_client.cpp -- the launch rules of csrc/psa_launch_rules.h on the CPU: plain C++, no HIP, no library.  Every
// expectation is a number worked out by hand from the launchers as they stood before the rules had a header of their own
// (64-thread workgroups while 2 * ceil(lanes / 64) <= SIMDs, 256 beyond; grid = ceil(lanes / workgroup); ...), not a value
// this header returned.  Built and run by tests/test_launch_rules.py.
#include <cstdio>

#include "psa_launch_rules.h"
#include "psa_rk4.h"

static int failures = 0;

#define EXPECT_EQ(expr, want)                                                                                   \
    do {                                                                                                        \
        const long long got_ = (long long)(expr), want_ = (long long)(want);                                    \
        if (got_ != want_) {                                                                                    \
            std::printf("line %d: %s = %lld, expected %lld\n", __LINE__, #expr, got_, want_);                   \
            ++failures;                                                                                         \
        }                                                                                                       \
    } while (0)

int main() {
    using namespace psa;
    const uint32_t NAN_ = PSA_OPT_CHECK_NAN, EXACT = PSA_OPT_EXACT_STEP, B64 = PSA_OPT_BLOCK64;

    // check mode: EXACT_STEP means something only with CHECK_NAN; no other flag takes part
    EXPECT_EQ(CHECK_NONE, 0);
    EXPECT_EQ(CHECK_BLOCK, 1);
    EXPECT_EQ(CHECK_EXACT, 2);
    EXPECT_EQ(check_mode(0), CHECK_NONE);
    EXPECT_EQ(check_mode(EXACT), CHECK_NONE);
    EXPECT_EQ(check_mode(NAN_), CHECK_BLOCK);
    EXPECT_EQ(check_mode(NAN_ | EXACT), CHECK_EXACT);
    EXPECT_EQ(check_mode(B64 | PSA_OPT_LOSSLESS | PSA_OPT_LDS_STAGING), CHECK_NONE);
    EXPECT_EQ(check_mode(NAN_ | B64 | PSA_OPT_LOSSLESS), CHECK_BLOCK);

    // workgroup size and grid.  MI355X: 256 CUs, 1 024 SIMDs -- 512 waves of 64 lanes are half of them
    EXPECT_EQ(workgroup_size(0, 32768, 1024), 64);
    EXPECT_EQ(grid_blocks(32768, 64), 512);
    EXPECT_EQ(workgroup_size(0, 32769, 1024), 256);
    EXPECT_EQ(grid_blocks(32769, 256), 129);
    EXPECT_EQ(workgroup_size(B64, 32769, 1024), 64);
    EXPECT_EQ(grid_blocks(32769, 64), 513);
    EXPECT_EQ(workgroup_size(0, 1, 1024), 64);
    EXPECT_EQ(grid_blocks(1, 64), 1);
    EXPECT_EQ(workgroup_size(0, 256, 8), 64);     // 4 waves, 8 SIMDs
    EXPECT_EQ(workgroup_size(0, 257, 8), 256);    // 5 waves
    EXPECT_EQ(workgroup_size(B64, 1 << 20, 1024), 64);
    EXPECT_EQ(workgroup_size(NAN_ | EXACT | PSA_OPT_LOSSLESS, 32769, 1024), 256);   // no other flag forces 64
    EXPECT_EQ(grid_blocks(256, 256), 1);
    EXPECT_EQ(grid_blocks(257, 256), 2);
    EXPECT_EQ(grid_blocks(3LL << 30, 64), 50331648);   // lanes above 2^31

    // two float32 points per lane: lanes = (n + 1) / 2, and the rule counts lanes
    EXPECT_EQ(packed_lanes(0), 0);
    EXPECT_EQ(packed_lanes(1), 1);
    EXPECT_EQ(packed_lanes(2), 1);
    EXPECT_EQ(packed_lanes(65536), 32768);
    EXPECT_EQ(workgroup_size(0, packed_lanes(65536), 1024), 64);
    EXPECT_EQ(packed_lanes(65537), 32769);
    EXPECT_EQ(workgroup_size(0, packed_lanes(65537), 1024), 256);

    // multi-channel model: L lanes per point for K pairs
    const int K[] = {1, 2, 3, 4, 5, 8, 9, 16}, L[] = {2, 2, 4, 4, 8, 8, 16, 16};
    for (int i = 0; i < 8; ++i) EXPECT_EQ(pairs_lanes_per_point(K[i]), L[i]);
    // ... the shared rule without rows, 256 with rows whatever BLOCK64 says
    EXPECT_EQ(pairs_workgroup_size(0, 32768, 1024, false), 64);
    EXPECT_EQ(pairs_workgroup_size(0, 32769, 1024, false), 256);
    EXPECT_EQ(pairs_workgroup_size(B64, 32769, 1024, false), 64);
    EXPECT_EQ(pairs_workgroup_size(0, 2, 1024, true), 256);
    EXPECT_EQ(pairs_workgroup_size(B64, 2, 1024, true), 256);
    EXPECT_EQ(pairs_workgroup_size(B64, 32769, 1024, true), 256);

    // float64 comb: 16 M bytes per lane of dynamic LDS from M = 10
    EXPECT_EQ(comb_rotators_in_lds(9), 0);
    EXPECT_EQ(comb_rotators_in_lds(10), 1);
    EXPECT_EQ(comb_lds_bytes(3, 64), 0);
    EXPECT_EQ(comb_lds_bytes(9, 256), 0);
    EXPECT_EQ(comb_lds_bytes(10, 64), 10240);
    EXPECT_EQ(comb_lds_bytes(12, 256), 49152);
    EXPECT_EQ(lds_limit_raised(comb_lds_bytes(PSA_MAX_LINES, 256)), 0);

    // float32 comb: 0, 1 or 3 vectors of 16 M bytes per lane; the limit is raised exactly above 64 KiB
    const int vec_m[] = {3, 7, 8, 9, 10, 11, 12}, vec[] = {0, 0, 1, 1, 3, 3, 3};
    for (int i = 0; i < 7; ++i) EXPECT_EQ(comb_pk_lds_vectors(vec_m[i]), vec[i]);
    EXPECT_EQ(comb_pk_lds_bytes(7, 256), 0);
    EXPECT_EQ(comb_pk_lds_bytes(8, 256), 32768);
    EXPECT_EQ(lds_limit_raised(comb_pk_lds_bytes(8, 256)), 0);
    EXPECT_EQ(comb_pk_lds_bytes(10, 64), 30720);
    EXPECT_EQ(lds_limit_raised(comb_pk_lds_bytes(10, 64)), 0);
    EXPECT_EQ(comb_pk_lds_bytes(10, 256), 122880);
    EXPECT_EQ(lds_limit_raised(comb_pk_lds_bytes(10, 256)), 1);
    EXPECT_EQ(comb_pk_lds_bytes(12, 256), 147456);
    EXPECT_EQ(lds_limit_raised(comb_pk_lds_bytes(12, 256)), 1);
    EXPECT_EQ(lds_limit_raised(0), 0);
    EXPECT_EQ(lds_limit_raised(65536), 0);
    EXPECT_EQ(lds_limit_raised(65537), 1);

    if (failures) {
        std::printf("launch_rules_client: %d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("launch_rules_client ok\n");
    return 0;
}
