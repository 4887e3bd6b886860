/* The chain entry points of include/psa_rk4.h (4/6 waves in both precisions, single pump; host and `_dev` forms) and the two
 * workspace sizes, called with invalid argument sets and with n_points = 0: every call ends in validation, so no device is
 * needed.  Built with the host sanitizers by tools/chain_host_sanitize.sh, where a clean exit is the result; the codes are
 * those of tests/golden/cabi_errors.json.  Exit code 0 = all as documented. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "psa_rk4.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #cond, __LINE__, psa_last_error()); return 1; } } while (0)

static double buf[64];
static float buf32[64];
static int64_t bad[8];

/* one call of every form on the same grid; the f32 forms share the f64 forms' rules */
static int chain(int dev, int f32, int nw, int64_t n, int S, const int64_t *steps, const double *lens, int32_t se,
                 const void *dbeta2, uint32_t flags, void *traj, void *wend, void *wmax, void *ws) {
    void *b = f32 ? (void *)buf32 : (void *)buf, *in = n ? b : NULL;
    int64_t *fb = n ? bad : NULL;
    if (f32)
        return dev ? psa_rk4_chain_f32_dev(NULL, nw, n, S, steps, lens, se, in, dbeta2, in, in, in, NULL, flags, in, in, in, fb, traj, wend, wmax, ws)
                   : psa_rk4_chain_f32(0, nw, n, S, steps, lens, se, in, dbeta2, in, in, in, NULL, flags, in, in, in, fb, traj, NULL, wend, wmax);
    return dev ? psa_rk4_chain_f64_dev(NULL, nw, n, S, steps, lens, se, in, dbeta2, in, in, in, NULL, flags, in, in, in, fb, traj, wend, wmax, ws)
               : psa_rk4_chain_f64(0, nw, n, S, steps, lens, se, in, dbeta2, in, in, in, NULL, flags, in, in, in, fb, traj, NULL, wend, wmax);
}

static int single_pump(int dev, int64_t n, int S, const int64_t *steps, const double *lens, int32_t se, const double *dbeta,
                       uint32_t flags, double *wmax, double *traj, void *ws) {
    double *in = n ? buf : NULL;
    int64_t *fb = n ? bad : NULL;
    return dev ? psa_rk4_single_pump_chain_f64_dev(NULL, n, S, steps, lens, se, dbeta, in, in, in, NULL, flags, in, in, wmax, fb, traj, ws)
               : psa_rk4_single_pump_chain_f64(0, n, S, steps, lens, se, dbeta, in, in, in, NULL, flags, in, in, wmax, fb, traj, NULL);
}

int main(void) {
    const int64_t steps[2] = {10, 20}, zero_first[2] = {0, 20}, zero_second[2] = {10, 0}, odd[2] = {10, 21}, huge[2] = {10, 2684354560LL};
    const double lens[2] = {1.0, 2.0}, nan_second[2] = {1.0, NAN}, zero_first_len[2] = {0.0, 2.0};
    int dev, f32;
    for (dev = 0; dev < 2; ++dev) {
        for (f32 = 0; f32 < 2; ++f32) {
            void *b = f32 ? (void *)buf32 : (void *)buf;
            EXPECT(chain(dev, f32, 4, 8, 0, steps, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NSTEPS);
            EXPECT(chain(dev, f32, 4, 8, 2, NULL, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NULLPTR);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, NULL, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NULLPTR);
            EXPECT(chain(dev, f32, 5, 8, 2, steps, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NWAVES);
            EXPECT(chain(dev, f32, 4, -1, 2, steps, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NPOINTS);
            EXPECT(chain(dev, f32, 4, 8, 2, zero_first, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NSTEPS);
            EXPECT(chain(dev, f32, 4, 8, 2, zero_second, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NSTEPS);
            EXPECT(chain(dev, f32, 4, 8, 2, huge, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_NSTEPS);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, zero_first_len, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_ZMAX);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, nan_second, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_ZMAX);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, lens, 0, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_SAVE_EVERY);
            EXPECT(chain(dev, f32, 4, 8, 2, odd, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_SAVE_EVERY);
            EXPECT(chain(dev, f32, 6, 8, 2, steps, lens, 5, NULL, 0u, NULL, NULL, NULL, b) == PSA_E_DBETA2);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, lens, 5, b, 0u, NULL, NULL, NULL, b) == PSA_E_DBETA2);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, lens, 5, NULL, PSA_OPT_SPLIT_POINT | PSA_OPT_ONE_LANE, NULL, NULL, NULL, b) == PSA_E_FLAGS);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, lens, 5, NULL, 0u, NULL, b, NULL, b) == PSA_E_NULLPTR);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, lens, 5, NULL, 0u, NULL, NULL, b, b) == PSA_E_NULLPTR);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, lens, 5, NULL, 0u, b, b, b, b) == PSA_E_FLAGS);
            EXPECT(chain(dev, f32, 4, 8, 2, steps, lens, 5, NULL, PSA_OPT_BLOCK64, NULL, b, b, b) == PSA_E_FLAGS);
            EXPECT(chain(dev, f32, 4, f32 ? 268435456LL : 134217728LL, 2, steps, lens, 5, NULL, 0u, b, NULL, NULL, b) == PSA_E_TOO_LARGE);
            EXPECT(chain(dev, f32, 4, 0, 2, steps, lens, 5, NULL, 0u, NULL, NULL, NULL, NULL) == PSA_OK);
            EXPECT(chain(dev, f32, 6, 0, 1, steps, lens, 5, NULL, PSA_OPT_CHECK_NAN, NULL, NULL, NULL, NULL) == PSA_OK);
        }
        EXPECT(chain(1, dev, 4, 8, 2, steps, lens, 5, NULL, 0u, NULL, NULL, NULL, NULL) == PSA_E_NULLPTR);   /* no d_workspace */
        EXPECT(strstr(psa_last_error(), "d_workspace") != NULL);

        EXPECT(single_pump(dev, 8, 0, steps, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_NSTEPS);
        EXPECT(single_pump(dev, 8, -1, steps, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_NSTEPS);
        EXPECT(single_pump(dev, 8, 2, NULL, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_NULLPTR);
        EXPECT(single_pump(dev, 8, 2, steps, NULL, 5, buf, 0u, buf, NULL, buf) == PSA_E_NULLPTR);
        EXPECT(single_pump(dev, -1, 2, steps, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_NPOINTS);
        EXPECT(single_pump(dev, PSA_MAX_POINTS + 1LL, 2, steps, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_TOO_LARGE);
        EXPECT(single_pump(dev, 8, 2, zero_first, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_NSTEPS);
        EXPECT(single_pump(dev, 8, 2, zero_second, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_NSTEPS);
        EXPECT(single_pump(dev, 8, 2, huge, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_NSTEPS);
        EXPECT(single_pump(dev, 8, 2, steps, zero_first_len, 5, buf, 0u, buf, NULL, buf) == PSA_E_ZMAX);
        EXPECT(single_pump(dev, 8, 2, steps, nan_second, 5, buf, 0u, buf, NULL, buf) == PSA_E_ZMAX);
        EXPECT(single_pump(dev, 8, 2, steps, lens, 0, buf, 0u, buf, NULL, buf) == PSA_E_SAVE_EVERY);
        EXPECT(single_pump(dev, 8, 2, odd, lens, 5, buf, 0u, buf, NULL, buf) == PSA_E_SAVE_EVERY);
        EXPECT(single_pump(dev, 8, 2, steps, lens, 5, dev ? NULL : buf, 0u, dev ? buf : NULL, NULL, buf) == PSA_E_NULLPTR);
        EXPECT(single_pump(dev, 8, 2, steps, lens, 5, buf, PSA_OPT_ONE_LANE | PSA_OPT_CHECK_NAN, buf, NULL, buf) == PSA_E_FLAGS);
        EXPECT(single_pump(dev, 8, 2, steps, lens, 5, buf, 1u << 30, NULL, NULL, buf) == PSA_E_FLAGS);
        EXPECT(single_pump(dev, 268435456LL, 2, steps, lens, 5, buf, 0u, buf, buf, buf) == PSA_E_TOO_LARGE);
        EXPECT(single_pump(dev, 8, 2, steps, lens, 5, buf, PSA_BCAST_TRANSFER | PSA_OPT_LOSSLESS | PSA_OPT_BLOCK64, NULL, NULL, buf) == PSA_E_NULLPTR);
        EXPECT(single_pump(dev, 0, 2, steps, lens, 5, NULL, 0u, NULL, NULL, NULL) == PSA_OK);
        EXPECT(single_pump(dev, 0, 1, steps, lens, 5, NULL, PSA_OPT_CHECK_NAN, NULL, NULL, NULL) == PSA_OK);
    }
    EXPECT(single_pump(0, 8, 2, steps, lens, 5, buf, PSA_OPT_TRAJ_LD, buf, NULL, NULL) == PSA_E_FLAGS);   /* the _dev form's bit */
    EXPECT(single_pump(1, 8, 2, steps, lens, 5, buf, 0u, buf, NULL, NULL) == PSA_E_NULLPTR);             /* no d_workspace */
    EXPECT(strstr(psa_last_error(), "d_workspace") != NULL);

    EXPECT(psa_rk4_chain_workspace_bytes(4, 0, 8, 0) == 0 && psa_rk4_chain_workspace_bytes(6, 0, 4, 1) == 0);
    EXPECT(psa_rk4_chain_workspace_bytes(4, 300, 8, 0) == 2560 + 2 * 19200 + 2 * 2560 + 2560);
    EXPECT(psa_rk4_chain_workspace_bytes(6, 300, 4, 1) == 2 * 2560 + 2 * 14592 + 2 * 1280 + 2560 + 2 * 7424);
    EXPECT(psa_rk4_chain_workspace_bytes(5, 300, 8, 0) == -1 && psa_rk4_chain_workspace_bytes(4, -1, 8, 0) == -1);
    EXPECT(psa_rk4_chain_workspace_bytes(4, 300, 2, 0) == -1 && psa_rk4_chain_workspace_bytes(4, 300, -8, 1) == -1);
    EXPECT(psa_rk4_single_pump_chain_workspace_bytes(0) == 0);
    EXPECT(psa_rk4_single_pump_chain_workspace_bytes(300) == 2 * 2560 + 2 * 14592 + 2 * 7424);
    EXPECT(psa_rk4_single_pump_chain_workspace_bytes(-1) == -1 && psa_rk4_single_pump_chain_workspace_bytes(-(1LL << 40)) == -1);
    printf("chain_args_client ok: %s\n", psa_version());
    return 0;
}
