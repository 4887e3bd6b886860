// psa_rk4_carried.inc.h -- the step, the replay and the z-loops of the float64 RK4 sweep kernels that CARRY ONE PHASE FACTOR
// PER LANE (gfx950): two lanes per point (psa_rk4_split_kernel.inc.h), four lanes per point (psa_rk4_quad_kernel.inc.h),
// one lane per signal/idler pair (psa_rk4_pairs_kernel.inc.h) and the single-pump model (psa_rk4_single_pump_kernel.inc.h).
// A kernel brings its loads and lane roles, its stage function, its non-finite test over the lanes of a point, its running
// summaries and its stores; the method is here, once.  (sweep_point of psa_rk4_kernel.inc.h -- frame-anchored step, two
// phase factors for six waves, the mirrored half state -- and the packed float32 body keep loops of their own.)
//
// The rules of the loops:
//
//  * Phase.  A lane carries P(z) = amp * exp(i*dbeta*z) with the stage coefficient folded into amp.  P is seeded exactly
//    (one sincos of dbeta * (i*h), z_i formed from the integer step index) on the ABSOLUTE grid i = 0, RESYNC, 2*RESYNC, ...
//    and rotated by exp(i*dbeta*h/2) twice per step in between.  The grid does not depend on save_every, so the computed
//    trajectory does not depend on which rows are saved: A[-1] at any stride is the same row of the every-step run bit for
//    bit, as upstream, where the stride only selects rows (integrators.py:137-140).
//
//  * Events.  The steps between two events (a saved row, a re-seed, the end) run in a branch-free unrolled inner loop:
//    with one wave per SIMD every taken branch is an exposed instruction refetch.  Every branch is
//    wave-uniform: on a kernel argument, the loop counters or a ballot.
//
//  * Tail.  A[-1] is the last SAVED row, not necessarily z_max.  The steps behind it change no output but first_bad_step,
//    so they run only under a check (n_run = n_steps), otherwise the loop ends at the last saved row.
//
//  * Checks.  CHECK_NONE: first_bad_step = -1, NaNs propagate.  CHECK_BLOCK: one test per saved row and one for the tail;
//    the answer is the last step of the first non-finite block.  CHECK_EXACT: the forward pass tests as CHECK_BLOCK does and
//    keeps the state of the last test point (y, P, the step index); when a test finds a point of the wave newly non-finite,
//    the steps since then are REPLAYED on a copy with a test after each one.  The replay repeats the forward pass operation
//    for operation -- the same step function, re-seeds at the same absolute steps, rotations in between -- so it reproduces
//    the forward trajectory bit for bit and the index it finds is the reference's per-step index (integrators.py:132-135).
//    Only waves with a failing point take the branch, and the steady-state loop holds no test.
//
//  * Fallback.  If a replay should stay finite although the forward pass was not -- it cannot, short of a fault, since it
//    repeats the same operations -- `bad` becomes the block-mode answer i_now - 1 rather than staying -1: a point that is
//    non-finite in its outputs never reports "healthy".
//
//  * Lanes of a point.  nonfinite_on may exchange values between the lanes of a point (DPP reads lanes that EXEC has
//    disabled).  It is reached as `bad < 0 && nonfinite_on(y)`: `bad` is written only from results of nonfinite_on, which
//    are the same in every lane of a point, so the lanes of a point skip or run an exchange together.
#pragma once
#include <type_traits>

#include "psa_internal.h"
#include "psa_rk4_prims.inc.h"

namespace psa {

// Stage coefficients folded into the physics constants -- d = h/2 for stages 1, 2 and 4, h for stage 3 -- and the half-step
// rotator of the lane's phase rate.  ha = -alpha/2.
struct CarriedConsts {
    double hd, g_d, tg_d, ha_d, g_h, tg_h, ha_h, rc, rs;
};
__device__ __forceinline__ CarriedConsts carried_consts(const double g, const double ha, const double dbd, const double z_max,
                                                        const int n_steps) {
    CarriedConsts K;
    const double tg = g + g;
    K.hd = z_max / (double)n_steps;   // np.linspace step
    const double hh = 0.5 * K.hd;
    K.g_d = hh * g, K.tg_d = hh * tg, K.ha_d = hh * ha;
    K.g_h = K.hd * g, K.tg_h = K.hd * tg, K.ha_h = K.hd * ha;
    Phase<double>::eval(dbd * (0.5 * K.hd), K.rc, K.rs);
    return K;
}

// exact (re-)seed of the carried factor at z = step * h
__device__ __forceinline__ void carried_seed(const double amp, const double dbd, const double hd, const int step, double &pr,
                                             double &pi) {
    double c, s;
    Phase<double>::eval(dbd * ((double)step * hd), c, s);
    pr = amp * c;
    pi = amp * s;
}

using HalfStage = std::false_type;   // the h/2 coefficients apply
using FullStage = std::true_type;    // the h coefficients apply (stage 3), and the factor handed in is the doubled one

// One classic RK4 step (integrators.py:54-59), regrouped: Y2 = y + d k1, Y3 = y + d k2, Y4 = y + h k3, D = t + d k4 with
// t = Y2 + 2 Y3 + Y4 - 4 y, y += D/3.  stage(which, a, base, pr, pi, out) forms out = base + c * dA/dz(a) with the factor
// (pr, pi); (pr, pi) enters at z_step and leaves rotated to z_step + h.
template <int NC, typename Stage>
__device__ __forceinline__ void carried_step(double (&y)[NC], double &pr, double &pi, const double rc, const double rs,
                                             Stage &stage) {
    double Y2[NC], Y3[NC], Y4[NC], t[NC], D[NC];
    stage(HalfStage{}, y, y, pr, pi, Y2);
    rotate(pr, pi, rc, rs);   // z + h/2
    stage(HalfStage{}, Y2, y, pr, pi, Y3);
    stage(FullStage{}, Y3, y, pr + pr, pi + pi, Y4);
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = fma_(2.0, Y3[c], fma_(-4.0, y[c], Y2[c])) + Y4[c];
    rotate(pr, pi, rc, rs);   // z + h
    stage(HalfStage{}, Y4, t, pr, pi, D);
    const double third = 1.0 / 3.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = fma_(D[c], third, y[c]);
}

// The event-driven z-loop with the block test and the exact index by replay; returns first_bad_step.  DEPTH = steps per trip
// of the inner loop (4: then two, then one; 2: then one).  step_on(y, pr, pi), seed_on(step, pr, pi) and nonfinite_on(y) work
// on the state they are handed (the replay hands them a copy).  At a saved row, in this order: summarise(), the block test,
// the exact test, save_row(row, last) -- `last` marks A[-1].  A sweep without a saved row after z = 0 calls neither.
template <int CHECK, int DEPTH, int NC, typename StepOn, typename SeedOn, typename NonfiniteOn, typename Summarise, typename SaveRow>
__device__ __forceinline__ long long carried_event_loop(double (&y)[NC], double &pr, double &pi, const int n_steps, const int se,
                                                        StepOn &step_on, SeedOn &seed_on, NonfiniteOn &nonfinite_on,
                                                        Summarise &summarise, SaveRow &save_row) {
    static_assert(DEPTH == 2 || DEPTH == 4, "steps per trip");
    constexpr int RESYNC = Phase<double>::RESYNC;
    const int n_rows = n_steps / se;                                  // saved rows after z = 0
    const int n_run = (CHECK != CHECK_NONE) ? n_steps : n_rows * se;   // the tail only matters for the check
    long long bad = -1;

    constexpr bool REPLAY = CHECK == CHECK_EXACT;
    double y_chk[REPLAY ? NC : 1], pr_chk = pr, pi_chk = pi;
    int i_chk = 0;
    auto checkpoint = [&](const int step) {
        if constexpr (REPLAY) {
#pragma unroll
            for (int c = 0; c < NC; ++c) y_chk[c] = y[c];
            pr_chk = pr;
            pi_chk = pi;
            i_chk = step;
        }
    };
    auto exact_test = [&](const int i_now) {   // at a test point: y is the state after step i_now - 1
        if constexpr (REPLAY) {
            const bool newly_bad = bad < 0 && nonfinite_on(y);
            if (__builtin_amdgcn_ballot_w64(newly_bad) != 0) {
                double yy[NC], qr = pr_chk, qi = pi_chk;
#pragma unroll
                for (int c = 0; c < NC; ++c) yy[c] = y_chk[c];
                int ii = i_chk;
                while (ii < i_now) {
                    if (ii % RESYNC == 0) seed_on(ii, qr, qi);   // the forward pass seeds at the same steps
                    const int to_seed = RESYNC - ii % RESYNC;
                    const int e = (i_now - ii > to_seed) ? ii + to_seed : i_now;
#pragma nounroll
                    for (int st = ii; st < e; ++st) {
                        step_on(yy, qr, qi);
                        if (bad < 0 && nonfinite_on(yy)) bad = st;
                    }
                    ii = e;
                }
                if (newly_bad && bad < 0) bad = i_now - 1;   // the replay stayed finite: the block-mode answer
            }
            checkpoint(i_now);
        }
    };

    int i = 0, row = 0;
    int next_save = (n_rows > 0) ? se : 0x7fffffff;
    int next_seed = 0;
    checkpoint(0);
    while (i < n_run) {
        if (i == next_seed) {
            seed_on(i, pr, pi);
            next_seed = (n_run - i > RESYNC) ? i + RESYNC : 0x7fffffff;   // no overflow near 2^31 steps
        }
        int end = n_run < next_seed ? n_run : next_seed;
        end = end < next_save ? end : next_save;
        const int m = end - i;
        int j = 0;
        if constexpr (DEPTH == 4) {
            for (; j + 4 <= m; j += 4) {
                step_on(y, pr, pi);
                step_on(y, pr, pi);
                step_on(y, pr, pi);
                step_on(y, pr, pi);
            }
        }
        for (; j + 2 <= m; j += 2) {
            step_on(y, pr, pi);
            step_on(y, pr, pi);
        }
        if (j < m) step_on(y, pr, pi);
        i = end;
        if (i == next_save) {
            ++row;
            summarise();
            if constexpr (CHECK == CHECK_BLOCK) {
                if (bad < 0 && nonfinite_on(y)) bad = i - 1;
            }
            exact_test(i);
            const bool last = row == n_rows;   // the last saved row, not necessarily z_max
            save_row(row, last);
            next_save = last ? 0x7fffffff : next_save + se;
        }
    }
    if constexpr (CHECK == CHECK_BLOCK) {   // covers the unsaved tail
        if (bad < 0 && n_run > 0 && nonfinite_on(y)) bad = n_run - 1;
    }
    if (n_run > i_chk) exact_test(n_run);   // the unsaved tail (CHECK_EXACT only; compiled out otherwise)
    return bad;
}

// save_every == 1 with a trajectory: EVERY step is a saved row, the HBM-bound regime.  A dedicated loop keeps the per-row work
// to what the row needs -- summarise(), the finite test, store_row(r) -- with no event bookkeeping between steps, two steps
// per trip so that the stores of one row issue under the next step, one seed per RESYNC chunk.  A row is a step here, so the
// test is exact in either check mode and nothing is replayed.  summarise() may leave NaN propagation to its caller, after
// the loop: NaN is sticky in y.  Returns first_bad_step.
template <int CHECK, int NC, typename StepOn, typename SeedOn, typename NonfiniteOn, typename Summarise, typename StoreRow>
__device__ __forceinline__ long long carried_every_step_loop(double (&y)[NC], double &pr, double &pi, const int n_steps,
                                                             StepOn &step_on, SeedOn &seed_on, NonfiniteOn &nonfinite_on,
                                                             Summarise &summarise, StoreRow &store_row) {
    constexpr int RESYNC = Phase<double>::RESYNC;
    long long bad = -1;
    auto save_row = [&](const int r) {
        summarise();
        if constexpr (CHECK != CHECK_NONE) {
            if (bad < 0 && nonfinite_on(y)) bad = r - 1;
        }
        store_row(r);
    };
    int i = 0;
    while (i < n_steps) {
        seed_on(i, pr, pi);
        const int end = (n_steps - i > RESYNC) ? i + RESYNC : n_steps;
        for (; i + 2 <= end; i += 2) {
            step_on(y, pr, pi);
            save_row(i + 1);
            step_on(y, pr, pi);
            save_row(i + 2);
        }
        if (i < end) {
            step_on(y, pr, pi);
            save_row(i + 1);
            ++i;
        }
    }
    return bad;
}

}  // namespace psa
