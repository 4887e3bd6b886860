// psa_rk4_pk_body.inc.h -- the per-lane body of rk4_sweep_pk_kernel: everything behind the a0 loads.  NOT a header: the kernel
// includes this text twice, once per z-loop, inside a scope that provides
//     MIRROR (constexpr bool), A, idx, N, pt[2], live1, wave_full, load2(base, stride)  and the state  V y[MIRROR ? NW : 2 * NW].
// MIRROR = true (4 waves) is the same body on HALF the state, as in sweep_point: y, yb, dl, k, ys and acc hold
// [Re A1, Im A1, Re A3, Im A3] of points whose a0 has A2 == A1 and A4 == A3 bit for bit, the stage is yaman_stage_mirrored
// (un-fused), and waves 2 and 4 of the record are written from the registers of waves 1 and 3.  The step, seeds,
// fold(), event loop, track, tail, every-step loop and summary are this one text for both.
// 168 packed instructions per step and point pair instead of 328 (4 * 32 stage + 6 rotation + 6 * 4 update + 2 * 4 state
// = 166 by hand; the general step 4 * 64 + 6 + 6 * 8 + 2 * 8 = 326; as built, tools/isa_loop_stats.py).
//
// Why text and not a function template like sweep_point: a function, even a forced-inline one, is optimised on its own
// before it is inlined, the kernel-argument loads of the general instantiations then all move to the kernel's entry and
// every one of them needs 2 to 13 VGPRs more (the 6-wave per-wave-summary ones leave the 256 that two waves per SIMD allow).
// Included into the kernel, the general loop is compiled exactly as before there was a second one.
    static_assert(!MIRROR || NW == 4, "the mirrored body exists for the 4-wave step");
    constexpr int NS = MIRROR ? NW : NC;        // components of the state this lane carries
    constexpr int NWS = NS / 2;                 // waves of that state
    constexpr int SIG = MIRROR ? 2 : 4;         // Re A_sig in the state
    auto at = [](const int c) { return MIRROR ? (((c >> 2) << 1) | (c & 1)) : c; };   // record component -> state component

    const V g = load2(A.gamma, A.gamma_stride);
    const V tg = g + g;
    const V ha = splat2(-0.5f) * load2(A.alpha, A.alpha_stride);
    double dbd[NP][2];
    {
        const V d0 = load2(A.dbeta, 1);
        dbd[0][0] = (double)d0.x;
        dbd[0][1] = (double)d0.y;
        if constexpr (NP == 2) {
            const V d1 = load2(A.dbeta2, 1);
            dbd[1][0] = (double)d1.x;
            dbd[1][1] = (double)d1.y;
        }
    }
    const double hd = A.z_max / (double)A.n_steps;
    const V h = splat2((float)hd), hh = splat2((float)(0.5 * hd)), h6 = splat2((float)(hd / 6.0));
    const V two = splat2(2.0f);

    V rc[NP], rs[NP], Er[NP], Ei[NP];
    auto seed = [&](const double z, V (&outc)[NP], V (&outs)[NP], const V amp) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float c0, s0, c1, s1;
            Phase<float>::eval(dbd[p][0] * z, c0, s0);
            Phase<float>::eval(dbd[p][1] * z, c1, s1);
            outc[p] = amp * (V){c0, c1};
            outs[p] = amp * (V){s0, s1};
        }
    };
    seed(0.5 * hd, rc, rs, splat2(1.0f));   // half-step rotator exp(i*dbeta*h/2)
#pragma unroll
    for (int p = 0; p < NP; ++p) { Er[p] = tg; Ei[p] = V{}; }
    auto seed_phase = [&](const int step) { seed((double)step * hd, Er, Ei, tg); };   // exact re-seed of the phase recurrence at z = step * h

    // Compensated state.  float32 loses the part of each increment (~1e-5 |y| at 1e6 steps) below ulp(y): plain y += inc
    // drifts ~n * ulp (5e-3 at BASELINE config 4's 1e6 steps).  The state is therefore kept as  yb + dl : a base yb and a
    // SMALL running offset dl that collects the increments (rounded at ulp(dl) ~ 1e-4 ulp(y)); y = fl(yb + dl) is formed once
    // per step for the stage inputs, and every FOLD steps dl is folded into yb with its rounding residue kept (Fast2Sum).
    // 16 + 8 + 24/FOLD instructions per step and component pair against 40 for a Kahan update of y every step.
    constexpr int FOLD = RESYNC;      // folded where the phase is re-seeded
    V yb[NS], dl[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        yb[c] = y[c];
        dl[c] = V{};
    }
    auto fold = [&]() { pk_fold(y, [&](const int c) -> V & { return yb[c]; }, [&](const int c) -> V & { return dl[c]; }); };
    V pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
    V pm = pe;
    long long bad[2] = {-1, -1};
    V pwm[WSUM ? NWS : 1];   // WSUM: np.max of |A_j|^2 over saved rows, every wave of the state
    if constexpr (WSUM) {
#pragma unroll
        for (int j = 0; j < NWS; ++j) pwm[j] = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
    }
    auto track = [&](const int step) { pk_track(y, step, bad); };
    auto store_rows = [&](float *base) {  // base[c * N + point]
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float *dst = base + (long long)c * N + pt[0];
            if (wave_full) {
                *reinterpret_cast<f32x2_u *>(dst) = y[at(c)];
            } else {
                dst[0] = y[at(c)].x;
                if (live1) dst[1] = y[at(c)].y;
            }
        }
    };
    auto store2 = [&](float *base, const V v) {   // base[pt0], base[pt1]
        if (wave_full) {
            *reinterpret_cast<f32x2_u *>(base + pt[0]) = v;
        } else {
            base[pt[0]] = v.x;
            if (live1) base[pt[1]] = v.y;
        }
    };

    const int se = A.save_every;
    const int n_rows = A.n_steps / se;
    const int n_run = (CHECK != CHECK_NONE) ? A.n_steps : n_rows * se;
    // trajectory rows [row][wave][N][2]: the lane's two points are adjacent, so each wave of the model is ONE 16-B streaming
    // store per lane (1 KiB per wave instruction); the (row, wave) part of the address stays in SGPRs and the lane adds a
    // 32-bit byte offset (the C-ABI keeps N * 8 B < 2^31 for trajectory launches), exactly as rk4_sweep_kernel does.
    const long long LD = A.traj_ld;   // points per (row, wave) region (psa_traj_ld)
    const unsigned lane_off = (unsigned)idx * 16u;
    auto store_traj_row = [&](const int r) {
        const char *rowb = reinterpret_cast<const char *>(A.traj) + (long long)r * NW * LD * 8;
        if (wave_full) {
#pragma unroll
            for (int j = 0; j < NW; ++j)
                store_quad_nt(rowb + (long long)j * LD * 8, lane_off, (f32x4){y[at(2 * j)].x, y[at(2 * j + 1)].x, y[at(2 * j)].y, y[at(2 * j + 1)].y});
        } else {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const char *wb = rowb + (long long)j * LD * 8;
                store_pair_nt(wb, lane_off, (f32x2){y[at(2 * j)].x, y[at(2 * j + 1)].x});
                if (live1) store_pair_nt(wb, lane_off + 8u, (f32x2){y[at(2 * j)].y, y[at(2 * j + 1)].y});
            }
        }
    };
    if constexpr (TRAJ) store_traj_row(0);
    auto store_wave_end = [&]() {   // WSUM: |A_j|^2 of the row a_end holds
        if constexpr (WSUM) {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const V xr = y[at(2 * j)], xi = y[at(2 * j + 1)];
                store2(A.p_wave_end + (long long)j * N, fma_(xr, xr, xi * xi));
            }
        }
    };
    if (n_rows == 0) {
        store_rows(A.a_end);
        store_wave_end();
    }

    auto rhs = [&](const V (&a)[NS], V (&k)[NS]) {   // dA/dz(a) at the carried phase factor
        if constexpr (MIRROR) yaman_stage_mirrored<V, true, false>(a, a, Er[0], Ei[0], g, tg + tg, ha, k);
        else yaman_rhs<V, NW>(a, Er, Ei, g, tg, ha, k);
    };
    auto rk4_step = [&](const int step_index) {  // integrators.py:54-59, low storage: y, y_stage, accumulator
        V k[NS], ys[NS], acc[NS];
        rhs(y, k);
#pragma unroll
        for (int c = 0; c < NS; ++c) { acc[c] = k[c]; ys[c] = fma_(hh, k[c], y[c]); }
#pragma unroll
        for (int p = 0; p < NP; ++p) rotate(Er[p], Ei[p], rc[p], rs[p]);
        rhs(ys, k);
#pragma unroll
        for (int c = 0; c < NS; ++c) { acc[c] = fma_(two, k[c], acc[c]); ys[c] = fma_(hh, k[c], y[c]); }
        rhs(ys, k);
#pragma unroll
        for (int c = 0; c < NS; ++c) { acc[c] = fma_(two, k[c], acc[c]); ys[c] = fma_(h, k[c], y[c]); }
#pragma unroll
        for (int p = 0; p < NP; ++p) rotate(Er[p], Ei[p], rc[p], rs[p]);
        rhs(ys, k);
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            dl[c] = fma_(h6, acc[c] + k[c], dl[c]);   // the increment joins the small offset ...
            y[c] = yb[c] + dl[c];                     // ... and y is the rounded state again (next stage input, saved rows)
        }
        if constexpr (CHECK == CHECK_EXACT) track(step_index);
    };

    auto write_summary = [&]() {
        store2(A.p_end, pe);
        store2(A.p_max, pm);
        A.first_bad[pt[0]] = bad[0];
        if (live1) A.first_bad[pt[1]] = bad[1];
        if constexpr (WSUM) {
#pragma unroll
            for (int j = 0; j < NW; ++j) store2(A.p_wave_max + (long long)j * N, pwm[at(2 * j) / 2]);
        }
    };

    // ---- save_every == 1 with a trajectory: every step is a saved row (integrators.py:137) -- the HBM-bound regime.  A
    // dedicated loop, as in rk4_sweep_kernel: per row only |A_sig|^2, the running maximum, the block-mode finite test and
    // the NW streaming stores; two steps per trip so one row's stores issue under the next step.
    if constexpr (TRAJ) {
        if (se == 1) {
            auto save_row = [&](const int r) {
                pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
                pm = (V){__builtin_fmaxf(pe.x, pm.x), __builtin_fmaxf(pe.y, pm.y)};   // NaN is made to propagate below
                if constexpr (CHECK == CHECK_BLOCK) track(r - 1);
                store_traj_row(r);
            };
            int i = 0;
            while (i < n_run) {
                seed_phase(i);
                fold();                               // RESYNC == FOLD steps since the last one
                const int end = (n_run - i > RESYNC) ? i + RESYNC : n_run;
                for (; i + 2 <= end; i += 2) {
                    rk4_step(i);
                    save_row(i + 1);
                    rk4_step(i + 1);
                    save_row(i + 2);
                }
                if (i < end) {
                    rk4_step(i);
                    save_row(i + 1);
                    ++i;
                }
            }
            if (pe.x != pe.x) pm.x = pe.x;   // np.max over the saved rows propagates NaN (sticky in y)
            if (pe.y != pe.y) pm.y = pe.y;
            store_rows(A.a_end);
            write_summary();
            return;
        }
    }

    // seeds (and the folds of the compensated state, FOLD == RESYNC) on the absolute grid i = 0, RESYNC, ...: the trajectory
    // does not depend on save_every (see rk4_sweep_kernel)
    static_assert(FOLD == RESYNC, "the state is folded where the phase is re-seeded");
    int i = 0, row = 0;
    int next_save = (n_rows > 0) ? se : 0x7fffffff;
    int next_seed = 0;
    while (i < n_run) {
        if (i == next_seed) {
            seed_phase(i);
            fold();
            next_seed = (n_run - i > RESYNC) ? i + RESYNC : 0x7fffffff;
        }
        int end = n_run < next_seed ? n_run : next_seed;
        end = end < next_save ? end : next_save;
        const int m = end - i;
        int j = 0;
        for (; j + 2 <= m; j += 2) {
            rk4_step(i + j);
            rk4_step(i + j + 1);
        }
        if (j < m) rk4_step(i + j);
        i = end;
        if (i == next_save) {
            ++row;
            pe = fma_(y[SIG], y[SIG], y[SIG + 1] * y[SIG + 1]);
            pm.x = (pe.x > pm.x || pe.x != pe.x) ? pe.x : pm.x;  // np.max propagates NaN
            pm.y = (pe.y > pm.y || pe.y != pe.y) ? pe.y : pm.y;
            if constexpr (WSUM) {
#pragma unroll
                for (int j = 0; j < NWS; ++j) {
                    const V pj = fma_(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]);
                    pwm[j].x = (pj.x > pwm[j].x || pj.x != pj.x) ? pj.x : pwm[j].x;
                    pwm[j].y = (pj.y > pwm[j].y || pj.y != pj.y) ? pj.y : pwm[j].y;
                }
            }
            if constexpr (CHECK == CHECK_BLOCK) track(i - 1);
            if constexpr (TRAJ) store_traj_row(row);
            if (row == n_rows) {
                store_rows(A.a_end);
                store_wave_end();
                next_save = 0x7fffffff;
            } else {
                next_save += se;
            }
        }
    }
    if constexpr (CHECK == CHECK_BLOCK) {
        if (n_run > 0) track(n_run - 1);
    }
    write_summary();
