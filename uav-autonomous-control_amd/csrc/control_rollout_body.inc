// The body of control_rollout_kernel and scored_control_rollout_kernel (control_rollout.hip), included inside both: the unscored
// kernel compiles from it exactly as it did before the scored twin existed (a shared __device__ function, even always inlined,
// changed the unscored kernels' instruction schedule).  In scope where it is included: the kernel's template parameters and
// arguments, `constexpr bool SCORE` and `double *score`.  Not a header of its own.

    // WATCH: obstacles but no log at all -- the second wave exists all the same and only WATCHES: it takes the three
    // position values of every tick through the slab and tests them against obstacle bounds held in its registers.  In the
    // compute wave the same test cost 0.4 us per tick for four obstacles (a scalar-cache round trip per obstacle on the
    // one dependent instruction stream; bounds in lanes + v_readlane were slower still, and it has no registers to hold them).
    constexpr bool WATCH = AABB && !LOG_STATE && !LOG_CMD && CW == SW;
    constexpr bool LOGGING = LOG_STATE || LOG_CMD || WATCH;            // "a second wave takes a slab per tick"
    // PMODE (plan-fed kernels): who evaluates a target row and how a segment's coefficients reach the LDS tile.
    //   0  the compute wave; coefficients through registers on the spot (what a full chip without a second wave uses)
    //   1  the compute wave; coefficients by LDS-DMA an outer tick ahead (see coeffs_dma)
    //   2  the SECOND wave (TGW): it idles four fifths of every tick at the barrier, so it owns the trajectory cursor, evaluates
    //      the next target row (Horner, atan2, yaw scan: ~1 200 cycles per outer tick, 6-10 % of the compute wave's tick) while
    //      the compute wave flies the inner ticks, and hands the row over through a [10][64] LDS tile.
    constexpr bool ADMA = PMODE == 1;
    constexpr bool TGW = PMODE == 2;
    static_assert(!TGW || (POLY && LOGGING), "target rows by the second wave: plan-fed kernels that have one");
    constexpr int NU = 64 * CW;                                        // UAVs per workgroup
    constexpr int NR = (LOG_STATE ? 13 : 0) + (LOG_CMD ? UAVAC_CMD_COLS : 0) + (WATCH ? 3 : 0);
    constexpr int CMD0 = LOG_STATE ? 13 : 0;                           // first command row in a slab
    extern __shared__ double slab[];                                   // [2][NR][NU]
    const size_t sB = (size_t)B;
    // The logs are [K][13 | 12][log_pitch]: rows of log_pitch >= B doubles.  With log_pitch a multiple of 16 every row starts
    // on a 128-byte line whatever B is (B = 65 534 with pitch B ran at half the rate of 65 536: every 512-byte wave store
    // straddled two partially written lines).
    const size_t sP = log_pitch;
    // PERSISTENT TILES.  A tile = NU consecutive UAVs flown for the launch's K ticks.  The launch has at most one workgroup
    // per SIMD (the launcher caps the grid when a log is written); a batch with more tiles than that is walked by the same
    // workgroups, pass after pass, each workgroup moving on to its next tile as soon as its own K ticks are done -- no launch
    // boundary between the passes at which every SIMD would wait for the slowest one (round 2 issued one launch per 65 536
    // columns: 262 144 UAVs ran at 45 G steps/s against 52 G at 65 536).  Results do not depend on the split (tested).
    // XCD-aware tile order inside a pass (uavac_internal.h): every XCD owns one contiguous span of the pass's columns.
    const int grid = (int)gridDim.x;
    int kk = 0;                                    // ticks of earlier tiles: the slab ping-pong keeps alternating across tiles

    // PLACEHOLDER WAVES.  A CU deals the waves of a workgroup round its SIMDs in the order s, s+2, s+1, s+3 and starts the
    // NEXT workgroup one position later in that sequence (tools/census_detail.py).  Four [compute, store] workgroups on a CU
    // therefore end up one compute + one store wave per SIMD -- but TWO of them (B <= 32 768) put the second compute wave on
    // the SIMD of the first store wave and leave one SIMD idle.  With a wave between the two that ends at once --
    // [compute, placeholder, store] -- two workgroups occupy all four SIMDs with one wave each.  A wave that has ended no
    // longer takes part in the workgroup's barriers.
    if (LOGGING && n_idle > 0 && threadIdx.x >= NU && threadIdx.x < NU + 64 * n_idle) return;

    if (LOGGING && threadIdx.x >= NU) {
        // ------------------------------------------------------------------------------ store wave(s)
        static_assert(CW == 1 && SW == 1, "one compute + one store wave per 64-UAV tile");
        constexpr int QPL = 1;
        // (Measured and not kept, all bit-identical, tools/rollout_shapes.py, profiles/r03_rollout_shapes_*.jsonl: two or three
        // store waves per tile sharing a tick's 13 log rows -- 0.93 -> 0.92 ms per 1 000 ticks at B = 32 768, slower from
        // 40 960 up; two compute + two store waves per 128-UAV workgroup, which a CU deals one per SIMD -- slower at every
        // size, 0.87 against 0.77 ms even at B = 16 384: the per-tick barrier then couples two compute waves.)
        const int lane = threadIdx.x & 63;
        __builtin_amdgcn_s_setprio(3);            // few instructions, all on the critical store stream: issue first
        const unsigned lane_bytes = (unsigned)lane * 8u;
        // With a state log the per-tick obstacle test runs HERE, on the positions this wave is about to store, after
        // its stores have been issued: the compute wave's tick stays as short as without obstacles (the two stages
        // couple through one barrier per tick; lengthening the compute stage to the length of the store stage cost
        // 40 % at config 5), and the comparisons fill time in which this wave would wait for the store path anyway.
        constexpr bool AABB_HERE = AABB && (LOG_STATE || WATCH) && QPL == 1;
        // The first kBoxRegs obstacles live in vector registers for the whole launch (this wave has ~200 to spare: the
        // kernel's allocation is sized by the compute wave).  Fetched through uniform addresses they would be scalar
        // loads -- one s_load + s_waitcnt round trip per obstacle per TICK on the critical store stream.
        constexpr int kBoxRegs = 8;
        double box[kBoxRegs][6];
        if (AABB_HERE) {
            int zero = 0;
            asm volatile("" : "+v"(zero));            // a per-lane offset the compiler cannot see through: vector loads
#pragma unroll
            for (int o = 0; o < kBoxRegs; ++o)
#pragma unroll
                for (int j = 0; j < 6; ++j) box[o][j] = o < n_obs ? aabbs[6 * o + j + zero] : 0.0;
            // the loads have landed before the tick loop starts: a load the compiler still sees in flight at the loop
            // head costs an s_waitcnt vmcnt(0) at the first use in EVERY iteration, i.e. a wait for this wave's own stores
#pragma unroll
            for (int o = 0; o < kBoxRegs; ++o)
#pragma unroll
                for (int j = 0; j < 6; ++j) settle(box[o][j]);
        }
      for (int tile0 = 0; tile0 < n_tiles; tile0 += grid, kk += K) {
        const int n_here = min(grid, n_tiles - tile0);
        if ((int)blockIdx.x >= n_here) break;
        const int col0 = (tile0 + xcd_contiguous(blockIdx.x, n_here)) * NU;
        const bool full = col0 + NU <= B;          // every column of this workgroup exists: no per-store mask
        const bool mine = col0 + lane < B;
        int coll = (AABB_HERE && mine) ? istate[2 * sB + col0 + lane] : 0;
        if (AABB_HERE) settle(coll);               // landed before the tick loop (see above)
        // ---- TGW: this wave owns the trajectory cursor of its 64 UAVs (the same arithmetic, in the same order, as the compute
        // wave's in the other modes: E = evaluate the row under the cursor, A = advance; E0 A0 E1 A1 ... -- here E runs one
        // outer tick AHEAD and its update of the yaw scan stays pending until the compute wave has consumed the row, so that
        // what a launch saves is exactly what the other modes save)
        double *tgt = slab + (size_t)2 * NR * NU + (size_t)CW * poly_tile_doubles(YAWSCAN) + lane;        // tgt[j * 64], j = 0 .. 9
        double *tile2 = slab + (size_t)2 * NR * NU;                                                       // the coefficient tile, [12][64][2]
        double *cf2 = tile2 + 2 * lane, *yw2 = tile2 + 24 * 64 + lane;
        const unsigned tile2_lds = TGW ? (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)tile2) : 0u;
        const int bb2 = mine ? col0 + lane : B - 1;
        int t_idx = 0, t_phase = 0, t_nrows = 0, t_pm = 1, t_seg = 0, t_rin = 0, t_srows = 0, t_srows_nx = 0, t_ybase = 0;
        int t_yhas = 0, t_yhas_n = 0, t_asked = 0;
        double t_yprev = 0.0, t_ysum = 0.0, t_yprev_n = 0.0, t_ysum_n = 0.0, t_first_yaw = 0.0;
        const int32_t *t_seg_rows = nullptr;
        const double *t_coeffs = nullptr, *t_yaws = nullptr;
        auto t_load_coeffs = [&](int s_) {           // through registers, on the spot: launch start, the scan's rebuild, empty segments
            const double *src = t_coeffs + 24 * s_;
#pragma unroll
            for (int j = 0; j < 24; ++j) cf2[minsnap_coeff_index<0>(j)] = src[j];
        };
        // E: the row under the cursor -> the target tile, in four pieces (one axis each, then the yaw) spread over four ticks: in
        // one piece it is ~1 300 cycles of a 2 000-cycle tick, and a second wave that is late at the barrier stalls the compute
        // wave (1.30 against 1.26 ms per 1 000 ticks at 65 536 UAVs before the split); the scan's update stays pending
        double t_px = 0, t_py = 0, t_pz = 0, t_vx = 0, t_vy = 0, t_vz = 0, t_ax = 0, t_ay = 0, t_az = 0;
        auto t_eval_axis = [&](int a_) {
            const double t_ = (double)t_rin * P.dt;
            if (a_ == 0) minsnap_eval_axis<0>(cf2, 0, t_, t_px, t_vx, t_ax);
            else if (a_ == 1) minsnap_eval_axis<0>(cf2, 1, t_, t_py, t_vy, t_ay);
            else minsnap_eval_axis<0>(cf2, 2, t_, t_pz, t_vz, t_az);
        };
        auto t_eval_yaw_and_hand_over = [&]() {
            double yaw_;
            t_yhas_n = t_yhas; t_yprev_n = t_yprev; t_ysum_n = t_ysum;
            if (YAWSCAN) {
                const bool yvalid = uavac_yaw::has_heading(t_vx, t_vy);
                const double yang = yvalid ? atan2(t_vy, t_vx) : 0.0;
                const double ycum = (yvalid && t_yhas) ? t_ysum + uavac_yaw::unwrap_correction(yang - t_yprev) : t_ysum;
                yaw_ = yvalid ? yang + ycum : (t_yhas ? t_yprev + t_ysum : t_first_yaw);
                if (t_idx + 1 < t_nrows) {
                    if (yvalid) { t_yhas_n = 1; t_yprev_n = yang; }
                    t_ysum_n = ycum;
                }
            } else {
                yaw_ = yw2[(t_idx - t_ybase) * 64];
            }
            tgt[0] = t_px; tgt[64] = t_py; tgt[128] = t_pz; tgt[192] = t_vx; tgt[256] = t_vy; tgt[320] = t_vz;
            tgt[384] = t_ax; tgt[448] = t_ay; tgt[512] = t_az; tgt[576] = yaw_;
            if (SCORE) tgt[640] = (double)t_idx;          // the row the scores measure this period against
        };
        auto t_eval = [&]() { t_eval_axis(0); t_eval_axis(1); t_eval_axis(2); t_eval_yaw_and_hand_over(); };      // launch start: all at once
        if (TGW) {
            const int64_t off2 = row_offsets[bb2];
            t_nrows = (int)(row_offsets[bb2 + 1] - off2);
            t_idx = istate[0 * sB + bb2];
            t_phase = istate[1 * sB + bb2] % V.F;
            t_pm = P.m;
            size_t seg0 = (size_t)bb2 * P.m;
            if (P.seg_offsets) {
                seg0 = (size_t)P.seg_offsets[bb2];
                const int64_t n_ = P.seg_offsets[bb2 + 1] - P.seg_offsets[bb2];
                t_pm = (int)(n_ < 1 ? 1 : (n_ > P.m ? P.m : n_));
            }
            t_seg_rows = P.seg_rows + seg0;
            t_coeffs = P.coeffs + seg0 * 24;
            t_yaws = YAWSCAN ? nullptr : P.yaw + off2;
            if (t_nrows > 0) {
                t_idx = min(max(t_idx, 0), t_nrows - 1);
                if (YAWSCAN) {
                    t_first_yaw = P.first_yaw[bb2];
                    const double scan_row = state[26 * sB + bb2];
                    if (scan_row == (double)t_idx) {
                        t_yhas = state[27 * sB + bb2] != 0.0;
                        t_yprev = state[28 * sB + bb2];
                        t_ysum = state[29 * sB + bb2];
                    } else {
                        // the cursor is not where the carried scan stands: rebuild it from the mission's first row (rare)
                        int s_ = 0, r_ = 0, n_ = t_seg_rows[0];
                        t_load_coeffs(0);
                        for (int row = 0; row < t_idx; ++row) {
                            while (r_ >= n_ && s_ + 1 < t_pm) { r_ -= n_; ++s_; n_ = t_seg_rows[s_]; t_load_coeffs(s_); }
                            double x_, y_, z_, vx_, vy_, vz_, ax_, ay_, az_;
                            minsnap_eval_row<0>(cf2, (double)r_ * P.dt, x_, y_, z_, vx_, vy_, vz_, ax_, ay_, az_);
                            if (uavac_yaw::has_heading(vx_, vy_)) {
                                const double a_ = atan2(vy_, vx_);
                                if (t_yhas) t_ysum = t_ysum + uavac_yaw::unwrap_correction(a_ - t_yprev);
                                t_yhas = 1;
                                t_yprev = a_;
                            }
                            ++r_;
                        }
                    }
                }
                t_rin = t_idx;
                t_srows = t_seg_rows[0];
                while (t_seg + 1 < t_pm && t_rin >= t_srows) { t_rin -= t_srows; ++t_seg; t_srows = t_seg_rows[t_seg]; }
                t_load_coeffs(t_seg);
                t_srows_nx = t_seg_rows[min(t_seg + 1, t_pm - 1)];
                if (!YAWSCAN) {
                    t_ybase = t_idx;
#pragma unroll
                    for (int j = 0; j < 16; ++j) yw2[j * 64] = t_yaws[min(t_ybase + j, t_nrows - 1)];
                }
                t_eval();
            }
            settle(t_srows_nx); settle(t_idx); settle(t_phase); settle(t_yprev); settle(t_ysum); settle(t_first_yaw);
            lds_barrier();                         // the first target row is in its tile (the compute wave waits here too)
        }
        for (int k = 0; k < K; ++k) {
            lds_barrier();                                             // slab k&1 is complete (stores of earlier ticks stay in flight)
            const double *src = slab + (size_t)((kk + k) & 1) * NR * NU + lane;
            // one log (13 or 12 rows) at a time: every LDS read first, then every store, so that neither the
            // LDS latency nor the store path's acceptance time is paid per element
            if (LOG_STATE) {
                double v[13];
#pragma unroll
                for (int r = 0; r < 13; ++r) v[r] = src[r * NU];
                double *dst = state_log + (size_t)k * 13 * sP + col0;               // wave-uniform: lives in SGPRs
#pragma unroll
                for (int r = 0; r < 13; ++r) {
                    if (full || mine) store_uniform_base(dst + r * sP, lane_bytes, v[r]);      // 512-B coalesced wave store
                    // one obstacle between two stores: the comparisons issue while the store path takes the store
                    if (AABB_HERE && r < kBoxRegs && r < n_obs) {
                        const double x = v[0], y = v[1], z = v[2];
                        const bool hit = (x >= box[r][0]) && (x <= box[r][1]) && (y >= box[r][2]) && (y <= box[r][3]) &&
                                         (z >= box[r][4]) && (z <= box[r][5]);      // inclusive, minimum_snap.py:352-357
                        coll |= hit ? 1 : 0;
                    }
                }
                if (AABB_HERE) {
                    const double x = v[0], y = v[1], z = v[2];
                    for (int o = kBoxRegs; o < n_obs; ++o) {      // more obstacles than registers hold: the slow way
                        const double *c = aabbs + 6 * o;          // uniform address: scalar loads
                        const bool hit = (x >= c[0]) && (x <= c[1]) && (y >= c[2]) && (y <= c[3]) && (z >= c[4]) &&
                                         (z <= c[5]);            // inclusive, minimum_snap.py:352-357
                        coll |= hit ? 1 : 0;
                    }
                }
            }
            if (WATCH) {
                const double x = src[0], y = src[NU], z = src[2 * NU];
#pragma unroll
                for (int o = 0; o < kBoxRegs; ++o)
                    if (o < n_obs) {
                        const bool hit = (x >= box[o][0]) & (x <= box[o][1]) & (y >= box[o][2]) & (y <= box[o][3]) &
                                         (z >= box[o][4]) & (z <= box[o][5]);       // inclusive, minimum_snap.py:352-357
                        coll |= hit ? 1 : 0;
                    }
                for (int o = kBoxRegs; o < n_obs; ++o) {
                    const double *c = aabbs + 6 * o;
                    const double x0 = c[0], x1 = c[1], y0 = c[2], y1 = c[3], z0 = c[4], z1 = c[5];
                    coll |= ((x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (z >= z0) & (z <= z1)) ? 1 : 0;
                }
            }
            if (LOG_CMD) {
                double v[UAVAC_CMD_COLS];
#pragma unroll
                for (int r = 0; r < UAVAC_CMD_COLS; ++r) v[r] = src[(CMD0 + r) * NU];
                double *dst = cmd_log + (size_t)k * UAVAC_CMD_COLS * sP + col0;
#pragma unroll
                for (int r = 0; r < UAVAC_CMD_COLS; ++r)
                    if (full || mine) store_uniform_base(dst + r * sP, lane_bytes, v[r]);
            }
            if (TGW) {
                constexpr int kStoresPerTick = (LOG_STATE ? 13 : 0) + (LOG_CMD ? UAVAC_CMD_COLS : 0);
                if (t_phase == 0 && t_nrows > 0) {
                    // the compute wave consumed the tile's row in the tick whose slab has just left: commit its share of the yaw
                    // scan and advance the cursor (main.py:61).  A cursor that enters a new segment asks for its coefficients
                    // (LDS-DMA) and for the row count of the segment after (in flight for a whole segment).  This wave has log
                    // stores in flight all the time and vmcnt counts loads and stores in issue order: waiting for "all but the
                    // youngest tick's stores" covers a load that is older than that without waiting for the newest stores.
                    t_yhas = t_yhas_n; t_yprev = t_yprev_n; t_ysum = t_ysum_n;
                    if (t_idx + 1 < t_nrows) {
                        ++t_idx;
                        if (++t_rin >= t_srows && t_seg + 1 < t_pm) {      // next segment (skipping empty ones, like the sampler's segment_of)
                            store_wave_loads_wait<kStoresPerTick>(t_srows_nx);
                            t_rin -= t_srows; ++t_seg; t_srows = t_srows_nx;
                            while (t_rin >= t_srows && t_seg + 1 < t_pm) { t_rin -= t_srows; ++t_seg; t_srows = t_seg_rows[t_seg]; }
                            coeffs_dma(t_coeffs + 24 * t_seg, tile2_lds);
                            seg_rows_issue(t_srows_nx, t_seg_rows + min(t_seg + 1, t_pm - 1));
                            t_asked = 1;
                        }
                        if (!YAWSCAN && t_idx - t_ybase == 16) {
                            t_ybase = t_idx;
#pragma unroll
                            for (int j = 0; j < 16; ++j) yw2[j * 64] = t_yaws[min(t_ybase + j, t_nrows - 1)];
                        }
                    }
                } else if (t_phase >= 1 && t_phase <= 4 && t_nrows > 0) {
                    // the row of the NEXT outer tick, a piece per tick over the four ticks that follow -- at the priority of a
                    // background job, a compute wave may share this SIMD.  (The coefficients asked for a tick ago are older than
                    // this tick's stores.)  The hand-over in the iteration of phase 4 is ordered before the compute wave's read at
                    // the start of its next phase-0 tick by a barrier for F >= 7 in either hand-over mode: with the late
                    // hand-over the compute wave calls barrier j in the middle of tick j + 1, so this wave's iteration k runs
                    // between the middle of tick k + 1 and the middle of tick k + 2.
                    __builtin_amdgcn_s_setprio(0);
                    if (t_phase == 1) {
                        // (only when some lane of the wave did ask for coefficients a tick ago -- 44 % of the outer ticks: the wait is
                        // for the previous tick's STORES as well, and at two workgroups per CU those are not always down yet)
                        if (__any(t_asked)) store_wave_loads_wait<kStoresPerTick>(t_srows_nx);
                        t_asked = 0;
                        t_eval_axis(0);
                    }
                    else if (t_phase == 2) t_eval_axis(1);
                    else if (t_phase == 3) t_eval_axis(2);
                    else t_eval_yaw_and_hand_over();
                    __builtin_amdgcn_s_setprio(3);
                }
                t_phase = (t_phase + 1 == V.F) ? 0 : t_phase + 1;
            }
        }
        if (TGW && mine) {                         // what the other modes' compute wave saves: cursor and the scan as it stands before it
            istate[0 * sB + col0 + lane] = t_idx;
            if (YAWSCAN) {
                state[26 * sB + col0 + lane] = (double)t_idx;
                state[27 * sB + col0 + lane] = t_yhas ? 1.0 : 0.0;
                state[28 * sB + col0 + lane] = t_yprev;
                state[29 * sB + col0 + lane] = t_ysum;
            }
        }
        if (TGW) store_wave_loads_wait<0>(t_srows_nx);       // nothing stays in flight into the tile the next pass reloads
        if (AABB_HERE && mine) istate[2 * sB + col0 + lane] = coll;
      }
        return;
    }

    // ---------------------------------------------------------------------------------- compute waves
    const int tid = threadIdx.x;
    // The constants of the per-tick path, in vector registers (see vk() in control_law.h): with all of VehK in scalar
    // registers the tick loop spilled SGPRs to VGPR lanes (v_readlane / v_writelane, 22 per tick) and rebuilt its fp64
    // literals on every tick (60 s_mov_b32).  The outer block keeps reading its own constants from the kernel arguments.
    VehK L = V;
#pragma unroll
    for (int i = 0; i < 3; ++i) { L.I[i] = vk(V.I[i]); L.inv_I[i] = vk(V.inv_I[i]); L.ikp[i] = vk(V.ikp[i]); }
    L.inv_mass = vk(V.inv_mass);     // (shares its 8-dword kernel-argument group with I[]: left in scalar registers, the whole
                                     // group was spilled and restored with eight v_readlane on every tick)
    L.arm = vk(V.arm); L.inv_arm = vk(V.inv_arm); L.kappa = vk(V.kappa); L.inv_kappa = vk(V.inv_kappa);
    L.kf = vk(V.kf); L.inv_kf = vk(V.inv_kf);
    L.lit_tiny = vk(V.lit_tiny); L.lit_h2_small = vk(V.lit_h2_small); L.lit_c8 = vk(V.lit_c8); L.lit_c6 = vk(V.lit_c6);
    L.lit_c4 = vk(V.lit_c4); L.lit_s9 = vk(V.lit_s9); L.lit_s7 = vk(V.lit_s7); L.lit_s5 = vk(V.lit_s5); L.lit_s3 = vk(V.lit_s3);
    L.lit_375 = vk(V.lit_375); L.lit_e_small = vk(V.lit_e_small);
    // The plan's sample period, used once per OUTER tick: in a vector register too in the kernels that log.  Left in scalar
    // registers it costs four v_readlane per outer tick -- and the bench launch shape 2.6 % at B = 4 096 (0.853 against 0.831
    // ms per 1 000 ticks, A/B in one process, tools/rollout_ab.py).  The kernels without a second wave keep it scalar: they
    // sit at the 256-register limit of two waves per SIMD (tests/test_abi_and_host.py checks that budget).
    const double plan_dt = !POLY ? 0.0 : (LOGGING ? vk(P.dt) : P.dt);
  for (int tile0 = 0; tile0 < n_tiles; tile0 += grid, kk += K) {
    const int n_here = min(grid, n_tiles - tile0);
    if ((int)blockIdx.x >= n_here) break;
    const int col0 = (tile0 + xcd_contiguous(blockIdx.x, n_here)) * NU;
    const int b = col0 + tid;
    const bool live = b < B;
    const int bb = live ? b : B - 1;                                   // dead lanes shadow the last UAV, store nothing

    double px = state[0 * sB + bb], py = state[1 * sB + bb], pz = state[2 * sB + bb];
    double q0 = state[3 * sB + bb], q1 = state[4 * sB + bb], q2 = state[5 * sB + bb], q3 = state[6 * sB + bb];
    double vx = state[7 * sB + bb], vy = state[8 * sB + bb], vz = state[9 * sB + bb];
    double wp = state[10 * sB + bb], wq = state[11 * sB + bb], wr = state[12 * sB + bb];
    double om[4], omc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { om[i] = state[(13 + i) * sB + bb]; omc[i] = state[(17 + i) * sB + bb]; }
    double integ = state[21 * sB + bb];
    double thrust_cmd = state[22 * sB + bb];
    double pc = state[23 * sB + bb], qc = state[24 * sB + bb], rc = state[25 * sB + bb];
    int idx = istate[0 * sB + bb];
    int inner = istate[1 * sB + bb];
    int collided = istate[2 * sB + bb];
    int gbits = GROUND ? istate[3 * sB + bb] : 0;

    const int64_t off = row_offsets[bb];
    const int nrows = (int)(row_offsets[bb + 1] - off);
    const double *rows = traj + off * UAVAC_TRAJ_COLS;
    int phase = inner % V.F;

    // SCORE: this lane's scores into its column of the slot (after the TGW target tile).  A period left pending by an earlier
    // launch resumes only at the very tick that launch stopped before (row 7: no tick ran in between, unscored ones included);
    // otherwise it is dropped.  (The period's first tick alone could not tell: an unscored launch inside the period keeps it.)
    double *sc = slab + (size_t)2 * NR * NU + (POLY ? (size_t)CW * poly_tile_doubles(YAWSCAN) : 0) + (TGW ? (size_t)tgt_rows(SCORE) * NU : 0) +
                 (tid & 63);
    if (SCORE) {
        double s[kScoreRows];
#pragma unroll
        for (int r = 0; r < kScoreRows; ++r) s[r] = score[r * sB + bb];
        if (s[6] != 0.0 && !(phase != 0 && s[7] == (double)inner)) s[6] = 0.0;
#pragma unroll
        for (int r = 0; r < kScoreRows; ++r) sc[r * 64] = s[r];
    }

    // Make every load above land before the tick loop: a load still pending at the loop header would be
    // waited for with vmcnt at its first use inside the loop on EVERY iteration, and those waits would also
    // expose the latency of the (asm-issued, compiler-invisible) row prefetch.
    settle(px); settle(py); settle(pz); settle(q0); settle(q1); settle(q2); settle(q3); settle(vx); settle(vy);
    settle(vz); settle(wp); settle(wq); settle(wr); settle(integ); settle(thrust_cmd); settle(pc); settle(qc);
    settle(rc);
#pragma unroll
    for (int i = 0; i < 4; ++i) { settle(om[i]); settle(omc[i]); }
    settle(idx); settle(phase); settle(collided);

    constexpr bool BOX_HERE = AABB && !((LOG_STATE || WATCH) && CW == SW);

    RowRegs nxt;
    if (!POLY && nrows > 0) row_issue(nxt, rows + (size_t)min(max(idx, 0), nrows - 1) * UAVAC_TRAJ_COLS);

    // POLY: segment / row-in-segment of the cursor, the segment's coefficients and the next 16 yaws, in LDS
    // this wave's coefficient tile: [24][64] doubles, or -- filled by LDS-DMA -- [12][64][2] (minsnap_eval.h, STRIDE 0)
    constexpr int CST = ADMA ? 0 : 64;
    double *tile = slab + (size_t)2 * NR * NU + (size_t)(tid >> 6) * poly_tile_doubles(YAWSCAN);
    double *cf = tile + (ADMA ? 2 : 1) * (tid & 63);                                                    // this lane's first coefficient
    double *yw = tile + 24 * 64 + (tid & 63);                                                           // yw[j * 64]
    const unsigned tile_lds = ADMA ? (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)tile) : 0u;   // LDS byte address (low half of the generic pointer)
    // segments of this lane's mission: P.m of them at bb * P.m, or -- ragged batch -- seg_offsets[bb + 1] - seg_offsets[bb]
    // of them at seg_offsets[bb] (clamped to 1 .. P.m, the batch's maximum)
    int pm = P.m;
    size_t seg0 = (size_t)bb * P.m;
    if (POLY && P.seg_offsets) {
        seg0 = (size_t)P.seg_offsets[bb];
        const int64_t n_ = P.seg_offsets[bb + 1] - P.seg_offsets[bb];
        pm = (int)(n_ < 1 ? 1 : (n_ > P.m ? P.m : n_));
    }
    const int32_t *seg_rows = POLY ? P.seg_rows + seg0 : nullptr;
    const double *mission_coeffs = POLY ? P.coeffs + seg0 * 24 : nullptr;
    const double *yaws = (POLY && !YAWSCAN) ? P.yaw + off : nullptr;
    int seg = 0, rin = 0, srows = 0, ybase = 0;
    int srows_nx = 0;                              // rows of segment seg + 1 (in flight from the moment seg is entered: plan_loads_wait)
    auto load_coeffs = [&](int s_) {               // through registers, on the spot: launch start and the scan's rebuild only
        const double *src = mission_coeffs + 24 * s_;
#pragma unroll
        for (int j = 0; j < 24; ++j) cf[minsnap_coeff_index<CST>(j)] = src[j];
    };
    auto load_yaws = [&](int base_) {
#pragma unroll
        for (int j = 0; j < 16; ++j) yw[j * 64] = yaws[min(base_ + j, nrows - 1)];
    };
    // YAWSCAN: the carried scan (state rows 26-29)
    int yhas = 0;
    double yprev = 0.0, ysum = 0.0, first_yaw = 0.0;
    if (POLY && !TGW && nrows > 0) {
        idx = min(max(idx, 0), nrows - 1);
        if (YAWSCAN) {
            first_yaw = P.first_yaw[bb];
            const double scan_row = state[26 * sB + bb];
            if (scan_row == (double)idx) {
                yhas = state[27 * sB + bb] != 0.0;
                yprev = state[28 * sB + bb];
                ysum = state[29 * sB + bb];
            } else {
                // the cursor is not where the carried scan stands: rebuild it from the mission's first row (rare: a
                // caller moved the cursor, or a launch without YAWSCAN advanced it)
                int s_ = 0, r_ = 0, n_ = seg_rows[0];
                load_coeffs(0);
                for (int row = 0; row < idx; ++row) {
                    while (r_ >= n_ && s_ + 1 < pm) { r_ -= n_; ++s_; n_ = seg_rows[s_]; load_coeffs(s_); }
                    double x_, y_, z_, vx_, vy_, vz_, ax_, ay_, az_;
                    minsnap_eval_row<CST>(cf, (double)r_ * plan_dt, x_, y_, z_, vx_, vy_, vz_, ax_, ay_, az_);
                    if (uavac_yaw::has_heading(vx_, vy_)) {
                        const double a_ = atan2(vy_, vx_);
                        if (yhas) ysum = ysum + uavac_yaw::unwrap_correction(a_ - yprev);
                        yhas = 1;
                        yprev = a_;
                    }
                    ++r_;
                }
            }
        }
        rin = idx;
        srows = seg_rows[0];
        while (seg + 1 < pm && rin >= srows) { rin -= srows; ++seg; srows = seg_rows[seg]; }
        load_coeffs(seg);
        if (ADMA) srows_nx = seg_rows[min(seg + 1, pm - 1)];
        if (!YAWSCAN) {
            ybase = idx;
            load_yaws(ybase);
        }
    }
    if (POLY && ADMA) settle(srows_nx);

    // 1/|q|^2 of the caller-supplied attitude; the free-body step leaves q unit, so 1 from then on
    // (a state this kernel wrote earlier is unit to rounding: take exactly 1 so that splitting a rollout over
    // launches is bit-identical to one launch)
    const double qn2 = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3;
    double inv_n2 = (fabs(qn2 - 1.0) < 1.0e-12) ? 1.0 : 1.0 / qn2;

    // TGW: the target row of the next outer tick, put there by the second wave (which also owns the cursor)
    const double *tgt = slab + (size_t)2 * NR * NU + (size_t)CW * poly_tile_doubles(YAWSCAN) + (tid & 63);
    if (TGW) lds_barrier();                        // the first row is in the tile
    for (int k = 0; k < K; ++k) {
        if (phase == 0 && nrows > 0) {
            // ------------------------------------------------------------- outer loop (main.py:47-61)
            double tg_x, tg_y, tg_z, tg_vx, tg_vy, tg_vz, tg_ax, tg_ay, tg_az, tg_yaw;
            if (TGW) {
                tg_x = tgt[0]; tg_y = tgt[64]; tg_z = tgt[128]; tg_vx = tgt[192]; tg_vy = tgt[256]; tg_vz = tgt[320];
                tg_ax = tgt[384]; tg_ay = tgt[448]; tg_az = tgt[512]; tg_yaw = tgt[576];
            } else if (POLY) {
                if (ADMA) plan_loads_wait(srows_nx);            // coefficients (and row count) asked for an outer tick ago have landed
                minsnap_eval_row<CST>(cf, (double)rin * plan_dt, tg_x, tg_y, tg_z, tg_vx, tg_vy, tg_vz, tg_ax, tg_ay, tg_az);
                if (YAWSCAN) {
                    // this row's yaw from the carried scan (minimum_snap.py:126-136); committed below only if the cursor moves on
                    const bool yvalid = uavac_yaw::has_heading(tg_vx, tg_vy);
                    const double yang = yvalid ? atan2(tg_vy, tg_vx) : 0.0;
                    const double ycum = (yvalid && yhas) ? ysum + uavac_yaw::unwrap_correction(yang - yprev) : ysum;
                    tg_yaw = yvalid ? yang + ycum : (yhas ? yprev + ysum : first_yaw);
                    if (idx + 1 < nrows) {
                        if (yvalid) { yhas = 1; yprev = yang; }
                        ysum = ycum;
                    }
                } else {
                    tg_yaw = yw[(idx - ybase) * 64];
                }
            } else {
                row_wait(nxt);
                tg_x = row_col(nxt, 0); tg_y = row_col(nxt, 1); tg_z = row_col(nxt, 2);
                tg_vx = row_col(nxt, 3); tg_vy = row_col(nxt, 4); tg_vz = row_col(nxt, 5);
                tg_ax = row_col(nxt, 6); tg_ay = row_col(nxt, 7); tg_az = row_col(nxt, 8);
                tg_yaw = row_col(nxt, 9);
            }
            if (SCORE) {                                // a period starts: its row (+ 1) and target xyz
                const int r = TGW ? (int)tgt[640] : (POLY ? idx : min(max(idx, 0), nrows - 1));
                sc[6 * 64] = (double)(r + 1);
                sc[8 * 64] = tg_x; sc[9 * 64] = tg_y; sc[10 * 64] = tg_z;
            }

            const VehK O = outer_constants();
            const Rot R = quat_to_rot(q0, q1, q2, q3);                 // shared by altitude and attitude
            thrust_cmd = altitude(O, tg_z, tg_vz, tg_az, pz, vz, R.r22, integ);
            double bxc, byc;
            lateral(O, tg_x, tg_vx, tg_ax, tg_y, tg_vy, tg_ay, px, py, vx, vy, thrust_cmd, bxc, byc);
            roll_pitch(O, bxc, byc, R, pc, qc);
            double psi, cth, sphi, cphi;
            euler_trig(q0, q1, q2, q3, psi, cth, sphi, cphi);
            rc = yaw_rate(O, tg_yaw, psi, cth, sphi, cphi, qc);
            // next row (main.py:61), consumed F ticks from now; issued last so that nothing in this block
            // still reads the registers it overwrites
            if (TGW) {
                // (the second wave advances the cursor)
            } else if (POLY) {
                if (idx + 1 < nrows) {                    // main.py:61: the cursor stops on the last row
                    ++idx;
                    if (++rin >= srows) {                 // next segment (skipping empty ones, like the sampler's segment_of)
                        if (!ADMA) {                      // full chip: through registers, on the spot (see the launcher)
                            while (rin >= srows && seg + 1 < pm) { rin -= srows; ++seg; srows = seg_rows[seg]; }
                            load_coeffs(seg);
                        } else if (seg + 1 < pm) {
                            rin -= srows; ++seg; srows = srows_nx;             // (its row count came with the segment before)
                            while (rin >= srows && seg + 1 < pm) { rin -= srows; ++seg; srows = seg_rows[seg]; }    // empty segments: rare, on the spot
                            coeffs_dma(mission_coeffs + 24 * seg, tile_lds);   // lands in this lane's column while the inner ticks run
                            seg_rows_issue(srows_nx, seg_rows + min(seg + 1, pm - 1));
                        }
                    }
                    if (!YAWSCAN && idx - ybase == 16) { ybase = idx; load_yaws(ybase); }
                }
            } else {
                idx = min(idx + 1, nrows - 1);
                row_issue(nxt, rows + (size_t)idx * UAVAC_TRAJ_COLS);
            }
        }

        // ----------------------------------------------------------------- inner loop, every tick
        double Mx, My, Mz, f[4];
        body_rate(L, pc, qc, rc, wp, wq, wr, Mx, My, Mz);
        allocate(L, thrust_cmd, Mx, My, Mz, f);
        motors(L, f, om, omc);
        // late hand-over: slab k-1 goes to the store wave HERE, a third of a tick after it was written -- the barrier's wait for
        // this wave's LDS writes then finds nothing outstanding (the launcher says when that pays)
        if (LOGGING && late_handover && k > 0) lds_barrier();

        double *my = LOGGING ? slab + (size_t)((kk + k) & 1) * NR * NU + tid : nullptr;
        if (LOG_CMD) {
            double *c = my + CMD0 * NU;
            c[0] = thrust_cmd; c[1 * NU] = pc; c[2 * NU] = qc; c[3 * NU] = rc;
#pragma unroll
            for (int i = 0; i < 4; ++i) { c[(4 + i) * NU] = omc[i]; c[(8 + i) * NU] = om[i]; }
        }

        free_body_step<GROUND>(L, om, px, py, pz, q0, q1, q2, q3, vx, vy, vz, wp, wq, wr, inv_n2);
        inv_n2 = 1.0;
        if (GROUND) gbits = ground_bits(L, pz, gbits);
        if (SCORE && phase + 1 == V.F) score_period_end(sc, px, py, pz);

        if (WATCH) { my[0] = px; my[1 * NU] = py; my[2 * NU] = pz; }
        if (BOX_HERE) {                                   // only with a command log alone; otherwise the second wave tests
            for (int o = 0; o < n_obs; ++o) {
                const double *c = aabbs + 6 * o;          // uniform address: scalar loads
                // all six bounds first, then six comparisons combined without short-circuit: one scalar-cache round
                // trip per obstacle (written with && it was one per BOUND: load, wait, compare, branch, six times)
                const double x0 = c[0], x1 = c[1], y0 = c[2], y1 = c[3], z0 = c[4], z1 = c[5];
                const bool hit = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (pz >= z0) &
                                 (pz <= z1);              // inclusive, minimum_snap.py:352-357
                collided |= hit ? 1 : 0;
            }
        }

        if (LOG_STATE) {
            my[0] = px; my[1 * NU] = py; my[2 * NU] = pz;
            my[3 * NU] = q0; my[4 * NU] = q1; my[5 * NU] = q2; my[6 * NU] = q3;
            my[7 * NU] = vx; my[8 * NU] = vy; my[9 * NU] = vz;
            my[10 * NU] = wp; my[11 * NU] = wq; my[12 * NU] = wr;
        }
        if (LOGGING && !late_handover) lds_barrier();        // hand slab (kk+k)&1 to the store wave; it was drained two ticks ago
        ++inner;
        phase = (phase + 1 == V.F) ? 0 : phase + 1;
    }
    if (LOGGING && late_handover && K > 0) lds_barrier();      // the last slab

    // nothing may stay in flight into these registers.  UNCONDITIONAL (not `if (nrows > 0)`, the mask the loads were issued under):
    // the build check follows the control-flow graph and cannot know that a skipped wait belongs to a skipped issue -- every path
    // from an issue site to the next pass or to the end of the kernel must cross a wait (a wave without rows waits for nothing)
    if (!POLY) row_wait(nxt);
    if (POLY && ADMA) plan_loads_wait(srows_nx);    // ... nor into this wave's coefficient tile (the next pass, or nobody, owns it)
    if (live) {
    state[0 * sB + b] = px; state[1 * sB + b] = py; state[2 * sB + b] = pz;
    state[3 * sB + b] = q0; state[4 * sB + b] = q1; state[5 * sB + b] = q2; state[6 * sB + b] = q3;
    state[7 * sB + b] = vx; state[8 * sB + b] = vy; state[9 * sB + b] = vz;
    state[10 * sB + b] = wp; state[11 * sB + b] = wq; state[12 * sB + b] = wr;
#pragma unroll
    for (int i = 0; i < 4; ++i) { state[(13 + i) * sB + b] = om[i]; state[(17 + i) * sB + b] = omc[i]; }
    state[21 * sB + b] = integ;
    state[22 * sB + b] = thrust_cmd;
    state[23 * sB + b] = pc; state[24 * sB + b] = qc; state[25 * sB + b] = rc;
    if (!TGW) istate[0 * sB + b] = idx;            // (TGW: the second wave owns and saves the cursor)
    istate[1 * sB + b] = inner;
    if (!AABB || BOX_HERE) istate[2 * sB + b] = collided;
    if (GROUND) istate[3 * sB + b] = gbits;
    if (POLY && YAWSCAN && !TGW) {
        state[26 * sB + b] = (double)idx;
        state[27 * sB + b] = yhas ? 1.0 : 0.0;
        state[28 * sB + b] = yprev;
        state[29 * sB + b] = ysum;
    }
    if (SCORE) {
#pragma unroll
        for (int r = 0; r < kScoreRows; ++r) score[r * sB + b] = r == 7 ? (double)inner : sc[r * 64];   // row 7: where this launch stopped
    }
    }
  }
