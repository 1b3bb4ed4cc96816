// The body of gemv_quad_kernel (lnb_kernels.hip), included once per kernel: LNB_QUAD_REPORT false in the production kernel, true in gemv_quad_report_kernel.
// TIMING (a constant of the including kernel): true in the instantiation launched when GemvParams.dbg is set -- the stamps and timed barriers exist only there
// (the norm's report compiled in, lnb_op_rmsnorm_sum).  Text, not a function: routed through an inlined body function hipcc allocated the production
// kernels' registers differently, and their code is to stay what it was.  No include guard: it is meant to be included twice.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long t_begin = LNB_DBG ? clock64() : 0, t_wait = 0, t_x = 0, t_aux = 0;
    const long long t_wall0 = LNB_DBG ? (long long)wall_clock64() : 0;
    constexpr int NCW = gq_ncw(RW), NW = NCW + NH;
    constexpr int KC = KS / 8;                            // 8-wide k chunks per stage
    constexpr int GS = KS / 16;                           // 16-step groups per stage
    constexpr int SA = RW * KS * 2;                       // bf16 bytes per stage
    constexpr int SB = 2 * SA;                            // f32 product bytes per stage
    constexpr int UNITS = RW * KC;                        // 16-byte weight units per stage
    constexpr int NP = UNITS / (64 * NH);                 // loads per lane per stage per helper
    static_assert(RW % 8 == 0 && KS % 16 == 0, "rows in eights (conflict-free product writes), whole 16-step groups");
    static_assert(UNITS % (64 * NH) == 0 && R * NP <= 60, "vmcnt is a 6-bit counter");
    static_assert(NH >= 2 && GS >= 4 && GS % 4 == 0, "stage geometry");
    char* ringB = smem;
    float* xs = (float*)(smem + GQ_SLOTS * SB);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int K = p.K, S = p.S;
    const int m = (S == 1) ? 0 : (int)(blockIdx.x % (unsigned)S);
    const int wg = (S == 1) ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)S);
    const size_t stream_bytes = (size_t)K * RW * 2;
    const int nstages = (int)((stream_bytes + SA - 1) / SA);
    const int nb_mine = (p.n_blocks - wg + p.n_wg - 1) / p.n_wg;       // row blocks wg, wg+n_wg, ...
    const int T = nb_mine * nstages;                                   // stages of this workgroup
    constexpr int NS = NW;                                             // every wave stages x
    const int kpad = nstages * KS + 320;                               // launcher guarantees kpad <= X_CH*NS*512
    const uint16_t* xrow = p.x + (size_t)m * K;

    if (wave >= NCW) {
        // ================================ helper waves ============================================
        const int hw = wave - NCW;
        u32x4 buf[R][NP];
        uint4 xv[XC], nv[XC];
        x_issue<NORM, NS>(p, xrow, wave, lane, xv, nv);
        __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0): x (and the norm weights) have landed (see gemv_chain_kernel)
        const size_t last16 = stream_bytes - 16;
        unsigned loff[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) loff[i] = (unsigned)(((i * NH + hw) * 64 + lane) * 16);
        int ib = wg, is = 0, issued = 0;
        auto issue_next = [&](u32x4 (&dst)[NP]) {
            const size_t soff = (size_t)is * SA;
            const char* sb = (const char*)p.w + (size_t)ib * stream_bytes + soff;     // wave-uniform
            const unsigned lim = (soff + SA <= stream_bytes) ? 0xFFFFFFFFu : (unsigned)(last16 - soff);
#pragma unroll
            for (int i = 0; i < NP; i++) ld_nt_asm(dst[i], loff[i] < lim ? loff[i] : lim, sb);
            if (issued + 1 < T) { issued++; if (++is == nstages) { is = 0; ib += p.n_wg; } }
        };
        constexpr bool late = NORM;                                    // the weight stream starts behind the norm's fold (see gemv_chain_kernel)
        constexpr int EARLY = late ? (LNB_EARLY_QUAD < R ? LNB_EARLY_QUAD : R) : R;
#pragma unroll
        for (int j = 0; j < EARLY; j++) issue_next(buf[j]);
        x_store<NORM, NS>(p, xs, kpad, wave, lane, xv);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        TIMED_BARRIER();                                               // B1: xs (or the squares) are in LDS
        if (NORM) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            rms_fold<rms_nf(NH), LNB_QUAD_REPORT, TIMING>(p, xs, ringB, hw < rms_nf(NH) ? hw : -1, lane, t_aux);      // X1, X2 inside; the first four helpers fold (four consecutive waves: four SIMDs)
            {                                                          // the walker walks now: the issue stall costs nothing here
#pragma unroll
                for (int j = EARLY; j < R; j++) issue_next(buf[j]);
            }
            TIMED_BARRIER();                                           // B2: r published
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if constexpr (NORM) x_normalize<NS>(p, xs, kpad, xs[kpad], wave, lane, xv, nv);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            TIMED_BARRIER();                                           // B3: xs normalised
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // unit of load i: q = kc*RW + r (stage-local k-chunk kc, row r); its eight products are the slots j0, j0+1 of group kc/2
        unsigned doff[NP]; int xoff[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int q = (i * NH + hw) * 64 + lane, kc = q / RW, r = q % RW;
            const int j0 = (kc & 1) * 2, sw = (r >> 1) & 3;
            doff[i] = (unsigned)((((kc >> 1) * RW + r) * 4 + (j0 ^ sw)) * 16);      // slot j0+1 sits at doff ^ 16 (j0 is even)
            xoff[i] = kc * 8;
        }
        int st = 0;                                        // stage-in-block of the stage being converted
        for (int it0 = 0; it0 <= T + 1; it0 += R) {
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int t = it0 + j;
                if (t <= T + 1) {
                    if (t < T) {
                        const long long tb_ = LNB_DBG_FULL ? clock64() : 0;
                        wait_ring<(R - 1) * NP, NP>(buf[j]);           // stage t landed; R-1 younger stages stay in flight
                        if (LNB_DBG_FULL) t_x += clock64() - tb_;
                        char* dst = ringB + (size_t)(t % GQ_SLOTS) * SB;
                        const float* xst = xs + (size_t)st * KS;
                        float4 xa[NP], xb[NP];
#pragma unroll
                        for (int i = 0; i < NP; i++) { xa[i] = *(const float4*)(xst + xoff[i]); xb[i] = *(const float4*)(xst + xoff[i] + 4); }
#pragma unroll
                        for (int i = 0; i < NP; i++) {
                            const u32x4 v = buf[j][i];
                            // exact products (8-bit x 8-bit significands): val1F32 * val2F32, operations_lineartransform.go:60
                            *(float4*)(dst + doff[i]) = mul4(xa[i], bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
                            *(float4*)(dst + (doff[i] ^ 16u)) = mul4(xb[i], bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w));
                        }
                        if (++st == nstages) st = 0;
                        __builtin_amdgcn_sched_barrier(0);             // refill AFTER the slot has been consumed (no register copies)
                        issue_next(buf[j]);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // ds_writes complete before the barrier
                    TIMED_BARRIER();
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");
        DBG_EXIT();
        return;
    }
    // ==================================== chain waves ==================================================
    {
        if constexpr (NORM && LNB_QUAD_REPORT) if (wave == 0) rms_report_park<rms_nf(NH)>(p, ringB, wg == 0 ? m : -1, lane);
        uint4 xv[XC], nv[XC];
        x_issue<NORM, NS>(p, xrow, wave, lane, xv, nv);
        LNB_STAMP(0);
        x_store<NORM, NS>(p, xs, kpad, wave, lane, xv);
        LNB_STAMP(1);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        TIMED_BARRIER();                                               // B1
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        LNB_STAMP(2);
        if (NORM) {
            float r;
#ifdef LNB_PROBE_WARM_XNORM
            // measurement only (tools/build_variant.sh warm -DLNB_PROBE_WARM_XNORM, profiles/prologue_fetch.md): the chain waves that idle until the walker is done run
            // the ONE copy of the x_normalize code below twice -- first with r = 1 into the third product slot (unused until B3), so that the real pass behind B2
            // finds its instructions fetched.  `warm` is opaque to the compiler: a peeled first pass would be a second copy of the code and warm nothing.
            int warm = __builtin_amdgcn_readfirstlane((wave != 0 && kpad * 4 <= SB) ? 1 : 0), warmed = 0;
            asm volatile("" : "+s"(warm));
            float* xdst = xs;
            for (;;) {
                if (warm) {
                    __builtin_amdgcn_s_barrier(); __builtin_amdgcn_s_barrier();     // X1, X2
                    r = 1.0f; xdst = (float*)(ringB + 2 * SB); warmed = 1;
                } else if (wave == 0) {
                    r = rms_scale_wide<rms_nf(NH), LNB_QUAD_REPORT ? 2 : 0, TIMING>(p, xs, ringB, lane, t_aux);     // X1, X2 inside
                    LNB_STAMP(3);
                    if (lane == 0) xs[kpad] = r;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    TIMED_BARRIER();                                   // B2
                    LNB_STAMP(4);
                } else {
                    if (!warmed) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_s_barrier(); }     // X1, X2
                    TIMED_BARRIER();                                   // B2
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    r = xs[kpad]; xdst = xs;
                    LNB_STAMP(4);
                }
                x_normalize<NS>(p, xdst, kpad, r, wave, lane, xv, nv);
                if (!warm) break;
                warm = 0;
            }
#else
            if (wave == 0) {
                r = rms_scale_wide<rms_nf(NH), LNB_QUAD_REPORT ? 2 : 0, TIMING>(p, xs, ringB, lane, t_aux);     // X1, X2 inside
                LNB_STAMP(3);
                if (lane == 0) xs[kpad] = r;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                TIMED_BARRIER();                                       // B2
                LNB_STAMP(4);
            } else {
                __builtin_amdgcn_s_barrier(); __builtin_amdgcn_s_barrier();     // X1, X2
                TIMED_BARRIER();                                       // B2
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                r = xs[kpad];
            }
            if constexpr (NORM) x_normalize<NS>(p, xs, kpad, r, wave, lane, xv, nv);
#endif
            LNB_STAMP(5);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            TIMED_BARRIER();                                           // B3
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            LNB_STAMP(6);
        }
    }
    if (LNB_DBG) { t_x = clock64() - t_begin; t_wait = 0; }              // (chain waves report the barrier wait of the main loop only)
    __builtin_amdgcn_s_setprio(3);
    constexpr int last_rows = RW - 16 * (NCW - 1);                     // rows of the last chain wave
    const int rows_here = wave == NCW - 1 ? last_rows : 16;
    const int rq = (lane >> 2) % rows_here, row = wave * 16 + rq, jq = lane & 3;
    const char* const src0 = ringB + (size_t)((row * 4 + (jq ^ ((row >> 1) & 3))) * 16);
    float acc[1] = {0.0f};
    float4 pq[4];
    int st = 0, blk = wg;
    for (int it = 0; it <= T + 1; it++) {
        if (it >= 2) {
            const char* cur = src0 + (size_t)((it - 2) % GQ_SLOTS) * SB;
            const char* nxt = src0 + (size_t)((it - 1) % GQ_SLOTS) * SB;       // complete since the last barrier (past the end: stale bytes, never added)
            if (it == 2) { pq[0] = *(const float4*)cur; pq[1] = *(const float4*)(cur + RW * 64); pq[2] = *(const float4*)(cur + 2 * RW * 64); }
#pragma unroll
            for (int g = 0; g < GS; g++) {
                pq[(g + 3) & 3] = g + 3 < GS ? *(const float4*)(cur + (g + 3) * (RW * 64)) : *(const float4*)(nxt + (g + 3 - GS) * (RW * 64));
                __builtin_amdgcn_sched_barrier(0);                     // the read is issued HERE, three groups ahead of its adds
                chain16q(acc[0], pq[g & 3]);                           // valDstF32 += p, k ascending (operations_lineartransform.go:63)
                __builtin_amdgcn_sched_barrier(0);
            }
            if (++st == nstages) {                                     // end of a row block: write it out, start the next
                gemv_epilogue<1, EPI, 4>(p, acc, m, blk * RW + row, jq == 0 && lane < rows_here * 4 && blk * RW + row < p.n_rows);
                acc[0] = 0.0f; st = 0; blk += p.n_wg;
            }
        }
        TIMED_BARRIER();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    DBG_EXIT();
