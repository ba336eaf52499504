/* ========================================================================
 * rx_pipe2.hip -- rx_pipe2_kernel: the receive pipeline (rx_pipe.h) laid out for up to 32 frames per workgroup (BASELINE config 4's per-GPU
 * share: 8192 frames = 32 per CU), where the recurrence costs the serial wave no more than for 16 frames and the
 * FILTER decides the time.  Measured on rx_fused_pipe_kernel's layouts: a FIR wave alone on its SIMD issues a
 * packed instruction every 6.2 cycles (every LDS instruction costs it ~15), two on one SIMD 4.07 between them (the
 * SIMD's rate); the serial wave loses half its speed as soon as anything shares its SIMD.  Hence:
 *   wave 0            the serial wave, alone on its SIMD (hardware waves 4 and 8 retire at once);
 *   hardware waves 1-3, 5-7, 9-11   up to nine FIR waves, two or three on each of the other SIMDs;
 *   unit              2 frames x 64 symbols of one chunk, lane = (frame of 2) x (q of 32), 2 symbols per lane.
 *                     FIR wave i owns units i, i + nfir (static), so SIMDs 1-3 carry 6, 5, 5 of a full
 *                     workgroup's 16 units.
 * What makes 32 frames fit the 160 KB: the window (hist + one chunk of samples, 5.4 KB per frame) belongs to the
 * WAVE, not the frame -- a wave stages, filters and hands over one unit after the other in the same 10.9 KB -- and
 * the 126 samples of history a frame carries from chunk to chunk stay in the owner's REGISTERS (they are the last
 * 128-sample block it loaded: 4 VGPRs per frame), so there is no history copy through LDS and no window to zero.
 * Rings, records, flush and the serial wave are those of rx_fused_pipe_kernel (costas_wave, flush_records).
 * ======================================================================== */
#include "rx_pipe2_geom.h"     /* the unit geometry (namespace pipe2), shared with rx_lean.hip and rx_hist.hip */
#include "fir_r2_asm.h"        /* the FIR step of a unit */

#ifndef QPSK_PIPE2_ASM
#define QPSK_PIPE2_ASM 1     /* 1: the FIR step as the generated instruction stream fir_r2_asm.h; 0: the compiler's (A/B builds) */
#endif
#ifndef QPSK_PIPE2_DEPTH
#define QPSK_PIPE2_DEPTH 1   /* blocks of 8 window positions fetched ahead of their use (measured: see DESIGN.md 4.1) */
#endif

namespace qpsk {

/* register budget of the generated stream (tools/gen_fir_asm.py): kernels with three waves per SIMD have 168 VGPRs; the serial wave's
 * stream (costas_asm.h) owns v100..v143 of its own wave only */
static_assert(FIR_R2_ASM_END_VGPR <= 168, "rx_pipe2_kernel: three FIR waves per SIMD");

/* NUW = units of this wave, unrolled: each unit's state (8 VGPRs of history, a few scalars) has its own registers.
 * [Measured and not kept: ONE copy of the unit's code with the state selected per iteration -- 47 KB of kernel
 * instead of 79 KB, no more instruction fetches beyond the cache two CUs share (the unrolled form reads 6 % more
 * bytes than the batch holds, PMC FETCH_SIZE) -- but the register allocator then reloads spilled loop invariants
 * right behind the sample prefetch, and a scratch reload waits for every load issued before it: 0.356 against
 * 0.32 ms at 8192 frames on the same box.] */
template <int NUW>
__device__ __forceinline__ void fir_wave2(const FusedArgs &a, Smem *sm, float2 *mywin, float2 *dring, float *zring, int G,
                                          int widx, int u0, int f0, int lane, int nchunks, int *status)
{
    constexpr int nuw = NUW;
    using namespace pipe2;
    using GM = GeomNarrow;    /* ring geometry (S, DSTRIDE, ZSTRIDE) shared with costas_wave / flush_records */
    constexpr int DSTRIDE = GM::DSTRIDE;
    const int L = a.frame_size;
    const int fl = lane / QL, q = lane % QL;
    const bool simd0 = ((threadIdx.x >> 6) & 3) == 0;       /* a FIR wave placed beside the serial wave (layout) */
    const float4 *taps4 = reinterpret_cast<const float4 *>(sm->taps);
    const float2 *rd = mywin + fl * WS + (PAD + PADS) * q;   /* FIR read base: position PAD*q -> slot (PAD+PADS)*q */

    Unit un[NUW];
#pragma unroll
    for (int ui = 0; ui < NUW; ui++) {
        Unit &U = un[ui];
        U.u = u0 + ui;
        U.all_valid = UF * U.u + UF <= G && f0 + UF * U.u + UF <= a.nframes;
#pragma unroll
        for (int ff = 0; ff < UF; ff++) {
            const int fr = f0 + UF * U.u + ff;
            U.fv[ff] = UF * U.u + ff < G && fr < a.nframes;      /* an odd G leaves the last unit one frame */
            const int ix = checked_index(a.index ? (U.fv[ff] ? a.index[fr] : 0) : a.fixed_index, a.status);   /* decimation offset, < C */
            U.ix[ff] = __builtin_amdgcn_readfirstlane(ix);
            U.src[ff] = reinterpret_cast<const float4 *>(a.x + (size_t)(U.fv[ff] ? fr : 0) * a.frame_pitch);
            U.hist[ff] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);       /* a fresh delay line (qpsk.c:37) */
        }
    }

    /* loads are UNCONDITIONAL (a per-load branch would make the compiler wait for each in turn): a chunk that lies
     * inside every frame of the unit loads straight; the tail chunk clamps the address and zeroes what lies past the
     * end.  L is even on this path (host-checked), so a 16-byte pair is either inside the frame or past it. */
    auto prefetch = [&](const Unit &U, float4 (&pre)[UF][NLD], int c) {
        if (U.all_valid && (c + 1) * CH <= L) {
#pragma unroll
            for (int ff = 0; ff < UF; ff++)
#pragma unroll
                for (int j = 0; j < NLD; j++)
                    pre[ff][j] = load_once(&U.src[ff][(c * CH + 128 * j + 2 * lane) >> 1]);
        } else {
#pragma unroll
            for (int ff = 0; ff < UF; ff++)
#pragma unroll
                for (int j = 0; j < NLD; j++) {
                    const int s = c * CH + 128 * j + 2 * lane;
                    const bool in = U.fv[ff] && s + 1 < L;
                    float4 v = load_once(&U.src[ff][in ? (s >> 1) : 0]);
                    if (!in) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    pre[ff][j] = v;
                }
        }
    };

    prof::FirProbe probe(a);      /* the measurement build's cycle accounting of this wave (rx_profile.h); nothing in the product */

    /* one unit of one chunk: stage the window from registers, start the next loads, filter, flush what the loop has
     * finished with, hand over */
    auto run_unit = [&](Unit &U, float4 (&pre)[UF][NLD], int c, const Unit &next, bool has_next, int cnext) -> bool {
        /* Waves of a SIMD are served oldest first, so the older FIR waves would race two chunks ahead of the loop and
         * then sleep while the youngest, whose chunk the loop is waiting for, crawls along alone (a lone wave pays for
         * every LDS instruction and every dependent result itself).  Priority by need instead: the fewer chunks a
         * wave is ahead of the loop, the higher its priority, so the waves of a SIMD advance together and keep its
         * issue slots full.  (The serial wave runs at priority 3.) */
        if (a.dbg & 256) {
        } else if (simd0 && !(a.dbg & 1024)) {
            __builtin_amdgcn_s_setprio(3);
        } else {
            const int lead = c - __hip_atomic_load(&sm->consumed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (lead <= 0) __builtin_amdgcn_s_setprio(2);
            else if (lead == 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        /* history (the previous chunk's last block, one block below block 0: the lanes whose pair lies before
         * the first tap's reach are skipped), then this chunk's samples */
#pragma unroll
        for (int ff = 0; ff < UF; ff++) {
            const int p0 = 2 * lane + HIST - U.ix[ff];             /* window position of sample 2*lane of the chunk */
            float2 *w0 = mywin + ff * WS + slot_of(p0), *w1 = mywin + ff * WS + slot_of(p0 + 1);
            if ((U.ix[ff] & 1) == 0) {      /* wave-uniform: every lane holds a pair of frame ff here */
                if (p0 >= 128) *reinterpret_cast<float4 *>(w0 - BLK) = U.hist[ff];
#pragma unroll
                for (int j = 0; j < NLD; j++)
                    *reinterpret_cast<float4 *>(w0 + BLK * j) = pre[ff][j];
            } else {
                if (p0 >= 128) w0[-BLK] = make_float2(U.hist[ff].x, U.hist[ff].y);
                if (p0 + 1 >= 128) w1[-BLK] = make_float2(U.hist[ff].z, U.hist[ff].w);
#pragma unroll
                for (int j = 0; j < NLD; j++) {
                    w0[BLK * j] = make_float2(pre[ff][j].x, pre[ff][j].y);
                    w1[BLK * j] = make_float2(pre[ff][j].z, pre[ff][j].w);
                }
            }
            U.hist[ff] = pre[ff][NLD - 1];
        }
        if (has_next) prefetch(next, pre, cnext);
        probe.tick(2);

        /* sliding-window FIR, the pinned two-symbol step of rx_fused_pipe_kernel: symbol r of this lane uses tap
         * k = t - C*r at window position PAD*q + t; taps 0..126 in order into one accumulator per symbol */
        v2f ac[R] = {v2f{0.0f, 0.0f}, v2f{0.0f, 0.0f}};
#if QPSK_PIPE2_ASM
        if (!QPSK_ABLATE(a, 1)) {
            /* the hand-scheduled stream (fir_r2_asm.h, generated by tools/gen_fir_asm.py): the sum below, same order */
            fir_r2_asm(lds_addr(rd), lds_addr(sm->taps), ac[0], ac[1]);
#else
        if (!QPSK_ABLATE(a, 1)) {
            /* Two symbols per lane leave a lone multiply/add pair per symbol and window position: too little
             * independent work for a wave that waits 8 cycles on every dependent result.  So positions go in PAIRS:
             * the four products of positions t, t+1 (two symbols each), then the four adds -- each accumulator still
             * receives its taps in order 0..126 (rrc_fir.c:22-26), an add follows its product by 4 instructions and
             * the previous add of its accumulator by 2.  Window values and tap groups are fetched from LDS DEPTH
             * blocks of 8 positions ahead of their use. */
            constexpr int NB = (TSTEPS + C - 1) / C, DEPTH = QPSK_PIPE2_DEPTH, NW = DEPTH + 1, NG = R + DEPTH;
            float tg[NG][C];
            float2 wv[NW][C];
            auto fetch_block = [&](int tb) {
                if (tb * C < NTAPS) {
                    const float4 ta = taps4[2 * tb], tb4 = taps4[2 * tb + 1];
                    float *g_ = tg[tb % NG];
                    g_[0] = ta.x; g_[1] = ta.y; g_[2] = ta.z; g_[3] = ta.w;
                    g_[4] = tb4.x; g_[5] = tb4.y; g_[6] = tb4.z; g_[7] = tb4.w;
                }
#pragma unroll
                for (int u = 0; u < C; u += 2) {
                    const int t = tb * C + u;      /* t even: positions t, t + 1 are one aligned 16-byte word */
                    if (t < TSTEPS) {
                        const float4 w4 = *reinterpret_cast<const float4 *>(rd + slot_of(t));
                        wv[tb % NW][u] = make_float2(w4.x, w4.y);
                        wv[tb % NW][u + 1] = make_float2(w4.z, w4.w);
                    }
                }
            };
            static_for<0, DEPTH>([&](auto d) { if (decltype(d)::value < NB) fetch_block(decltype(d)::value); });
            static_for<0, NB>([&](auto tbc) {
                constexpr int tb = decltype(tbc)::value;
                if (tb + DEPTH < NB) fetch_block(tb + DEPTH);
                static_for<0, C / 2>([&](auto uc) {
                    constexpr int u = 2 * decltype(uc)::value;
                    constexpr int t = tb * C + u;              /* positions t and t + 1 */
                    if constexpr (t < TSTEPS) {
                        constexpr bool a0 = t < NTAPS, a1 = t >= C && t - C < NTAPS;                  /* symbol 0 / 1 at t */
                        constexpr bool b0 = t + 1 < NTAPS, b1 = t + 1 >= C && t + 1 - C < NTAPS && t + 1 < TSTEPS;   /* at t + 1 */
                        const v2f va = v2f{wv[tb % NW][u].x, wv[tb % NW][u].y};
                        const v2f vb = v2f{wv[tb % NW][u + 1].x, wv[tb % NW][u + 1].y};
                        v2f pa0, pa1, pb0, pb1;    /* re*tap, im*tap (rrc_fir.c:24-25) */
                        if constexpr (a0) pa0 = va * tg[tb % NG][u];
                        if constexpr (a1) pa1 = va * tg[(tb - 1 + NG) % NG][u];
                        if constexpr (b0) pb0 = vb * tg[tb % NG][u + 1];
                        if constexpr (b1) pb1 = vb * tg[(tb - 1 + NG) % NG][u + 1];
                        if constexpr (a0 && a1 && b0 && b1) {
                            asm volatile("" : "+v"(pa0), "+v"(pa1), "+v"(pb0), "+v"(pb1));
                        } else {
                            if constexpr (a0) asm volatile("" : "+v"(pa0));
                            if constexpr (a1) asm volatile("" : "+v"(pa1));
                            if constexpr (b0) asm volatile("" : "+v"(pb0));
                            if constexpr (b1) asm volatile("" : "+v"(pb1));
                        }
                        if constexpr (a0) ac[0] = ac[0] + pa0;
                        if constexpr (a1) ac[1] = ac[1] + pa1;
                        if constexpr (b0) ac[0] = ac[0] + pb0;
                        if constexpr (b1) ac[1] = ac[1] + pb1;
                        asm volatile("" : "+v"(ac[0]), "+v"(ac[1]));
                    }
                });
            });
#endif
        } else {
            ac[0] = v2f{0.7f, 0.3f}; ac[1] = v2f{0.7f, 0.3f};
        }
        probe.tick(3);
        /* ring slot c % DR is free once chunk c - DR has been consumed, and that chunk's symbols leave first */
        const int g = UF * U.u + fl, frame = f0 + g;
        const bool mine = g < G && frame < a.nframes;     /* this lane's frame exists (rings have G rows) */
        if (c >= DR) {
            if (!wait_ge(&sm->consumed, c - DR + 1, &sm->abort_flag)) return false;
            probe.tick(0);
            /* the flush's addresses are recomputed here every time (the asm statement hides that g never changes):
             * hoisted out of the chunk loop they are spilled, and a scratch reload waits for every load issued before
             * it -- the next unit's samples, just requested (vmcnt counts in order) */
            int gf = g, qf = q;
            asm volatile("" : "+v"(gf), "+v"(qf));
            if (mine) flush_records<GM, R>(a, zring, dring, gf, f0 + gf, qf, c - DR);
            probe.tick(1);
        }
        if (g < G) {   /* the lane's two symbols are one aligned 16-byte word of the ring (rows are 16-byte aligned, R q even) */
            const float2 s0 = fir_gain(make_float2(ac[0].x, ac[0].y)), s1 = fir_gain(make_float2(ac[1].x, ac[1].y));
            int gr = g, qr = q;     /* as above: the ring address is cheaper to recompute than to reload */
            asm volatile("" : "+v"(gr), "+v"(qr));
            *reinterpret_cast<float4 *>(dring + (size_t)gr * DSTRIDE + (c % DR) * S + R * qr) = make_float4(s0.x, s0.y, s1.x, s1.y);
        }
        if (lane == 0) st_release(&sm->ready[U.u], c + 1);
        probe.tick(4);
        return true;
    };

    float4 pre[UF][NLD];
    prefetch(un[0], pre, 0);
    bool ok = true;
    probe.tick(-1);
    for (int c = 0; c < nchunks && ok; c++) {
        static_for<0, NUW>([&](auto uic) {
            constexpr int ui = decltype(uic)::value, nx = (ui + 1) % NUW;
            constexpr bool last_unit = ui + 1 == NUW;
            if (ok) ok = run_unit(un[ui], pre, c, un[nx], !last_unit || c + 1 < nchunks, last_unit ? c + 1 : c);
        });
    }
    if (ok) {
        ok = wait_ge(&sm->consumed, nchunks, &sm->abort_flag);
        if (ok)
#pragma unroll
            for (int ui = 0; ui < NUW; ui++) {
                const int g = UF * (u0 + ui) + fl, frame = f0 + g;
                for (int c = max(0, nchunks - DR); c < nchunks; c++)
                    if (g < G && frame < a.nframes) flush_records<GM, R>(a, zring, dring, g, frame, q, c);
            }
    }
    if (!ok && lane == 0) report_status(status, STATUS_PIPE_TIMEOUT);
    probe.report_fir_wave2(lane, widx, nuw, nchunks);
}

__global__ void __launch_bounds__(pipe2::MAX_THREADS)
rx_pipe2_kernel(FusedArgs a, unsigned long long layout, int nwin, int *status)
{
    using namespace pipe2;
    using GM = GeomNarrow;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem *sm = reinterpret_cast<Smem *>(smem_raw);
    const int G = a.G;                                   /* frames of a workgroup */
    float2 *win = reinterpret_cast<float2 *>(smem_raw + sizeof(Smem));      /* [nwin][UF][WS]: one window per FIR wave */
    float2 *dring = win + (size_t)nwin * UF * WS;                            /* [G][DSTRIDE] */
    float *zring = reinterpret_cast<float *>(dring + (size_t)G * GM::DSTRIDE);   /* [G*nbw][ZSTRIDE] */
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f0 = blockIdx.x * G;
    const int nchunks = (a.nsym + S - 1) / S;

    for (int i = tid; i < 128; i += blockDim.x)
        sm->taps[i] = i < NTAPS ? a.taps[i] : 0.0f;
    if (tid < MAX_WAVES) sm->ready[tid] = 0;
    if (tid == 0) { sm->consumed = 0; sm->abort_flag = 0; }
    __syncthreads();

    if (wave == 0) {
        costas_wave<GM>(a, sm, dring, zring, G, f0, lane, nchunks, status);   /* a.mixed == 2: lane g waits on ready[g / 2] */
        return;
    }
    /* layout: 4 bits per hardware wave = the units it owns (consecutive units, in wave order); 0 = the wave retires at
     * once (the host leaves the serial wave's SIMD -- waves 4, 8 -- empty unless asked otherwise) */
    const int mine = (int)((layout >> (4 * wave)) & 15);
    if (mine == 0) return;
    int u0 = 0, widx = 0;
    for (int v = 1; v < wave; v++) {
        const int cv = (int)((layout >> (4 * v)) & 15);
        u0 += cv;
        widx += cv != 0;
    }
    float2 *mywin = win + (size_t)widx * UF * WS;
    if (mine == 2)
        fir_wave2<2>(a, sm, mywin, dring, zring, G, widx, u0, f0, lane, nchunks, status);
    else
        fir_wave2<1>(a, sm, mywin, dring, zring, G, widx, u0, f0, lane, nchunks, status);
}

size_t pipe2_lds_bytes(int G, int nwin, int nbw)
{
    using GM = GeomNarrow;
    size_t b = sizeof(Smem) + sizeof(float2) * ((size_t)nwin * pipe2::UF * pipe2::WS + (size_t)G * GM::DSTRIDE) +
               sizeof(float) * (size_t)G * nbw * GM::ZSTRIDE;
    return (b + 15) & ~(size_t)15;
}

int pipe2_max_fir(void) { return pipe2::MAX_FIR; }
int pipe2_max_frames(void) { return pipe2::UF * pipe2::MAX_UNITS; }
int pipe2_max_units_per_wave(void) { return pipe2::MAX_UW; }
int pipe2_max_hw_waves(void) { return pipe2::MAX_THREADS / 64; }

/*
 * The default layout for NU units [measured, DESIGN.md 4.1].
 *   NU <= 8 (up to 16 frames per workgroup: the recurrence is the limit): one unit per wave on hardware waves 1-3,
 *     5-7, 9, 10 -- SIMDs 1-3; waves 4 and 8 would sit beside the serial wave and retire at once.
 *   NU > 8 (the filter is the limit): the serial wave leaves three quarters of its SIMD's issue slots unused, so
 *     hardware wave 4 filters too: one unit each on waves 1-7, 9, 10, then a second one on waves 1, 2, ... -- a full
 *     workgroup's 16 units sit 2, 5, 5, 4 on SIMDs 0-3 (nine windows are what the LDS holds beside 32 frames' rings).
 *     The kernel then runs the serial wave at priority 1 and the FIR wave beside it at 3 (see there).
 */
unsigned long long pipe2_default_layout(int NU)
{
    using namespace pipe2;
    int cnt[16] = {0};
    const int hwmax = MAX_THREADS / 64;
    const bool share = NU > 8 && MAX_UW == 2;
    int left = NU;
    for (int round = 0; round < MAX_UW && left > 0; round++)
        for (int w = 1; w < hwmax && left > 0; w++) {
            if ((w & 3) == 0 && !(share && w == 4)) continue;
            if (share && (w == 11 || (round == 1 && w > 7))) continue;
            cnt[w]++;
            left--;
        }
    unsigned long long layout = 0;
    for (int w = 1; w < hwmax; w++) layout |= (unsigned long long)cnt[w] << (4 * w);
    return left == 0 ? layout : 0;
}

/* G frames per workgroup (at most 32, G * nbw <= 64); layout as in the kernel: its counts must add up to the units */
int launch_rx_pipe2(const FusedArgs &a0, int G, unsigned long long layout, int *status, hipStream_t s)
{
    using namespace pipe2;
    if (a0.est_tw) return (int)hipErrorInvalidValue;   /* no in-launch timing estimate in this kernel: it would use fixed_index */
    FusedArgs a = a0;
    const int NU = (G + UF - 1) / UF;
    const LayoutCount n = layout_count(layout, MAX_UW);
    if (!n.valid || G < 1 || G > UF * MAX_UNITS || G * a.nbw > 64 || n.units != NU ||
        pipe2_lds_bytes(G, n.nwin, a.nbw) > (size_t)MAX_LDS_BYTES)
        return (int)hipErrorInvalidValue;
    a.G = G;
    a.lean_pair = 0;                                      /* one lane per loop: the paired stream is rx_lean_kernel's */
    a.mixed = 2;                                          /* the serial wave's lane for frame g waits on ready[g / 2] */
    a.share_simd0 = n.share_simd0;                        /* hardware waves 4, 8 */
    const int blocks = (a.nframes + G - 1) / G;
    hipLaunchKernelGGL(rx_pipe2_kernel, dim3(blocks), dim3(64 * n.hw), pipe2_lds_bytes(G, n.nwin, a.nbw), s, a, layout, n.nwin, status);
    return (int)hipGetLastError();
}

int prepare_rx_pipe2(void)
{
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(rx_pipe2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS_BYTES);
}

} // namespace qpsk
