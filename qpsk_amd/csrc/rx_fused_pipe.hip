/*
 * rx_fused_pipe.hip -- the receive pipeline (rx_pipe.h) in its first layout, 16 frames per workgroup with per-frame windows:
 * rx_fused_pipe_kernel (FIR waves of four frames x four symbols per lane or two x two, the FFT timing estimate inside the launch) and
 * costas_pipe_kernel (the same rings fed with already decimated symbols); their launch geometry and launchers; prepare_pipe_kernel.
 */
#include "rx_pipe.h"
#include "fir_r2_asm.h"        /* rx_fused_pipe_kernel's FIR waves with two symbols per lane */
#include "fir_r4_asm.h"        /* ... with four */
#include "fir_full8_asm.h"     /* the in-launch FFT timing estimate of rx_fused_pipe_kernel */
#include "timing_fft_wave.h"
#include "carrier.h"           /* costas_pipe_kernel's spare wave */

#ifndef QPSK_PIPE1_ASM
#define QPSK_PIPE1_ASM 1     /* rx_fused_pipe_kernel: FIR steps as the generated streams; 0: the compiler's pinned step (A/B builds) */
#endif
namespace qpsk {

static_assert(FIR_R4_ASM_END_VGPR <= 256, "rx_fused_pipe_kernel: two waves per SIMD");

/* ========================================================================
 * costas_pipe_kernel: the same pipeline with ALREADY DECIMATED symbols as
 * input (qpsk.c:196-212 alone: qpsk_costas_batch, and the streaming mode,
 * where decimated_frame[] carries the previous block, qpsk.c:186-197).
 * Waves 1..NF only move data: 64 symbols per frame per chunk from global
 * memory into the symbol ring, and the flush of consumed records.
 * a.dsrc rows are a.dstride symbols apart; one loop per frame (nbw = 1).
 * ======================================================================== */
__global__ void __launch_bounds__(64 * (GeomNarrow::MAX_NF + 2))
costas_pipe_kernel(FusedArgs a, int *status)
{
    using GM = GeomNarrow;
    QPSK_GEOM_CONSTANTS(GM);
    static_assert(R == 2 || R == 4, "flush_records packs 2 or 4 symbols per store");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem *sm = reinterpret_cast<Smem *>(smem_raw);
    const int NF = (int)blockDim.x / 64 - 1 - (a.carrier_state ? 1 : 0);
    const int G = NF * FWV;
    float2 *dring = reinterpret_cast<float2 *>(smem_raw + sizeof(Smem));     /* [G][DSTRIDE] */
    float *zring = reinterpret_cast<float *>(dring + (size_t)G * DSTRIDE);  /* [G][ZSTRIDE] */
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int N = a.nsym;
    const int f0 = blockIdx.x * G;
    const int nchunks = (N + S - 1) / S;
    if (tid < MAX_WAVES) sm->ready[tid] = 0;
    if (tid == 0) { sm->consumed = 0; sm->abort_flag = 0; }
    __syncthreads();

    if (wave == 0) {
        costas_wave<GM>(a, sm, dring, zring, G, f0, lane, nchunks, status);
        return;
    }
    if (wave == NF + 1) {      /* the spare wave (streams behind stream_scan_kernel MODE 2): the rest of the next block's carrier table */
        if (blockIdx.x == 0 && lane == 0)
            carrier_block(a.carrier_state, a.carrier_tab, a.carrier_frame, carrier_split(a.carrier_frame), a.carrier_frame / 2);
        return;
    }
    const int w = wave - 1;
    const int fl = lane / QL, q = lane % QL;
    const int g = w * FWV + fl;
    const int frame = f0 + g;
    const bool fvalid = frame < a.nframes;
    const float2 *src = a.dsrc + (size_t)(fvalid ? frame : 0) * a.dstride;
    int flushed = 0;
    bool ok = true;
    float2 pre[R];
    auto fetch = [&](int c) {
#pragma unroll
        for (int r = 0; r < R; r++)
            pre[r] = src[min(c * S + R * q + r, N - 1)];     /* clamped: symbols past N are never consumed */
    };
    fetch(0);
    for (int c = 0; c < nchunks; c++) {
        if (c >= DR) {
            ok = wait_ge(&sm->consumed, c - DR + 1, &sm->abort_flag);
            if (!ok) break;
            for (; flushed < c - DR + 1; flushed++)
                if (fvalid) flush_records<GM>(a, zring, dring, g, frame, q, flushed);
        }
        float2 *dw = dring + (size_t)g * DSTRIDE + (c % DR) * S + R * q;
#pragma unroll
        for (int r = 0; r < R; r++)
            dw[r] = pre[r];
        if (c + 1 < nchunks) fetch(c + 1);
        if (lane == 0) st_release(&sm->ready[w], c + 1);
        if (a.refill && fvalid) {
            /* decimated_frame[i] <- input_frame[i*CYCLES + index] of the block just filtered (qpsk.c:186-191):
             * the slots this lane has just emptied, off the hand-over path */
            const float2 *blk = a.refill + (size_t)frame * a.frame_size;
            float2 *row = a.refill_dst + (size_t)frame * a.dstride;
            const int ix = checked_index(a.index ? a.index[frame] : a.fixed_index, a.status);
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int i = c * S + R * q + r, s = i * a.cycles + ix;
                if (i < N) {
                    if (a.refill_planar) {      /* the block planar by decimation phase (streamscan.hip): [cycles][symbols]; an index of
                                                  * CYCLES or more (the histogram has 8 bins whatever CYCLES is) reaches into the next symbol */
                        const int pl = ix % a.cycles, sy = i + ix / a.cycles;
                        row[i] = sy < N ? blk[(size_t)pl * N + sy] : make_float2(0.0f, 0.0f);
                    } else {
                        row[i] = s < a.frame_size ? blk[s] : make_float2(0.0f, 0.0f);
                    }
                }
            }
        }
    }
    if (ok) {
        ok = wait_ge(&sm->consumed, nchunks, &sm->abort_flag);
        if (ok)
            for (; flushed < nchunks; flushed++)
                if (fvalid) flush_records<GM>(a, zring, dring, g, frame, q, flushed);
    }
    if (!ok && lane == 0) report_status(status, STATUS_PIPE_TIMEOUT);
}

template <class GM>
__global__ void __launch_bounds__(GM::MAX_THREADS)
rx_fused_pipe_kernel(FusedArgs a, int *status)
{
    QPSK_GEOM_CONSTANTS(GM);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem *sm = reinterpret_cast<Smem *>(smem_raw);
    /* Waves are dealt to the SIMDs round-robin, so waves 4, 8, ... land beside the serial wave 0.  With spare
     * waves the host launches those too and they retire at once: the serial wave keeps SIMD 0 to itself and the
     * FIR waves are hardware waves 1,2,3, 5,6,7, 9,10 (QPSK_PIPE_DBG bit 2 turns the spares off). */
    const bool spares = GM::SPARE && !(a.dbg & 4);
    const int nwaves = (int)blockDim.x / 64;
    const bool mixed = a.mixed != 0;                                        /* 16 frames, two lane mappings (see the FIR waves) */
    const int nfir = spares ? (nwaves - 1) - (nwaves - 1) / 4 : nwaves - 1;   /* FIR waves unless mixed */
    const int G = a.mixed == 1 ? 4 * FWV : a.mixed == 2 ? 2 * nfir : nfir * FWV;   /* frames of the workgroup */
    float2 *win = reinterpret_cast<float2 *>(smem_raw + sizeof(Smem));   /* [G][WSLOTS] */
    float2 *dring = win + (size_t)G * WSLOTS;                              /* [G][DSTRIDE] */
    float *zring = reinterpret_cast<float *>(dring + (size_t)G * DSTRIDE);   /* [G*nbw][ZSTRIDE] records: the phase each
                                                                               symbol's step started from, see flush_records */

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   /* scalar: per-wave frame pointers stay in SGPRs */
    const int L = a.frame_size, N = a.nsym;
    const int f0 = blockIdx.x * G;
    const int nchunks = (N + S - 1) / S;

    /* ---- common prologue: taps, counters, zeroed windows (= fresh delay lines, qpsk.c:37) */
    for (int i = tid; i < 128; i += blockDim.x)
        sm->taps[i] = i < NTAPS ? a.taps[i] : 0.0f;
    if (tid < MAX_WAVES) sm->ready[tid] = 0;
    if (tid == 0) { sm->consumed = 0; sm->abort_flag = 0; }
    __syncthreads();      /* (no window to zero: a fresh delay line is a zero history in the FIR waves' registers) */

    /* ---- BASELINE config 3: the FFT timing estimate inside the launch (timing_fft_wave.h; the host sets a.est_tw only for full
     * 16-frame workgroups = 8 hardware waves).  Every hardware wave -- the serial wave and the two that retire included, all idle
     * until the first chunk exists -- estimates frames 2 wave, 2 wave + 1 of the workgroup: 4 frames per SIMD, the full-rate
     * stream fir_full8_asm.h on 512 samples each, its window in the (not yet used) frame windows' LDS.  No launch of its own, no
     * drain and refill of the chip between the estimate and the pipeline; the indices never leave the CU. */
    if (a.est_tw) {
        float2 *ewin = win + (size_t)wave * tfft::WSLOTS;
        const unsigned erd = lds_addr(ewin + (tfft::R + tfft::PADS) * lane), etap = lds_addr(sm->taps);
        const int fe0 = f0 + 2 * wave;
        /* both frames unconditionally (a frame past the batch's end re-reads the last one and its result is dropped): the samples
         * stay in registers, the second frame's are in flight while the first is filtered */
        const float2 *srcA = a.x + (size_t)min(fe0, a.nframes - 1) * a.frame_pitch;
        const float2 *srcB = a.x + (size_t)min(fe0 + 1, a.nframes - 1) * a.frame_pitch;
        tfft::Pre5 pre = tfft::load_frame5(srcA, lane);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            tfft::stage_frame5(ewin, lane, pre);
            if (i == 0) pre = tfft::load_frame5(srcB, lane);
            tfft::wave_sync();
            v2f e0, e1, e2, e3, e4, e5, e6, e7;
            fir_full8_asm(erd, etap, e0, e1, e2, e3, e4, e5, e6, e7);
            const v2f eacc[tfft::R] = {e0, e1, e2, e3, e4, e5, e6, e7};
            double epv[tfft::R];
            const tfft::cd u = tfft::power_bin(eacc, ewin, lane, a.est_tw, tfft::NFFT / C, nullptr, epv);
            if (lane == 0 && fe0 + i < a.nframes) {
                const int best = tfft::pick_index(u, a.est_cs, C, nullptr);
                sm->est_index[2 * wave + i] = best;
                if (a.index_out) a.index_out[fe0 + i] = best;
            }
        }
        __syncthreads();
    }

    if (wave == 0) {
        costas_wave<GM>(a, sm, dring, zring, G, f0, lane, nchunks, status);
        return;
    }

    /* ======================================= FIR waves =========================================== */
    /* Which frames a hardware wave filters, and with which lane mapping.
     *   plain: FIR wave w owns the 4 frames of group w (with spares, hardware waves 4, 8 retire at once).
     *   mixed (measurement variant of the full narrow workgroup, QPSK_PIPE_DBG bit 7): four 4-frame units on
     *     three SIMDs leave one SIMD with two, so 12 frames go to hardware waves 1-3 in the 4-symbol mapping (one
     *     per SIMD) and the last 4 to hardware waves 6 and 7 (SIMDs 2 and 3), two frames each in the 2-symbol
     *     mapping (32 lanes per frame): 1, 1.5 and 1.5 units per SIMD instead of 2, 1, 1.  Every wave still owns
     *     its frames outright.  Bit-exact like the plain layout, and no faster (see the launcher). */
    int w, gbase, rslot;          /* FIR wave index, first frame slot, its ready[] counter */
    bool half = false;
    if (a.mixed == 2) {   /* several loops per frame: every FIR wave takes two frames, 2 symbols per lane (the flush
                             does sin/cos once per loop and symbol, so the frames are spread over more waves) */
        if (spares && (wave & 3) == 0) return;
        w = spares ? wave - 1 - wave / 4 : wave - 1;
        half = true;
        gbase = 2 * w;
        rslot = w;
    } else if (mixed) {
        if (wave >= 4 && wave <= 5) return;
        half = wave >= 6;
        w = half ? wave - 3 : wave - 1;
        gbase = half ? 12 + 2 * (wave - 6) : 4 * (wave - 1);
        rslot = w;
    } else {
        if (spares && (wave & 3) == 0) return;   /* a wave that would share a SIMD with wave 0 */
        w = spares ? wave - 1 - wave / 4 : wave - 1;   /* FIR wave index = the frame group it owns */
        gbase = w * GM::FWV;
        rslot = w;
    }

  auto fir_wave = [&](auto wmap) {
    /* this wave's lane mapping: QL lanes per frame, R symbols per lane (QL * R = S for every wave of the workgroup) */
    /* window image: position p at slot p + PADS (p / PAD), PADS = 2 -- lanes are 16-byte multiples apart (272 bytes for
     * four symbols per lane, 144 for two), so positions (t, t+1), t even, are one aligned 16-byte word, which is what
     * the hand-scheduled filter streams read (fir_r4_asm.h, fir_r2_asm.h: one ds_read_b128 per two positions) */
    constexpr int PADS = 2;
    constexpr int QL = decltype(wmap)::QL, R = decltype(wmap)::R, FWV = 64 / QL, PAD = R * C,
                  TSTEPS = NTAPS + C * (R - 1);
    static_assert(QL * R == S && 128 % PAD == 0 && PAD >= 2 * C, "chunk size and window padding are the workgroup's");
    const int fl = lane / QL, q = lane % QL;

    /* taps stay in LDS; the FIR loop keeps a rolling set of R + 1 groups of C taps in registers (broadcast reads) */
    const float4 *taps4 = reinterpret_cast<const float4 *>(sm->taps);
    constexpr int NLD = CH / 128;                          /* 16-byte loads per frame per chunk */

    /* what a wave needs to know about its frames: one 16-byte load covers 128 samples of ONE frame, so the
     * wave's 64 lanes sweep a frame in NLD loads; lane `lane` holds samples 2*lane, 2*lane+1 of each 128-block */
    struct Ctx {
        int group, g, frame;       /* ready[] slot, this lane's frame slot in the workgroup, its frame */
        bool fvalid, all_valid;
        float2 *wf;                /* this lane's frame window */
        const float2 *rd;          /* FIR read base: position PAD*q -> slot (PAD+1)*q */
        int wr0[FWV], wr1[FWV];    /* window write slots of the loaded pair, per frame of the wave */
        bool even[FWV];            /* the frame's decimation offset is even: the pair is one aligned 16-byte word */
        bool h0[FWV], h1[FWV];     /* per lane: the pair's first / second sample of the LAST block of a chunk is history of the next */
        float4 hist[FWV];          /* per lane: the pair it loaded from the last block of the previous chunk */
        const float4 *src[FWV];
        bool fv[FWV];
    };
    auto make_ctx = [&]() {
        Ctx cx;
        cx.group = rslot;
        cx.g = gbase + fl;
        cx.frame = f0 + cx.g;
        cx.fvalid = cx.frame < a.nframes;
        cx.all_valid = f0 + gbase + FWV <= a.nframes;
        cx.wf = win + (size_t)cx.g * WSLOTS;
        cx.rd = cx.wf + (PAD + PADS) * q;
#pragma unroll
        for (int ff = 0; ff < FWV; ff++) {
            const int fr = f0 + gbase + ff;
            cx.fv[ff] = fr < a.nframes;
            const int ix = a.est_tw ? (cx.fv[ff] ? sm->est_index[gbase + ff] : 0)
                                    : checked_index(a.index ? (cx.fv[ff] ? a.index[fr] : 0) : a.fixed_index, a.status);   /* decimation offset, < C */
            const int p0 = 2 * lane + 126 - ix;               /* window position of sample 2*lane of the chunk */
            cx.wr0[ff] = (gbase + ff) * WSLOTS + p0 + PADS * (p0 / PAD);
            cx.wr1[ff] = (gbase + ff) * WSLOTS + (p0 + 1) + PADS * ((p0 + 1) / PAD);
            cx.even[ff] = (ix & 1) == 0;
            cx.h0[ff] = p0 >= 128;                            /* position p0 - 128 of the next chunk's window exists */
            cx.h1[ff] = p0 + 1 >= 128;
            cx.hist[ff] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   /* a fresh delay line (qpsk.c:37) */
            cx.src[ff] = reinterpret_cast<const float4 *>(a.x + (size_t)(cx.fv[ff] ? fr : 0) * a.frame_pitch);
        }
        return cx;
    };

    /* L is even on this path (checked by the host), so a 16-byte pair is either inside the frame or past it.
     * Loads are UNCONDITIONAL (a per-load branch would make the compiler wait for each load in turn): a
     * chunk that lies inside every frame of the group -- all but the last one -- loads straight; the tail
     * chunk clamps the address into the frame and zeroes what lies past the end afterwards. */
    auto prefetch = [&](const Ctx &cx, float4 (&pre)[FWV][NLD], int c) {
        if (cx.all_valid && (c + 1) * CH <= L) {
#pragma unroll
            for (int ff = 0; ff < FWV; ff++)
#pragma unroll
                for (int j = 0; j < NLD; j++)
                    pre[ff][j] = load_once(&cx.src[ff][(c * CH + 128 * j + 2 * lane) >> 1]);
        } else {
#pragma unroll
            for (int ff = 0; ff < FWV; ff++) {
#pragma unroll
                for (int j = 0; j < NLD; j++) {
                    const int s = c * CH + 128 * j + 2 * lane;      /* first sample of the pair */
                    const bool in = cx.fv[ff] && s + 1 < L;
                    float4 v = load_once(&cx.src[ff][in ? (s >> 1) : 0]);
                    if (!in) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    pre[ff][j] = v;
                }
            }
        }
    };

    /* measurement build only (make -C qpsk_amd/csrc profile, then QPSK_PIPE_DBG bit 5): where a FIR wave of
     * workgroup 0 spends its shader cycles (rx_profile.h).  The product library carries neither the counters nor the printf. */
    prof::FirProbe probe(a);

    /* Every wave turns its own frames' records into symbols: the flush needs the symbols themselves, and they
     * stay in the ring only until their owner refills the slot -- which it does right after this flush.  (With the
     * (T, quadrant) records of the earlier design any wave could flush for any other, and the waves with slack did;
     * the phase records take 8 bytes per step off the serial wave's LDS writes instead.) */
    const int fbase[1] = {gbase};
    const int nflush = 1;
    auto flush_chunk = [&](int chunk) {
        for (int i = 0; i < nflush; i++) {
            const int g2 = fbase[i] + fl, fr2 = f0 + g2;
            if (fr2 < a.nframes) flush_records<GM, R>(a, zring, dring, g2, fr2, q, chunk);
        }
    };

    /* one chunk of one frame group: flush what the loop has finished with, stage the window, filter, hand over */
    auto run_chunk = [&](Ctx &cx, float4 (&pre)[FWV][NLD], int c, bool prefetch_next) -> bool {
        /* The window is rebuilt from REGISTERS every chunk: the 126 samples of history a frame carries are the tail
         * of the last 128-sample block its wave loaded for the previous chunk (4 VGPRs per frame), written one block
         * below block 0; then the prefetched samples of this chunk.  No copy through LDS, nothing to zero.  An even
         * decimation offset makes a lane's pair one aligned 16-byte word of the image. */
        constexpr int BLK = 128 + PADS * (128 / PAD);
#pragma unroll
        for (int ff = 0; ff < FWV; ff++) {
            if (cx.even[ff]) {      /* wave-uniform: every lane holds a pair of frame ff here */
                if (cx.h0[ff]) *reinterpret_cast<float4 *>(win + cx.wr0[ff] - BLK) = cx.hist[ff];
#pragma unroll
                for (int j = 0; j < NLD; j++)
                    *reinterpret_cast<float4 *>(win + cx.wr0[ff] + BLK * j) = pre[ff][j];
            } else {
                if (cx.h0[ff]) win[cx.wr0[ff] - BLK] = make_float2(cx.hist[ff].x, cx.hist[ff].y);
                if (cx.h1[ff]) win[cx.wr1[ff] - BLK] = make_float2(cx.hist[ff].z, cx.hist[ff].w);
#pragma unroll
                for (int j = 0; j < NLD; j++) {
                    win[cx.wr0[ff] + BLK * j] = make_float2(pre[ff][j].x, pre[ff][j].y);
                    win[cx.wr1[ff] + BLK * j] = make_float2(pre[ff][j].z, pre[ff][j].w);
                }
            }
            cx.hist[ff] = pre[ff][NLD - 1];
        }
        if (prefetch_next) prefetch(cx, pre, c + 1);
        probe.tick(2);

        /* sliding-window FIR: symbol r of this lane uses tap k = t - C*r at window position PAD*q + t */
        const float2 *rd = cx.rd;
        float2 acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = QPSK_ABLATE(a, 1) ? make_float2(0.7f, 0.3f) : make_float2(0.0f, 0.0f);
        /* t = C*tb + u: symbol r needs tap group tb - r (taps C*(tb-r) .. +C-1), so each group of C taps is
         * live for R consecutive blocks */
        static_assert(C == 8 && (R == 4 || R == 2), "the step below is written for C = 8 and R = 2 or 4");
        if constexpr (!GM::PINNED) {
            /* the compiler's own schedule of the same sum (a Geom with PINNED = false; no longer instantiated):
             * config 2 ran 0.2148 ms with it against 0.2088 ms with the pinned order below [measured, same process] */
            if (!QPSK_ABLATE(a, 1)) {
                float tgc[R][C];
#pragma unroll
                for (int tb = 0; tb * C < TSTEPS; tb++) {
                    if (tb * C < NTAPS) {
                        const float4 ta = taps4[2 * tb], tb4 = taps4[2 * tb + 1];
                        tgc[tb % R][0] = ta.x; tgc[tb % R][1] = ta.y; tgc[tb % R][2] = ta.z; tgc[tb % R][3] = ta.w;
                        tgc[tb % R][4] = tb4.x; tgc[tb % R][5] = tb4.y; tgc[tb % R][6] = tb4.z; tgc[tb % R][7] = tb4.w;
                    }
#pragma unroll
                    for (int u = 0; u < C; u++) {
                        const int t = tb * C + u;
                        if (t < TSTEPS) {
                            const float2 v = rd[t + PADS * (t / PAD)];
#pragma unroll
                            for (int r = 0; r < R; r++) {
                                const int k = t - C * r;
                                if (k >= 0 && k < NTAPS) fir_mac(acc[r], v, tgc[(tb - r + R) % R][u]);
                            }
                        }
                    }
                }
            }
        } else if (QPSK_PIPE1_ASM && !QPSK_ABLATE(a, 1)) {
            /* the hand-scheduled streams (generated, tools/gen_fir_asm.py): the sum of the step below, same order */
            if constexpr (R == 2) {
                v2f a0, a1;
                fir_r2_asm(lds_addr(rd), lds_addr(sm->taps), a0, a1);
                acc[0] = make_float2(a0.x, a0.y);
                acc[1] = make_float2(a1.x, a1.y);
            } else {
                v2f a0, a1, a2, a3;
                fir_r4_asm(lds_addr(rd), lds_addr(sm->taps), a0, a1, a2, a3);
                acc[0] = make_float2(a0.x, a0.y); acc[1] = make_float2(a1.x, a1.y);
                acc[R > 2 ? 2 : 0] = make_float2(a2.x, a2.y); acc[R > 2 ? 3 : 1] = make_float2(a3.x, a3.y);
            }
        } else if (!QPSK_ABLATE(a, 1)) { /* measurement build only: skip the filter arithmetic, keep the traffic */
            /* Software pipeline, one block of C window positions deep: the LDS reads of block tb+1 (window values
             * and tap group) are issued before the multiply-adds of block tb.  Groups rotate through R + 1 slots so
             * that the group fetched a block early does not overwrite the one symbol R-1 still needs.
             * Instruction order inside a step is pinned with empty asm statements (they keep their program order
             * and every value they name must exist where they stand): the R products of a step, then the R
             * adds.  A product is then R instructions ahead of its add and an accumulator's adds are 2R apart,
             * more than the ~8 cycles a dependent packed op waits. */
            constexpr int NB = (TSTEPS + C - 1) / C;
            float tg[R + 1][C];
            float2 wv[2][C];
            auto fetch_block = [&](int tb) {
                if (tb * C < NTAPS) {
                    /* (taps through the scalar cache into SGPRs instead -- s_load_dwordx8 from the constant address
                     * space, SGPR operands in the packed multiplies, 43 VGPRs fewer -- measured: 8192 frames
                     * 0.3456 against 0.3514 ms, 4096 frames 0.1951 against 0.1881 ms: the scalar loads share
                     * lgkmcnt with the window reads.  Not kept.) */
                    const float4 ta = taps4[2 * tb], tb4 = taps4[2 * tb + 1];
                    float *g_ = tg[tb % (R + 1)];
                    g_[0] = ta.x; g_[1] = ta.y; g_[2] = ta.z; g_[3] = ta.w;
                    g_[4] = tb4.x; g_[5] = tb4.y; g_[6] = tb4.z; g_[7] = tb4.w;
                }
#pragma unroll
                for (int u = 0; u < C; u++) {
                    const int t = tb * C + u;
                    if (t < TSTEPS) wv[tb & 1][u] = rd[t + PADS * (t / PAD)];
                }
            };
            v2f ac[R];
#pragma unroll
            for (int r = 0; r < R; r++) ac[r] = v2f{acc[r].x, acc[r].y};
            fetch_block(0);
            /* static_for: the compiler does not unroll a loop with an asm statement in it */
            static_for<0, NB>([&](auto tbc) {
                constexpr int tb = decltype(tbc)::value;
                if (tb + 1 < NB) fetch_block(tb + 1);
                static_for<0, C>([&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    constexpr int t = tb * C + u;
                    if constexpr (t < TSTEPS) {
                        const v2f v = v2f{wv[tb & 1][u].x, wv[tb & 1][u].y};
                        constexpr bool ok0 = t < NTAPS, ok1 = t >= C && t - C < NTAPS,
                                       ok2 = R > 2 && t >= 2 * C && t - 2 * C < NTAPS,
                                       ok3 = R > 2 && t >= 3 * C && t - 3 * C < NTAPS;
                        v2f p0, p1, p2, p3;    /* re*tap, im*tap (rrc_fir.c:24-25) */
                        if constexpr (ok0) p0 = v * tg[(tb + (R + 1)) % (R + 1)][u];
                        if constexpr (ok1) p1 = v * tg[(tb - 1 + (R + 1)) % (R + 1)][u];
                        if constexpr (ok2) p2 = v * tg[(tb - 2 + (R + 1)) % (R + 1)][u];
                        if constexpr (ok3) p3 = v * tg[(tb - 3 + (R + 1)) % (R + 1)][u];
                        if constexpr (ok0 && ok1 && ok2 && ok3) {
                            asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
                        } else if constexpr (R == 2 && ok0 && ok1) {
                            asm volatile("" : "+v"(p0), "+v"(p1));
                        } else {
                            if constexpr (ok0) asm volatile("" : "+v"(p0));
                            if constexpr (ok1) asm volatile("" : "+v"(p1));
                            if constexpr (ok2) asm volatile("" : "+v"(p2));
                            if constexpr (ok3) asm volatile("" : "+v"(p3));
                        }
                        if constexpr (ok0) ac[0] = ac[0] + p0;
                        if constexpr (ok1) ac[1] = ac[1] + p1;
                        if constexpr (ok2) ac[2] = ac[2] + p2;
                        if constexpr (ok3) ac[3] = ac[3] + p3;
                        if constexpr (R == 4) asm volatile("" : "+v"(ac[0]), "+v"(ac[1]), "+v"(ac[2]), "+v"(ac[3]));
                        else asm volatile("" : "+v"(ac[0]), "+v"(ac[1]));
                    }
                });
            });
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = make_float2(ac[r].x, ac[r].y);
        }
        probe.tick(3);
        /* Only now does the wave need the loop: ring slot c % DR is free once chunk c - DR has been consumed, and
         * that chunk's outputs leave first (staging and filtering above touch neither ring, so the FIR waves run
         * up to two chunks ahead of the loop instead of one) */
        if (c >= DR) {
            if (!wait_ge(&sm->consumed, c - DR + 1, &sm->abort_flag)) return false;
            probe.tick(0);
            flush_chunk(c - DR);
            probe.tick(1);
        }
        /* decimated symbols -> ring; a pick at or past the end of the block is 0 (cannot happen for idx < C) */
        float2 *dw = dring + (size_t)cx.g * DSTRIDE + (c % DR) * S + R * q;
#pragma unroll
        for (int r = 0; r < R; r++)
            dw[r] = fir_gain(acc[r]);
        if (lane == 0) st_release(&sm->ready[cx.group], c + 1);
        probe.tick(4);
        return true;
    };

    Ctx own = make_ctx();
    float4 pre[FWV][NLD];
    prefetch(own, pre, 0);
    bool ok = true;
    probe.tick(-1);
    for (int c = 0; c < nchunks && ok; c++) {
        /* mixed layout: SIMDs 2 and 3 each carry a four-frame wave and a (younger) two-frame wave, and a SIMD serves
         * its oldest wave first -- the two-frame waves were the ones with no slack.  The wave that is behind its SIMD
         * partner goes first, chunk by chunk (as in timing_scan_kernel): 1-2 % at config 2 (0.1707 against 0.1741 ms and
         * 0.1745 against 0.1757 ms in two same-process runs; QPSK_PIPE_DBG bit 64 = without). */
        if (a.mixed == 1 && w >= 1 && !(a.dbg & 64)) {
            const int pt = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&sm->ready[w <= 2 ? w + 2 : w - 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
            if (pt > c) __builtin_amdgcn_s_setprio(2);
            else if (pt < c) __builtin_amdgcn_s_setprio(0);
            else __builtin_amdgcn_s_setprio(1);
        }
        ok = run_chunk(own, pre, c, c + 1 < nchunks);
    }
    if (ok) {
        ok = wait_ge(&sm->consumed, nchunks, &sm->abort_flag);
        if (ok)
            for (int c = max(0, nchunks - DR); c < nchunks; c++) flush_chunk(c);
    }
    if (!ok && lane == 0) report_status(status, STATUS_PIPE_TIMEOUT);
    probe.report_fir_wave(lane, w, R, nchunks);
  };   /* fir_wave */

    if constexpr (GM::R == 4) {   /* the mixed workgroup exists for 64-symbol chunks only */
        if (half) {
            fir_wave(WaveMap<GM::S / 2, 2>{});
            return;
        }
    }
    fir_wave(WaveMap<GM::QL, GM::R>{});
}

/* frames of a workgroup with NF FIR waves */
template <class GM>
static int frames_of(int NF)
{
    return NF * GM::FWV;
}

template <class GM>
static size_t lds_bytes_of(int NF, int nbw)
{
    const size_t G = (size_t)frames_of<GM>(NF);
    size_t b = sizeof(Smem) + sizeof(float2) * (G * GM::WSLOTS + G * GM::DSTRIDE) + sizeof(float) * G * nbw * GM::ZSTRIDE;
    return (b + 15) & ~(size_t)15;
}

size_t pipe_lds_bytes(int NF, int nbw)
{
    return lds_bytes_of<GeomNarrow>(NF, nbw);
}

int pipe_frames(int NF) { return frames_of<GeomNarrow>(NF); }
int pipe_cycles(void) { return C; }
int pipe_max_nf(void) { return GeomNarrow::MAX_NF; }

int launch_rx_fused_pipe(const FusedArgs &a0, int NF, int *status, hipStream_t s)
{
    FusedArgs a = a0;
    a.lean_pair = 0;
    /* the full narrow workgroup runs with two lane mappings (see the kernel): no SIMD carries two four-frame
     * units, every FIR wave has slack and the kernel follows the loop.  QPSK_PIPE_DBG bit 7 = the plain layout
     * (4 FIR waves + 1 spare) for A/B runs */
    a.mixed = NF == GeomNarrow::MAX_NF && !(a.dbg & (128 | 4));
    /* several loops per frame (bandwidth sweeps): the flush costs a sin/cos per loop and symbol, so the frames go
     * two to a FIR wave (2 symbols per lane) instead of four */
    if (!a.mixed && a.nbw > 1 && NF <= 3 && !(a.dbg & (128 | 4))) a.mixed = 2;
    const int G = pipe_frames(NF);
    const int blocks = (a.nframes + G - 1) / G;
    const size_t lds = pipe_lds_bytes(NF, a.nbw);
    if (NF < 1 || NF > pipe_max_nf() || lds > (size_t)MAX_LDS_BYTES || G * a.nbw > 64) return (int)hipErrorInvalidValue;
    /* the in-launch FFT timing estimate is written for the full workgroup: 8 hardware waves x 2 frames, windows in the frame windows' LDS */
    if (a.est_tw && (a.mixed != 1 || !a.est_cs || a.frame_size < tfft::N0 + tfft::NFFT || a.index ||
                     (size_t)8 * tfft::WSLOTS > (size_t)G * GeomNarrow::WSLOTS))
        return (int)hipErrorInvalidValue;
    /* hardware waves of a workgroup with NF FIR waves: with spares, FIR wave k is hardware wave k + 1 + k/3 */
    const int nfir = a.mixed == 2 ? 2 * NF : NF;
    auto nwaves = [&](int spare) { return (spare && !(a.dbg & 4)) ? nfir + 1 + (nfir - 1) / 3 : nfir + 1; };
    /* mixed: hardware waves 0 (loop), 1-3 (4 frames each), 4-5 (retire), 6-7 (2 frames each) */
    const dim3 threads(a.mixed == 1 ? 512 : 64 * nwaves(GeomNarrow::SPARE));
    hipLaunchKernelGGL(rx_fused_pipe_kernel<GeomNarrow>, dim3(blocks), threads, lds, s, a, status);
    hipError_t e = hipGetLastError();
    return (int)e;
}

int launch_costas_pipe(const FusedArgs &a0, int NF, int *status, hipStream_t s)
{
    using GM = GeomNarrow;
    FusedArgs a = a0;
    a.lean_pair = 0;
    const int G = NF * GM::FWV;
    const int blocks = (a.nframes + G - 1) / G;
    const size_t lds = sizeof(Smem) + sizeof(float2) * (size_t)G * GM::DSTRIDE + sizeof(float) * (size_t)G * GM::ZSTRIDE;
    hipLaunchKernelGGL(costas_pipe_kernel, dim3(blocks), dim3(64 * (NF + 1 + (a.carrier_state ? 1 : 0))), lds, s, a, status);
    return (int)hipGetLastError();
}

/* every pipeline kernel may use the whole LDS; the first error wins.  This unit has two entries because the order of the calls is kept:
 * costas_pipe_kernel second, rx_fused_pipe_kernel last */
int prepare_costas_pipe(void)
{
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(costas_pipe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    MAX_LDS_BYTES);
}

int prepare_rx_fused_pipe(void)
{
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(rx_fused_pipe_kernel<GeomNarrow>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS_BYTES);
}

int prepare_pipe_kernel(void)
{
    int (*const steps[])(void) = {prepare_rx_hist, prepare_costas_pipe, prepare_rx_pipe2, prepare_rx_lean, prepare_rx_fused_pipe};
    for (auto step : steps) {
        const int e = step();
        if (e != (int)hipSuccess) return e;
    }
    return (int)hipSuccess;
}

} // namespace qpsk
