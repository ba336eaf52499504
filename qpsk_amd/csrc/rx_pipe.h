/*
 * rx_pipe.h -- what the receive pipeline kernels share (rx_fused_pipe.hip, rx_pipe2.hip, rx_lean.hip, rx_hist.hip): the
 * workgroup's geometry and LDS control block, the serial Costas wave (costas_wave) and the record flush (flush_records).
 *
 * The hot path: decimating RRC FIR + Costas loop + slicer in
 * one pass over the input (reference rrc_fir.c:17-30 evaluated only at the
 * samples qpsk.c:190 keeps, then qpsk.c:196-212 / costas_loop.c:44-74).
 *
 * Shape of the problem on MI355X ("rx_fused_pipe"):
 *   - the FIR is throughput work: 127 unfused mul+add pairs per symbol, any
 *     number of symbols in parallel;
 *   - the Costas loop is a strict recurrence per frame (phase -> sincos ->
 *     rotate -> detector -> phase): one wave can issue one VALU instruction
 *     per ~5 cycles, dependent ones every ~8, so a frame's 2048 symbols cost
 *     2048 x (instructions per step) x 5 cycles however many CUs idle.
 * So each workgroup is a producer/consumer pipeline in LDS:
 *   wave 0           the Costas recurrence (costas_asm.h), one lane per (frame, loop); it never waits
 *                    for HBM and leaves one 4-byte record per step in an LDS ring: the phase the step
 *                    started from (four steps per LDS write);
 *   FIR waves        each owns its frames outright (loads, history, filter, and the flush of their
 *                    records: sin/cos of the recorded phase again, de-rotation of the symbol -- still in the
 *                    symbol ring -- to costas_frame[], slicer, coalesced stores), so FIR waves never
 *                    synchronise with each other, only with wave 0 through two monotonic counters in LDS
 *                    (bounded spins; a timeout is reported through *status);
 *   spare waves      hardware waves that would land on wave 0's SIMD exit at once.
 * A full workgroup (16 frames) has three FIR waves of 4 frames (4 symbols per lane) and two of 2 frames
 * (2 symbols per lane): 1, 1.5, 1.5 filter units on the three SIMDs the serial wave leaves free.
 *
 * FIR wave layout of rx_fused_pipe_kernel (Geom<16,4,4,1>; rx_pipe2_kernel, rx_pipe2.hip, lays the same pipeline
 * out for 32 frames per workgroup): lane = (frame f of 4) x (q of 16); per chunk of S = 64
 * symbols the lane produces the R = 4 consecutive symbols 4q..4q+3 of its
 * frame with a sliding window: one 8-byte LDS read feeds up to 4 of the 508
 * multiply-adds, taps come from LDS broadcast reads (R + 1 groups of 8 live at
 * a time), each symbol's taps are summed 0..126 in one fp32 accumulator
 * (bit-exactness).
 * LDS image of a frame's window: position p (0 = the oldest sample the
 * chunk needs, i.e. sample chunk_start + index - 126) at float2 slot
 * p + p/32; lanes of one frame are 32 samples apart -> 33 slots -> the 16 x 2
 * lanes of a half wave hit 32 distinct even banks.  The per-frame decimation
 * index is absorbed when the window is WRITTEN (two per-lane base addresses),
 * so every FIR read is "one VGPR base + immediate".
 *
 * HBM traffic: every input sample is read exactly once (16-byte coalesced
 * loads, prefetched one chunk ahead into registers); 1 byte per symbol out.
 */
#ifndef QPSK_RX_PIPE_H
#define QPSK_RX_PIPE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qpsk_device.h"
#include "costas_asm.h"        /* the serial wave's streams: every pipeline kernel runs them (rx_hist_kernel their low-register build) */
#include "kernels.h"
#include "rx_profile.h"        /* the measurement build's hooks; empty in the product */

namespace qpsk {

namespace pipe {

constexpr int C = 8;            /* CYCLES this instantiation is built for */
constexpr int DR = 2;            /* depth of the symbol rings in chunks */
constexpr int MAX_WAVES = 16;    /* ready[] counters: FIR waves of rx_fused_pipe_kernel / two-frame units of rx_pipe2_kernel */
constexpr int SPIN_LIMIT = 1 << 24;

/*
 * Geometry of a workgroup.  The LDS (window + rings per frame) decides how many frames it holds:
 *   Geom<16, 4>  "narrow", the one the host uses: chunks of 64 symbols, 7.3 KB of LDS per frame, 16 frames per
 *                workgroup; the serial wave has a SIMD of its own (spare waves retire at once) and three SIMDs
 *                filter.  Lane mappings of its FIR waves: (frame of 4) x (q of 16) with 4 symbols per lane, or
 *                (frame of 2) x (q of 32) with 2 symbols per lane -- both in one workgroup when it is full (see
 *                the kernel).  Batches above 16 frames per CU go to rx_pipe2_kernel (api_rx.cpp).
 */
template <int QL_, int R_, int MAX_NF_, int SPARE_, bool PINNED_>
struct Geom {
    static constexpr bool PINNED = PINNED_;  /* FIR step with the product/add order pinned by hand (see the FIR loop) */
    static constexpr int QL = QL_;           /* lanes per frame */
    static constexpr int R = R_;             /* symbols per FIR lane per chunk */
    static constexpr int MAX_NF = MAX_NF_;   /* FIR waves per workgroup */
    static constexpr int SPARE = SPARE_;     /* 1: no FIR wave on the serial wave's SIMD (waves 4, 8 are launched and retire at once) */
    static constexpr int FWV = 64 / QL;      /* frames per FIR wave */
    static constexpr int S = R * QL;         /* symbols per chunk */
    static constexpr int CH = S * C;         /* samples per chunk per frame */
    static constexpr int TSTEPS = NTAPS + C * (R - 1);   /* window positions a lane sweeps per chunk */
    static constexpr int PAD = R * C;        /* lanes of a frame are PAD positions apart: position p lives at slot p + p/PAD */
    static constexpr int WL = CH + 128;      /* window positions kept per frame */
    /* padded image (two pad slots per PAD positions, see the FIR waves): 716 slots for the two-symbol lanes; frame
     * stride = 0 (mod 32) slots = 0 (mod 64) banks: the four frames whose lanes share a ds_read_b128 pass start in
     * bank quads 4q, which the 16 lanes of a pass then cover exactly once */
    static constexpr int WSLOTS = ((WL + 2 * (WL / (2 * C)) + 31) / 32) * 32;
    static constexpr int DSTRIDE = DR * S + 2;   /* float2 slots per frame row: 16-byte aligned rows (the Costas wave reads two
                                                    symbols per ds_read_b128), 4 dwords (mod 64) apart: lanes hit different bank quads */
    static constexpr int ZSTRIDE = DR * S + 4;   /* 4-byte records (the phase a step started from) per Costas row: 16-byte
                                                    aligned rows (four records per write), 4 dwords (mod 64) apart: 16 lanes x 16 bytes on 64 banks */
    static constexpr int MAX_THREADS = SPARE ? 512 : 64 * (MAX_NF + 1);   /* with spares: 3 + 2 FIR waves, 3 retiring ones */
    static_assert(QL == 16 && 64 % QL == 0 && 128 % PAD == 0, "slot arithmetic assumes 16 lanes per frame");
};
/* lane mapping of one FIR wave: QL lanes per frame, R symbols per lane */
template <int QL_, int R_>
struct WaveMap {
    static constexpr int QL = QL_, R = R_;
};
using GeomNarrow = Geom<16, 4, 4, 1, true>;
/* (Round 1 also had a "wide" geometry, Geom<16, 2, 8, 0>: 32 frames per workgroup in 32-symbol chunks, per-frame
 * windows, FIR waves beside the serial wave -- 0.365-0.379 ms at 8192 frames.  rx_pipe2_kernel (rx_pipe2.hip) replaces it.) */

#define QPSK_GEOM_CONSTANTS(GM)                                                                          \
    constexpr int QL = GM::QL, R = GM::R, FWV = GM::FWV, S = GM::S, CH = GM::CH, WSLOTS = GM::WSLOTS,    \
                  DSTRIDE = GM::DSTRIDE, ZSTRIDE = GM::ZSTRIDE, TSTEPS = GM::TSTEPS, PAD = GM::PAD,      \
                  MAX_NF = GM::MAX_NF;                                                                   \
    (void)QL; (void)R; (void)FWV; (void)S; (void)CH; (void)WSLOTS; (void)DSTRIDE; (void)ZSTRIDE;         \
    (void)TSTEPS; (void)PAD; (void)MAX_NF

struct Smem {
    float taps[128];
    int ready[MAX_WAVES];     /* chunks produced, per FIR wave */
    int consumed;             /* chunks consumed by the Costas wave */
    int abort_flag;
    int pad_[2];
    int est_index[16];        /* rx_fused_pipe_kernel with the FFT timing estimate in the launch: the workgroup's decimation offsets */
};

__device__ __forceinline__ int ld_acquire(const int *p)
{
    int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return v;
}

__device__ __forceinline__ void st_release(int *p, int v)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/* the context's status word lives in pinned host memory (api_ctx.cpp): the host reads it after any synchronisation */
__device__ __forceinline__ void report_status(int *status, int what)
{
    __hip_atomic_store(status, what, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

/* bounded wait until *p >= target; false if the workgroup gave up */
__device__ __forceinline__ bool wait_ge(int *p, int target, int *abort_flag)
{
    int spins = 0;
    while (ld_acquire(p) < target) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > SPIN_LIMIT || __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
            __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return false;
        }
    }
    return true;
}

} // namespace pipe

using namespace pipe;

/*
 * The serial wave: one lane per (frame, loop).  It waits for chunk c of its frame in the symbol ring (counter
 * ready[]), advances the loop over the chunk's symbols and leaves one 4-byte record per symbol in the record
 * ring (the phase the step started from, four steps per write), then publishes consumed = c + 1.  Shared by rx_fused_pipe_kernel (ring fed by FIR waves) and
 * costas_pipe_kernel (ring fed from already decimated symbols in global memory).
 */
/* which build of the instruction streams the serial wave runs: costas_asm.h's (VGPRs 100..143) or costas_asm_lo.h's (84..127: StreamLo,
 * beside its header's include in rx_hist.hip, the one unit that runs it) */
struct StreamHi {
    static constexpr int RING_GROUP = COSTAS_RING_GROUP;      /* steps per group of ring() / ring_pair(), the unit their k counts */
    template <class... A> static __device__ __forceinline__ void ring(A &&...a) { costas_asm_run_ring(a...); }
    template <class... A> static __device__ __forceinline__ void ring_pair(A &&...a) { costas_asm_run_ring_pair(a...); }
    template <class... A> static __device__ __forceinline__ unsigned run(A &&...a) { return costas_asm_run(a...); }
};

/* What the serial wave's loops ended on, held back instead of going to the status word (rx_hist_kernel: the loops ran on a GUESSED index,
 * and their verdict counts only for the frames the guess was right for).  One bit per lane of the serial wave; lane 0 writes the words,
 * then releases `done`. */
struct DeferredVerdict {
    unsigned over[2];         /* lanes whose loop went beyond the bounded 2 pi wrap (STATUS_PHASE_RANGE) */
    unsigned nonfinite[2];    /* lanes whose loop ended on a NaN / Inf state (STATUS_NONFINITE) */
    int done;
    int pad_[3];
};

template <class GM, class ST = StreamHi, class SM>   /* SM: Smem, or rx_lean_kernel's control block (ready[], consumed, abort_flag) */
__device__ __forceinline__ void costas_wave(const FusedArgs &a, SM *sm, const float2 *dring, float *zring, int G,
                                            int f0, int lane, int nchunks, int *status, DeferredVerdict *defer = nullptr)
{
    QPSK_GEOM_CONSTANTS(GM);
    const int nbw = a.nbw, N = a.nsym;
    /* =============================== Costas + slicer wave ===================================== */
    /* Alone on its SIMD the wave takes priority 3.  rx_pipe2_kernel may place a FIR wave beside it (a.share_simd0):
     * the recurrence has slack there (32 frames per workgroup: the filter is the limit) and a FIR wave that only
     * gets the serial wave's leftovers becomes the slowest of the workgroup, so the priorities are the other way
     * round: this wave 1, the FIR wave beside it 3 [measured: 0.335 -> 0.294 ms at 8192 frames] */
    if (a.share_simd0 != ((a.dbg & 512) != 0)) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(3);
    /* a.lean_pair (rx_lean_kernel, one loop per frame, at most 32 frames per workgroup): lanes 2g and 2g + 1 both carry frame g's loop
     * and share the two polynomial chains of its step between them (costas_asm.h, costas_asm_run_ring_pair); wherever the instruction
     * stream is not running the two lanes simply do the same thing */
    const bool pair = a.lean_pair != 0;
    const bool odd = pair && (lane & 1);
    const int g = pair ? lane >> 1 : lane / nbw, b = pair ? 0 : lane - g * nbw;
    const bool inwg = pair ? lane < 2 * G : lane < G * nbw;
    const bool active = inwg && f0 + g < a.nframes;
    Loop st = {0.0f, 0.0f};
    LoopGains lg = {0.0f, 0.0f, a.min_freq, a.max_freq};
    bool over = false;   /* a phase beyond the bounded 2 pi wrap (qpsk_device.h, phase_wrap) */
    if (active) {
        lg.alpha = a.gains[2 * b];
        lg.beta = a.gains[2 * b + 1];
        if (a.state_in) {
            st.phase = a.state_in[2 * ((size_t)(f0 + g) * nbw + b)];
            st.freq = a.state_in[2 * ((size_t)(f0 + g) * nbw + b) + 1];
            /* a caller's seed (qpsk_rx_batch_ext): set_phase() / set_frequency() here, in the prologue, so that the first record -- the
             * phase the first step starts from -- is the wrapped seed, and the -0 tests below see the state the steps will see */
            if (a.seed_setters) seed_setters(st.phase, st.freq, a.min_freq, a.max_freq, over);
        }
    }
    /* the FIR wave that feeds this lane: 4 frames each; in the mixed workgroup frames 12..15 come two per wave */
    const int gl = inwg ? g : 0;
    const int gw = a.mixed == 2 ? gl / 2 : a.mixed == 1 && gl >= 12 ? 3 + (gl - 12) / 2 : gl / FWV;
    const float2 *dl = dring + (size_t)gl * DSTRIDE;
    float *zl = zring + (size_t)(pair ? gl : lane) * ZSTRIDE;   /* this lane's records: the phase each symbol's step started from */
    /* one median-of-3 instead of two compare/select pairs when the clamp is the usual min < 0 < max */
    const bool fast_clamp = a.min_freq < 0.0f && a.max_freq > 0.0f;
    float ph = st.phase, fr = st.freq;
    /* Symbols that are exactly (+0, +0) -- a stream's first block, a squelched input, an all-zero frame -- trip the instruction
     * stream's exact-zero test in every group although its step is the reference's for them (costas_asm.h, `ign`).  When a group
     * is abandoned, the lanes that tripped the test look at the symbols they have ahead in the chunk: nothing but +0.0 there and no
     * -0 in the loop state excuses them from the test for that stretch, and the stream takes the group again.  Without this such a
     * lane sent its whole workgroup through the C++ step, six times the cost (a squelched stream among 16; config 2 with one silent
     * frame: the launch waits for that workgroup). */
    auto zero_run = [&](int from, int to) {       /* ring slots [from, to) of this lane's row, both even: 16-byte reads */
        const uint4 *p = reinterpret_cast<const uint4 *>(dl + from);
        unsigned acc = 0;
        for (int i = 0; i < (to - from) / 2; i++) {
            const uint4 v = p[i];
            acc |= v.x | v.y | v.z | v.w;
        }
        return acc == 0u;
    };
    auto excusable = [&](unsigned long long lanes, int from, int to) {       /* -> the lanes of `lanes` with such a stretch ahead */
        const bool z = ((lanes >> lane) & 1ull) != 0ull && __float_as_uint(ph) != 0x80000000u && __float_as_uint(fr) != 0x80000000u &&
                       zero_run(from, to);
        return (unsigned long long)__ballot(z);
    };
    const float al = lg.alpha, be = lg.beta, fmin_ = a.min_freq, fmax_ = a.max_freq;
    bool ok = true;
    prof::SerialProbe probe(a, lane);      /* the measurement build's accounting of this wave (rx_profile.h); nothing in the product */
    /* full chunks go through the stream that runs across the ring hand-overs (costas_asm.h, costas_asm_run_ring); a
     * first chunk that starts from a loaded phase of -0, a last partial one and the variants below stay chunk by chunk */
    const bool ring_stream = fast_clamp && !(a.dbg & (8 | 16 | probe.chunkwise_bits())) && S == 4 * COSTAS_ASM_GROUP && DR == 2;
    /* the frame's first chunk goes through the stream too unless some loop starts from a LOADED phase of -0 (the
     * stream's sin/cos form is exact everywhere else; a -0 frequency is kept away from it group by group below) */
    const int first_ring_chunk = __any(active && __float_as_uint(ph) == 0x80000000u) ? 1 : 0;
    for (int c = 0; c < nchunks && ok; c++) {
        if (ring_stream && c >= first_ring_chunk && (c + 1) * S <= N) {
            const int cfull = N / S;      /* chunks c .. cfull - 1 are whole */
            if (active) {
                /* the stream's unit here: groups of AG steps, GPC of them in a chunk and 2 GPC in the ring; k counts groups */
                constexpr int AG = ST::RING_GROUP;
                constexpr unsigned GPC = S == 4 * COSTAS_ASM_GROUP ? (unsigned)(S / AG) : 1u, RPOS = 2u * GPC - 1u;      /* (ring_stream: S is 64) */
                unsigned k = GPC * (unsigned)c;
                const unsigned kend = GPC * (unsigned)cfull;
                const unsigned d_base = lds_addr(dl), z_base = lds_addr(zl);
                const unsigned ready_addr = lds_addr(&sm->ready[gw]), consumed_addr = lds_addr(&sm->consumed);
                unsigned long long ign = 0ull;      /* lanes excused from the zero test up to the end of the chunk they are in */
                while (k < kend) {
                    if ((k & (GPC - 1u)) == 0u) {     /* entering a chunk: the stream left because it was not there yet (or this is the start) */
                        ok = wait_ge(&sm->ready[gw], (int)(k / GPC) + 1, &sm->abort_flag);
                        if (!__all(ok)) { ok = false; break; }
                        if (ign) {            /* still nothing but zeros?  (the stream stops at every chunk end while some lane is excused) */
                            const int at = (int)(k & RPOS) * AG;
                            ign = excusable(ign, at, at + S);
                        }
                    }
                    unsigned long long fl = 0ull;
                    bool ran = false;
                    if (!__any(__float_as_uint(fr) == 0x80000000u)) {
                        unsigned ks = __builtin_amdgcn_readfirstlane(k);
                        const unsigned kstop = ign ? min(kend, (ks | (GPC - 1u)) + 1u) : kend;
                        probe.enter_stream();
                        if (pair)
                            ST::ring_pair(ph, fr, d_base, z_base, ready_addr, consumed_addr, ks, kstop, al, be, fmin_, fmax_, odd, fl, ign);
                        else
                            ST::ring(ph, fr, d_base, z_base, ready_addr, consumed_addr, ks, kstop, al, be, fmin_, fmax_, fl, ign);
                        ran = true;
                        probe.leave_stream();
                        k = ks;
                    }
                    if ((!ran || fl != 0ull) && k < kend) {      /* group k abandoned (or never started) */
                        const int at = (int)(k & RPOS) * AG;
                        const unsigned long long fresh = fl & ~ign;
                        if (ran && fresh) {
                            const unsigned long long zm = excusable(fresh, at, ((int)(k & RPOS) | (int)(GPC - 1u)) * AG + AG);
                            if ((fresh & ~zm) == 0ull) { ign |= zm; continue; }      /* every lane that tripped: the stream again */
                        }
                        /* the C++ step, then on */
                        for (int i = 0; i < AG; i++) {
                            float tx, ty; unsigned qq;
                            zl[at + i] = ph;
                            costas_step_t<true>(ph, fr, al, be, fmin_, fmax_, dl[at + i], tx, ty, qq, over);
                        }
                        k++;
                        if ((k & (GPC - 1u)) == 0u && lane == 0) st_release(&sm->consumed, (int)(k / GPC));
                    }
                }
            }
            ok = __all(ok);
            c = cfull - 1;
            continue;
        }
        ok = wait_ge(&sm->ready[gw], c + 1, &sm->abort_flag);
        if (!__all(ok)) { ok = false; break; }
        probe.chunk_waited(c);
        const int slot = (c % DR) * S;
        const int cnt = min(S, N - c * S);
        if (active && !QPSK_ABLATE(a, 2)) { /* measurement build only: skip the recurrence */
            int j = 0;
            if (c == 0) { /* a loaded phase may be -0: first step with the form that is exact there too */
                Loop s0 = {ph, fr};
                zl[slot] = ph;
                costas_step<true>(s0, lg, dl[slot], over);
                ph = s0.phase; fr = s0.freq;
                j = 1;
                /* the stream below starts on a symbol number that is a multiple of 4 (16-byte aligned reads of
                 * symbol pairs and writes of four records) */
                for (; j < min(4, cnt); j++) {
                    float tx, ty; unsigned qq;
                    zl[slot + j] = ph;
                    if (fast_clamp) costas_step_t<true>(ph, fr, al, be, fmin_, fmax_, dl[slot + j], tx, ty, qq, over);
                    else costas_step_t<false>(ph, fr, al, be, fmin_, fmax_, dl[slot + j], tx, ty, qq, over);
                }
            }
            /* the wave only advances the loop and leaves each step's starting phase; de-rotation to z (sin/cos
             * again, from that phase), the slicer and costas_frame[] happen in the FIR waves' flush */
            /* the next symbol is fetched from LDS one whole step ahead, so the recurrence never waits for
             * the LDS pipe (which the FIR waves keep busy); reading one slot past the chunk is harmless
             * (next slot or the row's padding element) */
            if (fast_clamp && !(a.dbg & 8)) {
                /* groups of steps in the hand-scheduled stream (costas_asm.h); a group it abandons (exact-zero
                 * detector input, double wrap) is redone here with the C++ step, and so is one that would start
                 * with freq = -0 (loaded state only), where the stream's zero error has the wrong sign */
                constexpr int AG = COSTAS_ASM_GROUP;
                unsigned long long ign = 0ull;      /* lanes excused from the zero test for the rest of this chunk's whole groups */
                while (cnt - j >= AG) {
                    unsigned da = lds_addr(dl + slot + j), za = lds_addr(zl + slot + j);
                    unsigned long long fl = 0ull;
                    bool ran = false;
                    const unsigned want = __builtin_amdgcn_readfirstlane((unsigned)(cnt - j) / AG);   /* wave-uniform */
                    unsigned left = want;
                    if (!__any(__float_as_uint(fr) == 0x80000000u)) {
                        left = ST::run(ph, fr, da, za, want, al, be, fmin_, fmax_, fl, ign);
                        ran = true;
                    }
                    j += AG * (int)(want - left);
                    if (left != 0) {
                        const unsigned long long fresh = fl & ~ign;
                        if (ran && fresh) {
                            const unsigned long long zm = excusable(fresh, slot + j, slot + j + AG * (int)left);
                            if ((fresh & ~zm) == 0ull) { ign |= zm; continue; }
                        }
                        for (int i = 0; i < AG; i++, j++) {
                            float tx, ty; unsigned qq;
                            zl[slot + j] = ph;
                            costas_step_t<true>(ph, fr, al, be, fmin_, fmax_, dl[slot + j], tx, ty, qq, over);
                        }
                    }
                }
            }
            float2 dcur = dl[slot + j];
            if (fast_clamp) {
#pragma unroll 1
                for (; j < cnt; j++) {
                    const float2 dnext = dl[slot + j + 1];
                    float tx, ty; unsigned qq;
                    zl[slot + j] = ph;
                    costas_step_t<true>(ph, fr, al, be, fmin_, fmax_, dcur, tx, ty, qq, over);
                    dcur = dnext;
                }
            } else {
#pragma unroll 4
                for (; j < cnt; j++) {
                    const float2 dnext = dl[slot + j + 1];
                    float tx, ty; unsigned qq;
                    zl[slot + j] = ph;
                    costas_step_t<false>(ph, fr, al, be, fmin_, fmax_, dcur, tx, ty, qq, over);
                    dcur = dnext;
                }
            }
        }
        if (lane == 0) st_release(&sm->consumed, c + 1);
        probe.chunk_done();
    }
    probe.finish(nchunks, S);
    st.phase = ph; st.freq = fr;
    if (active && ok && !odd) {
        const size_t o = (size_t)(f0 + g) * nbw + b;
        if (a.freq) a.freq[o] = st.freq;
        if (a.phase) a.phase[o] = st.phase;
        if (a.hz) a.hz[o] = (float)((double)st.freq * a.rs / TAU); /* qpsk.c:217 */
        if (a.state_out) { a.state_out[2 * o] = st.phase; a.state_out[2 * o + 1] = st.freq; }
    }
    if (!ok && lane == 0) report_status(status, STATUS_PIPE_TIMEOUT);
    const bool nonfinite = !over && active && ok && !loop_state_finite(ph, fr);
    if (defer) {
        /* the caller decides per frame whether these count (a timeout, above, always does) */
        const unsigned long long mo = __ballot(over), mn = __ballot(nonfinite);
        if (lane == 0) {
            defer->over[0] = (unsigned)mo; defer->over[1] = (unsigned)(mo >> 32);
            defer->nonfinite[0] = (unsigned)mn; defer->nonfinite[1] = (unsigned)(mn >> 32);
            st_release(&defer->done, 1);
        }
        return;
    }
    if (over) report_status(status, STATUS_PHASE_RANGE);
    else if (nonfinite) report_status(status, STATUS_NONFINITE);
}

/*
 * Flush of one consumed chunk for one frame by its lanes (lane q owns symbols R q .. R q + R - 1 of the chunk):
 * record = the phase the symbol's step started from; with the symbol itself, still in the symbol ring (the slot
 * is refilled only after this flush, by the same wave), z = symbol x conj(e^{j phase}) = costas_frame[] (qpsk.c:197)
 * exactly as the step formed it, then the slicer (qpsk.c:74-79), R symbols per store.
 */
template <class GM, int RW = GM::R, bool DATA = false>   /* RW symbols per lane: S / RW lanes per frame; DATA: the data rule, not the slicer */
__device__ __forceinline__ void flush_records(const FusedArgs &a, const float *zring, const float2 *dring, int g, int frame,
                                              int q, int chunk, uint8_t *sym_row = nullptr)
{   /* sym_row (one loop per frame): where this frame's symbols go instead of a.sym + frame * nsym (rx_lean_kernel's pad rows) */
    constexpr int DSTRIDE = GM::DSTRIDE;
    constexpr int R = RW, S = GM::S, ZSTRIDE = GM::ZSTRIDE;
    static_assert(R == 2 || R == 4, "packs 2 or 4 symbols per store");
    const int nbw = a.nbw, N = a.nsym;
    const int slot = (chunk % DR) * S, sym0 = chunk * S;
    const int cnt = min(S, N - sym0);
    for (int b = 0; b < nbw; b++) {
        const int row = g * nbw + b;
        const size_t o = ((size_t)frame * nbw + b) * N + sym0 + R * q;
        float2 z[R];
        uint32_t packed = 0;
        /* the lane's R records and R symbols: rows are 16-byte aligned and R q is a multiple of R, so they come
         * as whole 8- or 16-byte LDS reads */
        float phv[R];
        float2 dv[R];
        {
            const float *zp = zring + (size_t)row * ZSTRIDE + slot + R * q;
            const float2 *dp = dring + (size_t)g * DSTRIDE + slot + R * q;
            if constexpr (R == 4) {
                const float4 p4 = *reinterpret_cast<const float4 *>(zp);
                const float4 da = reinterpret_cast<const float4 *>(dp)[0], db = reinterpret_cast<const float4 *>(dp)[1];
                phv[0] = p4.x; phv[1] = p4.y; phv[2] = p4.z; phv[3] = p4.w;
                dv[0] = make_float2(da.x, da.y); dv[1] = make_float2(da.z, da.w);
                dv[2] = make_float2(db.x, db.y); dv[3] = make_float2(db.z, db.w);
            } else {
                const float2 p2 = *reinterpret_cast<const float2 *>(zp);
                const float4 da = *reinterpret_cast<const float4 *>(dp);
                phv[0] = p2.x; phv[1] = p2.y;
                dv[0] = make_float2(da.x, da.y); dv[1] = make_float2(da.z, da.w);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++)
            z[r] = derotate<false>(phv[r], dv[r]);
        if (chunk == 0 && q == 0)   /* the frame's first symbol: its phase may be a loaded -0 */
            z[0] = derotate<true>(phv[0], dv[0]);
#pragma unroll
        for (int r = 0; r < R; r++)
            packed |= (uint32_t)(DATA ? data_rule(z[r]) : slicer(z[r])) << (8 * r);
        if (a.sym) {
            uint8_t *so = sym_row ? sym_row + sym0 + R * q : a.sym + o;
            if (R * q + R <= cnt && ((N | sym0) & (R - 1)) == 0) {   /* o is a multiple of R: one aligned store */
                if constexpr (R == 4) *reinterpret_cast<uint32_t *>(so) = packed;
                else *reinterpret_cast<uint16_t *>(so) = (uint16_t)packed;
            } else {
                for (int r = 0; r < R; r++)
                    if (R * q + r < cnt) so[r] = (uint8_t)(packed >> (8 * r));
            }
        }
        if (a.costas) {
            for (int r = 0; r < R; r++)
                if (R * q + r < cnt) a.costas[o + r] = z[r];
        }
    }
}

} // namespace qpsk
#endif
