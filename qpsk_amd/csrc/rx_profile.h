/*
 * rx_profile.h -- everything the MEASUREMENT BUILD (make -C qpsk_amd/csrc profile: -DQPSK_PIPE_PROFILE, libqpsk_hip_prof.so) adds to the
 * receive pipeline kernels (rx_pipe.h and the four units that include it), as probes the kernels call unconditionally.
 *
 * The product build is the first half of this file: every probe is an empty always-inline body, so a call site costs the shipped kernels
 * nothing, and nothing but this header changes between the two builds.  The measurement build is the second half: cycle accounting of the
 * serial wave and of the FIR waves (FusedArgs::dbg bit 5 = 32, bits 11 and 12 with it), result-changing ablations (bits 0, 1 and the lean
 * streams' 14-20), frame-source overrides (bits 21, 22) and the wall-clock timeline of one rx_lean_kernel launch (bit 23).  api_rx.cpp masks
 * those bits off in the product (PIPE_VARIANT_MASK), which therefore computes the reference's result whatever the environment says.
 *
 * The units are built without relocatable device code, so a __device__ variable cannot be shared between them: each unit that includes
 * this header has its own g_timeline.  Only rx_lean_kernel's launches are ever read back, so the copy that counts is rx_lean.hip's, where
 * qpsk_prof_timeline (the read-back) lives too.
 */
#ifndef QPSK_RX_PROFILE_H
#define QPSK_RX_PROFILE_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "kernels.h"

#ifndef QPSK_PIPE_PROFILE
/* ====================================== the product: no probe does anything ====================================================== */
#define QPSK_ABLATE(a, bit) false

namespace qpsk {
namespace prof {

/* the serial wave (costas_wave) */
struct SerialProbe {
    __device__ __forceinline__ SerialProbe(const FusedArgs &, int /* lane */) {}
    __device__ __forceinline__ int chunkwise_bits() const { return 0; }      /* dbg bits that keep the wave chunk by chunk, beside 8 and 16 */
    __device__ __forceinline__ void enter_stream() {}
    __device__ __forceinline__ void leave_stream() {}
    __device__ __forceinline__ void chunk_waited(int /* chunk */) {}
    __device__ __forceinline__ void chunk_done() {}
    __device__ __forceinline__ void finish(int /* nchunks */, int /* symbols per chunk */) {}
};

/* a FIR wave of rx_fused_pipe_kernel / rx_pipe2_kernel: tick(k) closes phase k of a chunk (-1: starts the clock) */
struct FirProbe {
    __device__ __forceinline__ explicit FirProbe(const FusedArgs &) {}
    __device__ __forceinline__ void tick(int) {}
    __device__ __forceinline__ void report_fir_wave(int /* lane */, int /* wave */, int /* symbols per lane */, int /* nchunks */) {}
    __device__ __forceinline__ void report_fir_wave2(int /* lane */, int /* wave */, int /* units */, int /* nchunks */) {}
};

/* rx_lean_kernel */
__device__ __forceinline__ void timeline_entry(const FusedArgs &, int /* tid */) {}
__device__ __forceinline__ void timeline_stamp(const FusedArgs &, int /* lane */, int /* slot */) {}
__device__ __forceinline__ void timeline_wave_end(const FusedArgs &, int /* lane */, int /* hardware wave */) {}
__device__ __forceinline__ size_t frame_number(const FusedArgs &, int /* frame of the workgroup */, size_t frame) { return frame; }
__device__ __forceinline__ unsigned long long frame_source(const FusedArgs &, int /* f0 */, int /* frame of the workgroup */, unsigned long long src)
{
    return src;
}
/* has a measured stream run in the ordinary one's place (and left its status in st)? */
template <int NUW, class LaneAddr>
__device__ __forceinline__ bool lean_measured_stream(const FusedArgs &, unsigned, unsigned, unsigned, unsigned, unsigned, const LaneAddr &, int, int, int,
                                                     int &)
{
    return false;
}

} // namespace prof
} // namespace qpsk

#else
/* ====================================== the measurement build ==================================================================== */
/* Result-changing ablation knobs (FusedArgs::dbg bit 0: skip the filter arithmetic, bit 1: skip the recurrence) */
#define QPSK_ABLATE(a, bit) (((a).dbg & (bit)) != 0)

namespace qpsk {
namespace prof {

/* dbg bit 23: wall-clock stamps (100 MHz constant clock) of one rx_lean_kernel launch, 48 per workgroup: [0] entry, [1..4] the serial wave
 * in costas_wave / at its first step / behind its last step / at its end, [5 + w] the end of hardware wave w, [16 + w] FIR wave w behind
 * the workgroup's barrier, [32 + w] in front of its stream (tools/lean_timeline.py reads them through qpsk_prof_timeline) */
static __device__ unsigned long long g_timeline[1024 * 48];

__device__ __forceinline__ unsigned long long shader_clock()
{
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
__device__ __forceinline__ unsigned long long wall_clock()
{
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

/* the serial wave (costas_wave).  dbg 32: workgroup 0's cycles per chunk, waiting for the FIR waves / stepping, chunk by chunk (2048 with
 * it: the wait of single chunks); dbg 32 | 4096: the ring stream stays on and is timed instead (cycles inside the stream / outside it),
 * workgroups 0 and 77; dbg 4096 | 8388608: every workgroup leaves the wall-clock stamps of its serial wave in the timeline */
struct SerialProbe {
    const FusedArgs &a;
    const int lane;
    const bool cprof, timeline, ring_prof;
    unsigned long long cw = 0, cs = 0, ct = 0;
    unsigned long long rp_in = 0, rp_out = 0, rp_t = 0, rp_calls = 0, rp_rt0 = 0, rp_rt1 = 0, rp_rt2 = 0;

    __device__ __forceinline__ SerialProbe(const FusedArgs &a_, int lane_)
        : a(a_), lane(lane_), cprof((a_.dbg & 32) && blockIdx.x == 0), timeline((a_.dbg & 8388608) != 0),
          ring_prof((a_.dbg & 4096) != 0 && (blockIdx.x == 0 || blockIdx.x == 77 || timeline))
    {
        unsigned long long dummy = 0;
        ctick(dummy);
        rp_rt0 = rp_real();
    }
    __device__ __forceinline__ void ctick(unsigned long long &acc)
    {
        if (cprof) {
            const unsigned long long t = shader_clock();
            acc += t - ct;
            ct = t;
        }
    }
    __device__ __forceinline__ unsigned long long rp_real() const { return ring_prof ? wall_clock() : 0ull; }
    __device__ __forceinline__ void rp_tick(unsigned long long &acc)
    {
        if (ring_prof) {
            const unsigned long long t = shader_clock();
            if (rp_t) acc += t - rp_t;
            rp_t = t;
        }
    }
    /* the accounting per chunk needs the wave chunk by chunk (32, unless 4096 asks for the ring stream's own timing); so does the
     * ablated recurrence (2) */
    __device__ __forceinline__ int chunkwise_bits() const { return 2 | ((a.dbg & 4096) ? 0 : 32); }
    __device__ __forceinline__ void enter_stream()
    {
        rp_tick(rp_out);
        if (rp_calls++ == 0) rp_rt1 = rp_real();
    }
    __device__ __forceinline__ void leave_stream()
    {
        rp_tick(rp_in);
        rp_rt2 = rp_real();
    }
    __device__ __forceinline__ void chunk_waited(int c)
    {
        const unsigned long long before = cw;
        ctick(cw);
        if (cprof && lane == 0 && (a.dbg & 2048) && (c < 4 || c % 8 == 0)) printf("  serial wave: chunk %d waited %llu cycles\n", c, cw - before);
    }
    __device__ __forceinline__ void chunk_done() { ctick(cs); }
    __device__ __forceinline__ void finish(int nchunks, int S)
    {
        if (cprof && lane == 0 && !ring_prof)
            printf("serial wave: %d chunks; cycles per chunk: wait for the FIR waves %llu, steps %llu\n", nchunks, cw / nchunks, cs / nchunks);
        if (timeline) {
            if (lane == 0 && blockIdx.x < 1024) {
                unsigned long long *tl = g_timeline + 48 * blockIdx.x;
                tl[1] = rp_rt0; tl[2] = rp_rt1; tl[3] = rp_rt2; tl[4] = rp_real();
            }
        } else if (ring_prof && lane == 0)
            printf("wg %3d serial wave: %d chunks, %llu entries into the stream; cycles per chunk inside the stream %llu (= %llu per step), "
                   "outside it (waiting for the FIR waves, redone groups) %llu; wall time (100 MHz clock): wave start -> first step %.2f us, "
                   "first -> last step %.2f us\n", (int)blockIdx.x, nchunks, rp_calls, rp_in / nchunks,
                   rp_in / nchunks / S, rp_out / nchunks, (double)(rp_rt1 - rp_rt0) * 0.01, (double)(rp_rt2 - rp_rt1) * 0.01);
    }
};

/* dbg 32: where a FIR wave of workgroup 0 spends its shader cycles.  tick(k) adds the time since the last tick to phase k of
 * 0 wait for the loop, 1 flush, 2 window staging, 3 filter, 4 ring hand-over (-1: starts the clock) */
struct FirProbe {
    const bool on;
    unsigned long long tacc[5] = {0, 0, 0, 0, 0}, tlast = 0;
    __device__ __forceinline__ explicit FirProbe(const FusedArgs &a) : on((a.dbg & 32) && blockIdx.x == 0) {}
    __device__ __forceinline__ void tick(int k)
    {
        if (on) {
            const unsigned long long t = shader_clock();
            if (k >= 0) tacc[k] += t - tlast;
            tlast = t;
        }
    }
    __device__ __forceinline__ void report_fir_wave(int lane, int w, int R, int nchunks)
    {
        if (on && lane == 0)
            printf("FIR wave %d (%d symbols per lane): %d chunks; cycles per chunk: wait for the loop %llu, flush %llu, history + window %llu, "
                   "filter %llu, ring hand-over %llu\n", w, R, nchunks, tacc[0] / nchunks, tacc[1] / nchunks, tacc[2] / nchunks,
                   tacc[3] / nchunks, tacc[4] / nchunks);
    }
    __device__ __forceinline__ void report_fir_wave2(int lane, int widx, int nuw, int nchunks)
    {
        if (on && lane == 0)
            printf("FIR wave %d (%d units): %d chunks; cycles per chunk: wait for the loop %llu, flush %llu, window staging %llu, "
                   "filter %llu, ring hand-over %llu\n", widx, nuw, nchunks, tacc[0] / nchunks, tacc[1] / nchunks, tacc[2] / nchunks,
                   tacc[3] / nchunks, tacc[4] / nchunks);
    }
};

/* ---- rx_lean_kernel: the timeline (dbg bit 23) */
__device__ __forceinline__ void timeline_entry(const FusedArgs &a, int tid)
{
    if ((a.dbg & 8388608) && tid == 0) {
        const unsigned long long t = wall_clock();
        if (blockIdx.x < 1024) g_timeline[48 * blockIdx.x] = t;
    }
}
__device__ __forceinline__ void timeline_stamp(const FusedArgs &a, int lane, int slot)
{
    if ((a.dbg & 8388608) && lane == 0 && blockIdx.x < 1024) g_timeline[48 * blockIdx.x + slot] = wall_clock();
}
__device__ __forceinline__ void timeline_wave_end(const FusedArgs &a, int lane, int hwave)
{
    if ((a.dbg & 8388608) && lane == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long t = wall_clock();
        if (blockIdx.x < 1024 && hwave < 11) g_timeline[48 * blockIdx.x + 5 + hwave] = t;
    }
}

/* ---- rx_lean_kernel: where frame k of the workgroup whose first frame is f0 is read from (WRONG frame -> output mapping; the visit
 * order of the batch in memory is what is measured).  dbg bit 21: a workgroup's frames a grid apart instead of adjacent */
__device__ __forceinline__ size_t frame_number(const FusedArgs &a, int k, size_t frame)
{
    return (a.dbg & 2097152) ? (size_t)k * gridDim.x + blockIdx.x : frame;
}
/* dbg bit 22: the workgroup's frames as one contiguous tile per chunk (see gen_lean_asm.py, "tiled") */
__device__ __forceinline__ unsigned long long frame_source(const FusedArgs &a, int f0, int k, unsigned long long src)
{
    return (a.dbg & 4194304) ? (unsigned long long)(a.x + (size_t)f0 * a.frame_pitch) + (unsigned long long)k * 4096ull : src;
}

#ifdef QPSK_FIR_LEAN_PROF_ASM_H      /* the unit that runs the lean streams includes fir_lean_prof_asm.h in front of this header */
/* ---- rx_lean_kernel: a measured stream in the ordinary one's place.  dbg 32: the stream with cycle stamps between the phases of a unit;
 * otherwise streams with a part of the work left out (WRONG results): 1 the filter's multiplies and adds, 16384 its window reads, 32768
 * the flush's arithmetic, 65536 the window staging writes, 262144 the symbol stores, 524288 the hand-over write of the symbols -- what
 * each costs in time and in energy at the board's power limit (one at a time: the first bit set wins); 4194304 with the frame source of
 * bit 22; 1048576: the unit's loads issued frame-alternating (right results).  -> true if one ran; its status is in st */
template <int NUW, class LaneAddr>
__device__ __forceinline__ bool lean_measured_stream(const FusedArgs &a, unsigned prm, unsigned rd, unsigned voff, unsigned symoff, unsigned smem,
                                                     const LaneAddr &w, int lane, int hwave, int nchunks, int &st)
{
    if (a.dbg & 32) {
        unsigned pf[FIR_LEAN_NPROF];
        const unsigned long long t0 = shader_clock();
        if constexpr (NUW == 2) st = fir_lean_loop2_prof(prm, rd, voff, symoff, smem, w, pf);
        else st = fir_lean_loop1_prof(prm, rd, voff, symoff, smem, w, pf);
        const unsigned long long t1 = shader_clock();
        if ((blockIdx.x == 0 || blockIdx.x == 77) && lane == 0)
            printf("wg %3d FIR wave hw %2d (%d units): %d chunks, %llu cycles in the stream; per chunk: samples %u, stage+loads %u, "
                   "filter+gain %u, wait for the loop %u, flush %u, hand-over %u\n", (int)blockIdx.x, hwave, NUW, nchunks, t1 - t0,
                   pf[0] / nchunks, pf[1] / nchunks, pf[2] / nchunks, pf[3] / nchunks, pf[4] / nchunks, pf[5] / nchunks);
        return true;
    }
    if (!(a.dbg & (1 | 16384 | 32768 | 65536 | 262144 | 524288 | 1048576 | 4194304))) return false;
#define QPSK_LEAN_ABLATED(SFX) (NUW == 2 ? fir_lean_loop2_##SFX(prm, rd, voff, symoff, smem, w) : fir_lean_loop1_##SFX(prm, rd, voff, symoff, smem, w))
    if (a.dbg & 1) st = QPSK_LEAN_ABLATED(avalu);
    else if (a.dbg & 16384) st = QPSK_LEAN_ABLATED(alds);
    else if (a.dbg & 32768) st = QPSK_LEAN_ABLATED(aflush);
    else if (a.dbg & 65536) st = QPSK_LEAN_ABLATED(astage);
    else if (a.dbg & 262144) st = QPSK_LEAN_ABLATED(astore);
    else if (a.dbg & 524288) st = QPSK_LEAN_ABLATED(aring);
    else if (a.dbg & 4194304) st = QPSK_LEAN_ABLATED(atiled);
    else st = QPSK_LEAN_ABLATED(aorder);
#undef QPSK_LEAN_ABLATED
    return true;
}
#endif

} // namespace prof
} // namespace qpsk
#endif
#endif
