/* kernels.h -- launch interface between the C-ABI layer (api_*.cpp) and kernels.hip */
#ifndef QPSK_KERNELS_H
#define QPSK_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace qpsk {

constexpr int LOOKBACK = 128;  /* >= 126 samples of FIR history, kept 16-byte friendly */
constexpr int LOOKAHEAD = 8;   /* the decimation offset can reach 7 (qpsk.c:173-180) */
constexpr int MAX_LDS_BYTES = 160 * 1024;
constexpr int MAX_INDEX = 7;
/* values a kernel stores in the context's status word (FusedArgs::status; api_ctx.cpp check_status) */
constexpr int STATUS_PIPE_TIMEOUT = 1;   /* the in-LDS producer/consumer pipeline exhausted its bounded spins */
constexpr int STATUS_PHASE_RANGE = 2;    /* a loop phase beyond the bounded 2 pi wrap (qpsk_device.h, phase_wrap) */
constexpr int STATUS_NONFINITE = 3;      /* a loop ended on a NaN / Inf phase or frequency: the input held a non-finite sample */
constexpr int STATUS_BAD_INDEX = 4;      /* a per-frame decimation offset outside 0..MAX_INDEX (caller-supplied: qpsk_rx_batch_ext); the kernel
                                            addressed with 0 instead */
constexpr int STATUS_EST_NONFINITE = 5;  /* qpsk_carrier_est_batch: a NaN / Inf sample inside the window the estimate reads */
constexpr int STATUS_SOFT_NONFINITE = 6; /* qpsk_soft_batch, qpsk_deframer_push_coded: a NaN / Inf sample among those a row's sums or soft output use, or a NaN / Inf gain */
constexpr int STATUS_SOFT_BAD_LAG = 7;   /* qpsk_soft_batch: a per-row lag that would leave the row; that row's soft output is zeros */

struct FusedArgs {
    const float2 *x;        /* [nframes] frames of frame_size samples, frame_pitch samples apart */
    size_t frame_pitch;     /* >= frame_size (qpsk_rx_batch: = frame_size) */
    int nframes, frame_size, cycles, nsym;
    int G, S;               /* frames per workgroup, symbols per chunk */
    int mixed;              /* rx_fused_pipe_kernel, set by its launcher: 0 = every FIR wave filters 4 frames, 4 symbols per
                               lane; 1 = 16 frames per workgroup, the last four by two waves of 2 frames with 2 symbols
                               per lane; 2 = every FIR wave 2 frames with 2 symbols per lane (see the kernel) */
    int share_simd0;        /* rx_pipe2_kernel, set by its launcher: a FIR wave sits beside the serial wave (priorities, see there) */
    const int32_t *index;   /* [nframes] or NULL -> fixed_index */
    int fixed_index;
    /* rx_fused_pipe_kernel, full 16-frame workgroups only (set by api_rx.cpp when the shape allows it): the FFT timing estimate
     * runs INSIDE the launch -- every hardware wave estimates two of the workgroup's frames before the pipeline starts
     * (timing_fft_wave.h) -- instead of in a launch of its own in front.  est_tw: size-512 twiddle table, est_cs: the CYCLES
     * candidate phases (both host-built, api_rx.cpp); index_out [nframes] or NULL receives the indices.  NULL = off */
    const double2 *est_tw, *est_cs;
    int32_t *index_out;
    int lean_twowin;        /* rx_lean_kernel, set by launch_rx_lean when the LDS allows it (workgroups of up to 16 frames): every two-frame unit has
                               a window of its own, so a two-unit FIR wave's DMAs run a whole unit ahead (fir_lean_loop2_dma2w) */
    int lean_dma;           /* rx_lean_kernel: 1 = FIR waves whose frames all have an even decimation offset stage their windows by LDS-DMA
                               (fir_lean_asm.h, the _dma loops); 0 = always through registers.  Same bits either way ("QPSK_LEAN_DMA") */
    int est_waves;          /* rx_lean_kernel with the FFT timing estimate inside the launch: hardware waves launched for it (0 = the library's 12, the most the register budget allows) ("QPSK_EST_WAVES") */
    int lean_pair;          /* rx_lean_kernel: the serial wave runs every loop in TWO lanes that share the step's sin/cos polynomial chains
                               (costas_asm.h, QPSK_BODY_P): 1 = in workgroups of up to 16 frames, 2 = up to 32, 3 = up to 24 (the library's rule), 0 = never; launch_rx_lean turns the wish into 0 / 1.  Same bits ("QPSK_LEAN_PAIR") */
    int dbg;                /* layout variants of the pipeline kernel, all bit-exact (qpsk_ctx_set_tuning "QPSK_PIPE_DBG"):
                               4 no spare waves, 8 C++ Costas step, 16 serial wave chunk by chunk (no stream across the ring hand-overs), 64 FIR waves that share a SIMD keep their hardware order (16-frame kernel), 128 one lane mapping for all FIR waves (the plain
                               layout).  Measurement build only (-DQPSK_PIPE_PROFILE; masked off by api_rx.cpp otherwise):
                               1 skip FIR arithmetic, 2 skip the Costas recurrence (both change the result), 32 print the
                               cycle accounting of workgroup 0's FIR waves */
    const float2 *dsrc;     /* costas_pipe_kernel only: decimated symbols, rows dstride symbols apart */
    int dstride;
    /* costas_pipe_kernel, streaming mode (qpsk.c:186-191): once symbol i of a row has been taken, its slot is
     * refilled with the next block's pick refill[frame][i*cycles + index[frame]] (0 past the block);
     * refill rows are frame_size samples apart.  NULL = leave dsrc alone */
    const float2 *refill;
    float2 *refill_dst;     /* = dsrc, writable */
    int refill_planar;      /* refill rows are [cycles][nsym] planes (phase-major: what stream_scan_kernel leaves) instead of frame_size samples */
    /* rx_fused_kernel as the fall-back pass of the one-pass histogram route (rx_hist_kernel, rx_hist.hip): the launch covers the frames
     * frame_list[0 .. *frame_list_count) instead of 0 .. nframes (both in device memory: the count is known only on the device; workgroups
     * beyond it retire at once); inputs, per-frame index and every output are addressed by the listed frame number.  NULL = off */
    const int32_t *frame_list, *frame_list_count;
    const float *taps;      /* [127] */
    const float *gains;     /* [nbw][2] alpha, beta */
    int nbw;
    float min_freq, max_freq;
    double rs;
    const float *state_in;  /* [nframes][nbw][2] phase, freq or NULL */
    int seed_setters;       /* state_in is a caller's seed (qpsk_rx_batch_ext): the serial wave applies set_phase() / set_frequency()
                               (costas_loop.c:117-132) at the load -- phase_wrap, then the [min_freq, max_freq] clamp.  0 = loaded raw
                               (qpsk_costas_batch, the streams' carried state) */
    float *state_out;       /* same or NULL */
    uint8_t *sym;           /* [nframes][nbw][nsym] */
    uint8_t *sym_pad;       /* rx_lean_kernel on a batch whose last workgroup is not full: [G][nsym] bytes for the pad frames' symbols (and for
                               the last real frame of an odd batch, whose two-frame unit reaches past the end); NULL = whole workgroups only */
    float *freq, *phase;    /* [nframes][nbw] or NULL */
    float2 *costas;         /* [nframes][nbw][nsym] or NULL */
    float *hz;              /* [nframes][nbw] or NULL */
    int *status;            /* the context's status word (pinned host memory): a kernel stores STATUS_* there when a
                               call's results are invalid (pipeline timeout, phase beyond the bounded 2 pi wrap) */
    /* costas_pipe_kernel behind stream_scan_kernel MODE 2 (carrier.h): a spare wave of workgroup 0 finishes the carrier table of the
     * next block.  carrier_state NULL = no spare wave */
    float *carrier_state;
    float2 *carrier_tab;
    int carrier_frame;      /* samples per block of that table */
    int data_rule;          /* rx_lean_kernel only (qpsk_rx_batch_data): sym / sym_pad receive the data rule's decisions (qpsk_device.h,
                               data_rule) instead of the slicer's.  0 = the slicer */
};

size_t fused_lds_bytes(int G, int S, int cycles, int nbw);
int prepare_kernels(void);
int launch_rx_fused(const FusedArgs &a, hipStream_t s);
/* rx_fused_pipe.hip: the producer/consumer pipeline kernel (CYCLES = 8 only; the pipeline's shape: rx_pipe.h) */
size_t pipe_lds_bytes(int NF, int nbw);
int pipe_frames(int NF);               /* frames of a workgroup with NF FIR waves: 4 per wave */
int pipe_cycles(void);
int pipe_max_nf(void);                 /* FIR waves per workgroup: 4 (16 frames) */
int prepare_pipe_kernel(void);           /* every pipeline kernel: the four units' own prepare_*() below, the first error wins */
#define QPSK_UNIT_LOCAL __attribute__((visibility("hidden")))      /* between the library's units only: not among its exported symbols */
QPSK_UNIT_LOCAL int prepare_costas_pipe(void);
QPSK_UNIT_LOCAL int prepare_rx_fused_pipe(void);
int launch_rx_fused_pipe(const FusedArgs &a, int NF, int *status, hipStream_t s);
int launch_costas_pipe(const FusedArgs &a, int NF, int *status, hipStream_t s);
/* rx_pipe2.hip: the pipeline kernel for up to 32 frames per workgroup (two-frame units, per-wave windows) */
size_t pipe2_lds_bytes(int G, int nwin, int nbw);      /* nwin = FIR waves (one window each) */
int pipe2_max_fir(void);
int pipe2_max_frames(void);
int pipe2_max_units_per_wave(void);
int pipe2_max_hw_waves(void);
unsigned long long pipe2_default_layout(int NU);        /* 4 bits per hardware wave: units it owns; 0 if NU does not fit */
/* THE decoder of a wave layout word on the host (the kernels deal their waves by the same word): what it adds up to -- the two-frame
 * units of all its waves, the waves that own any (one frame window each), the hardware waves to launch (the last owner's number + 1),
 * whether one sits beside the serial wave (hardware waves 4, 8) -- and whether it is one at all: nothing on wave 0 (the serial wave),
 * at most max_per_wave units on a wave, no unit on a hardware wave the kernels do not have */
struct LayoutCount {
    int units, nwin, hw;
    bool share_simd0, valid;
};
inline LayoutCount layout_count(unsigned long long layout, int max_per_wave = pipe2_max_units_per_wave())
{
    LayoutCount n = {0, 0, 1, false, (layout & 15) == 0};
    for (int w = 1; w < 16; w++) {
        const int cw = (int)((layout >> (4 * w)) & 15);
        if (cw > max_per_wave || (cw && w >= pipe2_max_hw_waves())) n.valid = false;
        n.units += cw;
        n.nwin += cw != 0;
        if (cw) n.hw = w + 1;
        if (cw && (w == 4 || w == 8)) n.share_simd0 = true;
    }
    return n;
}
int launch_rx_pipe2(const FusedArgs &a, int G, unsigned long long layout, int *status, hipStream_t s);
QPSK_UNIT_LOCAL int prepare_rx_pipe2(void);
/* rx_lean.hip: the same pipeline with the FIR waves' chunk loop as one hand-written stream (fir_lean_asm.h) */
size_t lean_lds_bytes(int G, int nwin);
unsigned long long lean_default_layout(int NU);         /* rx_lean_kernel: 1, 5, 5, 5 units on SIMDs 0-3 for a full workgroup */
bool lean_shape_ok(const FusedArgs &a, int G);          /* one loop per frame, whole chunks, an even workgroup size, ... */
int launch_rx_lean(const FusedArgs &a, int G, unsigned long long layout, int *status, hipStream_t s);
QPSK_UNIT_LOCAL int prepare_rx_lean(void);
bool lean_est_ok(const FusedArgs &a, int G, unsigned long long layout);   /* the FFT timing estimate inside rx_lean_kernel's launch fits this geometry */
/* rx_hist.hip: the reference's histogram timing mode in ONE pass (timing scan + receive path on a guessed index, verified per frame) */
bool rx_hist_shape_ok(const FusedArgs &a);
int launch_rx_hist(const FusedArgs &a, int32_t *index_true, const int32_t *hint, int32_t *mis_list, int32_t *mis_count, int *status, hipStream_t s);
int launch_index_majority(const int32_t *index, int nframes, int32_t *hint, int32_t *mis_count, int32_t *h_stats, hipStream_t s);
QPSK_UNIT_LOCAL int prepare_rx_hist(void);
int launch_rrc_fir(const float *x, const float *memory, float *y, const float *taps, int nframes, int length,
                   hipStream_t s, size_t in_pitch = 0);      /* in_pitch: samples between input frames (0 = length) */
/* firstream.hip: the same filter as the generated stream fir_full8s_asm.h (SYMMETRIC taps only: the caller checks) */
int launch_rrc_fir_stream(const float *x, const float *memory, float *y, const float *taps, int nframes, int length,
                          hipStream_t s, size_t in_pitch = 0, int ncu = 0);
/* its run geometry: a frame is ntiles 512-output tiles, cut into parts runs of tpp consecutive tiles (the last may be shorter), one
 * wave per run; ncu: compute units of the device (qpsk_test_fir_runs reports it) */
struct FirRuns { int ntiles, parts, tpp; };
FirRuns rrc_fir_stream_runs(int nframes, int length, int ncu);
int launch_delay_line(const float *x, float *memory, int nframes, int length, hipStream_t s);
/* firfast.hip: overlap-save FIR, 512-point fp32 FFTs (not a parity path); H, tw: [512][2] floats from qpsk_host_fir_fast_tables */
int launch_rrc_fir_fast(const float *x, const float *memory, float *y, const float *H, const float *tw, int nframes, int length,
                        hipStream_t s);
int rrc_fir_fast_hop(void);
int rrc_fir_fast_nfft(void);
int launch_timing_hist(const float *y, int nframes, int frame_size, int cycles, int32_t *index, int32_t *hist,
                       bool generic, hipStream_t s);   /* generic: always the any-CYCLES scan (test knob) */
int launch_costas(const float *d, int nframes, int nsym, int dstride, int nbw, const float *gains, float min_freq,
                  float max_freq, const float *state_in, float *state_out, uint8_t *sym, float *costas, int *status,
                  hipStream_t s);
int launch_decimate(const float *filtered, const int32_t *index, float *dec, int nstreams, int frame_size,
                    int cycles, int nsym, hipStream_t s);
int launch_mixer(const int16_t *pcm, float *out, float *state, int nstreams, int frame_size, hipStream_t s);
int launch_fft(const double *in, double *out, const double *tw, int nbatch, int n, int log2n, int inverse,
               hipStream_t s);                 /* n <= fft_lds_max_n(): one workgroup per transform, LDS-resident */
int fft_lds_max_n(void);
int fft_big_block(void);
int launch_fft_big(const double *in, double *out, const double *twb, const double *twn, int nbatch, int n, int log2n,
                   int inverse, hipStream_t s);   /* larger powers of two, two passes; in != out */
/* timing_scan.hip: full-rate FIR + histogram scan fused through LDS (CYCLES = 8, frame_size % timing_scan_tile() == 0) */
size_t timing_scan_lds_bytes(void);
int timing_scan_tile(void);
int prepare_timing_scan(void);
int launch_timing_scan(const float *x, int nframes, int frame_size, const float *taps, int32_t *index, int32_t *hist,
                       int *status, hipStream_t s, size_t pitch = 0, bool symmetric = false);   /* symmetric taps: the SGPR-tap stream */
/* timing_fft.hip */
int launch_timing_fft(const float *x, int nframes, int frame_size, int cycles, const float *taps, const double *tw,
                      const double *cs, int32_t *index, float *yout, double *Xout, double *Xk, hipStream_t s, size_t pitch = 0,
                      int ncu = 0, bool symmetric = false);   /* optional, for the parity tests: yout [nframes][512][2] the estimator's filtered samples,
                      Xout [nframes][512][2] the whole spectrum (selects the variant that runs the full transform beside the
                      pruned one), Xk [nframes][2] the symbol-rate bin as the pruned transform delivers it */
int timing_fft_nfft(void);
int timing_fft_first(void);
/* carrier_est.hip: the fourth-power carrier estimate (qpsk_carrier_est_batch) over S = [klo, khi] (kdef: the member of S with the
 * smallest |k|); tw: the size-n twiddle table; pitch in samples; each output may be NULL */
int prepare_carrier_est(void);
int launch_carrier_est(const float *x, size_t pitch, int nframes, int start, int n, int cycles, int klo, int khi, int kdef,
                       const float *taps, const double *tw, float *seed, float *freq, int32_t *bin, double *line, int *status,
                       bool symmetric, hipStream_t s);
/* streamblock.hip: one launch per rx_frame() block and stream (few, short streams: the reference's call pattern) */
struct StreamBlockArgs {
    const int16_t *pcm;     /* [n][frame_size] PCM (device memory or mapped pinned host memory), or NULL: */
    const float2 *cplx;     /* [n][frame_size] complex samples at the rrc_fir() call (qpsk.c:125) */
    float *mixer;           /* [n][4] carrier phase and step (PCM input), in/out */
    float2 *memory;         /* [n][127] delay lines, in/out */
    float2 *dec;            /* [n][nsym] decimated_frame[]: the previous block's picks in, this block's out */
    float *loop;            /* [n][2] phase, freq in/out */
    const float *loop_in;   /* [n][2] or NULL: loop state to start from instead of `loop` (host staging) */
    float *loop_out;        /* [n][2] or NULL: a second copy of the final state (host staging) */
    const float *taps, *gains;   /* [127]; [2] alpha, beta */
    float min_freq, max_freq;
    int frame_size, cycles, nsym, hist_timing, fixed_index;
    uint8_t *sym;           /* [n][nsym] */
    float2 *costas;         /* [n][nsym] or NULL */
    int32_t *index;         /* [n] or NULL */
    float2 *filtered;       /* [n][frame_size] or NULL */
    int *status;
    unsigned *done;         /* mapped pinned host counter or NULL: every wave adds 1 behind its last store (system scope), so the host
                               can watch the block finish instead of going through the stream's completion signal */
    /* the streams' ONE carrier (carrier.h; set together or not at all): this block's phases from ctab instead of each stream's own
     * recurrence (the longest stretch of wave 1's chain), the next block's into ctab_next by a third wave of workgroup 0 beside the
     * Costas wave; `mixer` is then neither read nor written */
    const float2 *ctab;
    float2 *ctab_next;
    float *cstate;
};
/* Blocks small enough travel INSIDE the kernel arguments (the dispatch packet's argument buffer is device memory the host writes
 * through the PCIe aperture: posted writes), so the kernel never reads host memory -- on this pool a read of pinned host memory
 * from the GPU takes 8-14 us, the whole budget of a 512-sample block [measured, profiles/r04_stream_block.txt] */
struct StreamBlockInline {
    static constexpr int MAX_STREAMS = 8, MAX_SAMPLES = 1024;      /* n <= 8 streams, n * frame_size <= 1024 samples (2 KB) */
    float loop[2 * MAX_STREAMS];
    uint4 pcm[MAX_SAMPLES / 8];
};
size_t stream_block_lds_bytes(int frame_size, int nsym);
int stream_block_max_frame(void);
int prepare_stream_block(void);
int launch_stream_block(const StreamBlockArgs &a, int nstreams, hipStream_t s, const StreamBlockInline *inl = nullptr);   /* inl: PCM and, if
                        a.loop_in is set (to anything), the loop state come from *inl instead of a.pcm / a.loop_in */
/* streamscan.hip: PCM -> mix -> rrc_fir() -> histogram timing of running streams in one kernel (CYCLES = 8 or 4, frame_size %
 * stream_scan_tile() == 0, symmetric taps); yout [n][cycles][frame_size / cycles] planar by decimation phase; updates mixer [n][4], memory [n][127] */
int stream_scan_tile(void);
int prepare_stream_scan(void);
int launch_stream_scan(const int16_t *pcm, const float *x, float *mixer, float *memory, float *yout, const float *taps, int32_t *index,
                       int nstreams, int frame_size, int *status, hipStream_t s, const float *ctab = nullptr, float *ctab_next = nullptr,
                       float *cstate = nullptr, unsigned cseq = 0, int cycles = 8);
/* the shared carrier of MODE 2 (streamscan.hip): cstate [8] = {phase the next table starts from, fbb_rx_rect, phase the last table
 * started from, the relay counter of stream_scan_kernel's spare waves (an unsigned int, wrapping: zero it with cseq = 0), unused}; a table = the frame_size
 * phases of one block; cseq = the number of MODE 2 launches since that counter was zeroed.  ctab != NULL selects MODE 2: this block's phases from ctab,
 * the next block's into ctab_next (by a spare wave of workgroup 0), cstate advanced; the per-stream mixer[] is then not touched */
int launch_carrier_table(float *cstate, float *tab, int frame_size, bool rest_only, hipStream_t s);   /* whole table, or what stream_scan_kernel left (carrier.h) */
int launch_carrier_broadcast(const float *cstate, float *mixer, int nstreams, hipStream_t s);   /* exactly one of pcm / x (complex blocks: no mixer) */
/* bitstages.hip */
int launch_crc16(const uint8_t *data, int npackets, int nbytes, uint16_t *crc, hipStream_t s);
int launch_interleave(uint8_t *data, int npackets, int nbytes, unsigned b, int dir, hipStream_t s);
int launch_scramble(uint8_t *sym, const uint8_t *keystream, int npackets, int nsym, hipStream_t s);
int launch_pack_dibits(const uint8_t *sym, uint8_t *packed, size_t nrows, int nsym, hipStream_t s);      /* sym 16-byte aligned when nsym % 16 == 0 */
/* sync.hip: the sync-word search of qpsk_sync_batch (h_sync: nsync <= SYNC_MAX_WORD dibits on the host, passed in the kernel arguments; the
 * caller has checked every bound), and the data rule over a costas_frame[] dump (qpsk_rx_batch_data off rx_lean_kernel) */
constexpr int SYNC_MAX_WORD = 128;
int launch_sync_search(const uint8_t *data, int nframes, int nsym, const uint8_t *h_sync, int nsync, int lag_min, int lag_max, int nout,
                       uint8_t *out, int32_t *lag, int32_t *rot, int32_t *score, hipStream_t s);
int launch_data_from_costas(const float2 *costas, uint8_t *data, size_t n, hipStream_t s);
/* soft.hip: qpsk_soft_batch (the definition: include/qpsk_hip.h).  One workgroup per row; pitch in symbols; mode = SOFT_MODE_*.
 * onepass: nsym <= SOFT_ONE_PASS_MAX, the row staged in LDS and read once (gain_in != NULL replaces the row's own gain);
 * sums: quality / sums / the gain per row into gain_out (each may be NULL); apply: soft output from gain [nrows] (check_gain: flag a
 * NaN / Inf entry).  lag, rot may be NULL (0) */
constexpr int SOFT_ONE_PASS_MAX = 4096;
constexpr int SOFT_MAX_NSYM = 1 << 21;
constexpr int SOFT_MODE_UNIT = 0, SOFT_MODE_LLR = 1;
int launch_soft_onepass(const float *x, size_t pitch, int nrows, int nsym, int skip, int mode, float scale, const float *gain_in,
                        const int32_t *lag, const int32_t *rot, int first, int nout, int8_t *soft, float *quality, double *sums, int *status,
                        hipStream_t s);
int launch_soft_sums(const float *x, size_t pitch, int nrows, int nsym, int skip, int mode, float scale, float *gain_out, float *quality,
                     double *sums, int *status, hipStream_t s);
int launch_soft_apply(const float *x, size_t pitch, int nrows, int nsym, const float *gain, bool check_gain, const int32_t *lag,
                      const int32_t *rot, int first, int nout, int8_t *soft, int *status, hipStream_t s);
/* viterbi.hip: qpsk_conv_encode_batch / qpsk_viterbi_batch (the definition: include/qpsk_hip.h).  One wave per row, lane = state; the
 * 64-bit decision word of every step waits for the trace-back in scratch ([nrows][viterbi_scratch_bytes_per_row] bytes: viterbi_kernel)
 * or, lds = true, in dynamic LDS (rows of up to VITERBI_LDS_MAX_BYTES: viterbi_lds_kernel).  pitch in steps; flip, and one of bits / info,
 * may be NULL.  The PROFILE flags exist in the measurement build only (make viterbi_profile, -DQPSK_VITERBI_PROFILE): stop after the
 * forward pass / info words 1, 2 = the shader cycles of the forward pass and of the trace-back */
constexpr int VITERBI_MAX_STEPS = 131072;
constexpr int VITERBI_LDS_MAX_BYTES = 65536;
constexpr int VITERBI_OPEN_START = 1, VITERBI_OPEN_END = 2, VITERBI_PROFILE_FORWARD_ONLY = 0x100, VITERBI_PROFILE_CYCLES = 0x200;
size_t viterbi_scratch_bytes_per_row(int nsteps);
/* a pattern of PUNCTURING (include/qpsk_hip.h), checked by the host (api_coded.cpp, punct_make): 1 <= period <= 32, no mask bit at or above
 * period, K = popc(keep0) + popc(keep1) > 0 = the sent bits of a period */
struct Puncture {
    int period;
    unsigned keep0, keep1;
    int K;
};
/* the sent bits of nsteps steps: idx(nsteps, 0) */
inline long long punct_nsent(const Puncture &p, int nsteps)
{
    const unsigned r = (unsigned)(nsteps % p.period), low = (1u << r) - 1u;
    return (long long)(nsteps / p.period) * p.K + __builtin_popcount(p.keep0 & low) + __builtin_popcount(p.keep1 & low);
}
/* a stride of INTERLEAVING (include/qpsk_hip.h), checked by the host (api_coded.cpp, ilv_make): n = 2 ntx bits on air, 1 <= s < max(n, 2),
 * gcd(s, n) = 1, s sinv = 1 mod n.  pi(k) = k s mod n is where sent bit k lies on air; on-air bit a is sent bit a sinv mod n */
struct Interleave {
    unsigned n, s, sinv;
};
/* what a kernel takes of it: k -> k m mod n for k < n <= 2^18, m = s (the decoder's pi) or sinv (the encoders' gather).  The definition forms
 * the product in 64 bits; here it is split at 2^9 -- k m = (k >> 9) (2^9 m mod n) + (k & 511) m < 2^28 -- so that one 32-bit remainder
 * reduces it and no 64-bit division is ever expanded.  m9 = 2^9 m mod n comes from the host */
struct IlvMul {
    unsigned n, m, m9;
    __host__ __device__ __forceinline__ unsigned at(unsigned k) const { return ((k >> 9) * m9 + (k & 511u) * m) % n; }
    /* at(k + 1) from at(k): one conditional subtract */
    __host__ __device__ __forceinline__ unsigned next(unsigned a) const { return a + m >= n ? a + m - n : a + m; }
    /* at(k + b) from at(k), b = 0 or 1 */
    __host__ __device__ __forceinline__ unsigned ahead(unsigned a, unsigned b) const { return b ? next(a) : a; }
};
inline IlvMul ilv_mul(unsigned n, unsigned m) { return IlvMul{n, m, (unsigned)(((unsigned long long)m << 9) % n)}; }
/* the identity beside it: the position map of a row that is not interleaved.  ahead() is a sum here and a select there, which is why the maps
 * say it themselves: written as a select over next() the punctured decoders cost scalar registers */
struct FlatMap {
    template <class Pos> __host__ __device__ __forceinline__ Pos at(Pos k) const { return k; }
    template <class Pos> __host__ __device__ __forceinline__ Pos next(Pos a) const { return a + 1; }
    template <class Pos> __host__ __device__ __forceinline__ Pos ahead(Pos a, unsigned b) const { return a + b; }
};
/* WHERE THE CODED BITS OF nsteps TRELLIS STEPS LIE IN THE TRANSMITTED ROW, said once for every stage of the coded path (the encoders, the
 * decoders, the framer, the coded deframer).  Three kinds, each the one before behind one more layer:
 *     CODED_PLAIN   rate 1/2: step t is dibit t of the row
 *     CODED_PUNCT   behind a pattern: sent bit k is flat bit k of the row's ntx dibits
 *     CODED_ILV     behind a pattern and a stride: sent bit k is flat bit pi(k)
 * The kind is the ENTRY POINT's, not the values': the pattern (1, 1, 1) behind qpsk_viterbi_punct_batch is CODED_PUNCT and runs the punctured
 * kernels.  Made and checked by the host (api_coded.cpp, layout_add_pattern / layout_add_stride); the layers a kind does not have keep the values below */
enum CodedKind { CODED_PLAIN = 0, CODED_PUNCT = 1, CODED_ILV = 2 };
struct CodedLayout {
    CodedKind kind = CODED_PLAIN;
    Puncture punct = {1, 1u, 1u, 2};
    Interleave ilv = {2u, 1u, 1u};
};
/* the sent bits of nsteps steps (2 nsteps at rate 1/2: the pattern a plain layout keeps says so), and their dibits on air, ntx */
inline long long coded_nsent(const CodedLayout &l, int nsteps) { return punct_nsent(l.punct, nsteps); }
inline long long coded_ndibits(const CodedLayout &l, int nsteps) { return (coded_nsent(l, nsteps) + 1) / 2; }
/* what every launch below asks of a layout and its steps; that K counts the masks' bits, s is coprime to n and sinv its inverse is the host's */
inline bool coded_layout_fits(const CodedLayout &l, int nsteps)
{
    if (nsteps < 1 || nsteps > VITERBI_MAX_STEPS || l.punct.period < 1 || l.punct.period > 32 || l.punct.K < 1 || l.punct.K > 64) return false;
    if (l.kind != CODED_ILV) return true;
    const long long ntx = coded_ndibits(l, nsteps);
    return ntx >= 1 && l.ilv.n == 2u * (unsigned)ntx && l.ilv.s >= 1 && l.ilv.s < l.ilv.n && l.ilv.sinv >= 1 && l.ilv.sinv < l.ilv.n;
}
/* the six decode kernels, by the layout's kind and lds: viterbi_kernel / viterbi_punct_kernel / viterbi_ilv_kernel and their _lds_ twins.  pitch
 * and flip go by the row's dibits on air (steps at rate 1/2, ntx otherwise); the residency rule goes by nsteps whatever the kind */
int launch_viterbi(const int8_t *soft, size_t pitch, int nrows, int nsteps, const CodedLayout &layout, const uint8_t *flip, int flags,
                   unsigned long long *scratch, bool lds, uint8_t *bits, int32_t *info, hipStream_t s);
/* conv_encode_kernel (one thread per step), or one thread per transmitted dibit: conv_encode_punct_kernel / conv_encode_ilv_kernel, dibits
 * [nrows][ntx], ntx >= 1 */
int launch_conv_encode(const uint8_t *bits, int nrows, int nbits, int nsteps, const CodedLayout &layout, uint8_t *dibits, hipStream_t s);
/* viterbi_stream.hip: the streaming decoder (VITERBI STREAM in include/qpsk_hip.h).  One wave per stream over state_stride bytes of state each
 * (vstream_state_stride(nring); the layout is that file's).  The host keeps the positions and hands a launch small numbers only:
 *     nring, dblk, wblk   (D + W) / 64, D / 64, W / 64
 *     pc                  pending steps the state holds, total % 64
 *     slot                push: the ring slot of the first block it completes; flush: the slot of the newest block (the partial one if pc > 0)
 *     have                push: the blocks the ring holds, min(total / 64, nring); flush: the blocks it walks, all of them emitted
 *     wphase              push: whole blocks since the last decision point, (total / 64) % wblk
 *     n, soft, pitch      push: the trellis steps of the call, and every stream's row of transmitted dibits, pitch dibits apart
 * bits rows bits_pitch bytes apart, info [nstreams][4]; one of the two may be NULL */
constexpr int VSTREAM_MAX_SPAN = 8192;      /* D + W at most */
constexpr int VSTREAM_TERMINATED = 1;
struct VStreamArgs {
    const int8_t *soft;
    size_t pitch;
    int n, pc, slot, have, wphase;
    int nring, dblk, wblk;
    int flags;                    /* flush: VSTREAM_TERMINATED */
    uint8_t *state;
    size_t state_stride;
    uint8_t *bits;
    size_t bits_pitch;
    int32_t *info;
    Puncture punct;
};
size_t vstream_state_stride(int nring);
int launch_vstream_init(const VStreamArgs &a, int nstreams, hipStream_t s);
/* viterbi_stream_kernel, or punctured = true viterbi_stream_punct_kernel */
int launch_vstream_push(const VStreamArgs &a, int nstreams, bool punctured, hipStream_t s);
int launch_vstream_flush(const VStreamArgs &a, int nstreams, hipStream_t s);
/* outer.hip: the outer link of a continuous stream (OUTER LINK in include/qpsk_hip.h).  One wave per stream over state_stride bytes of state
 * each (outer_state_stride(n, branches, lock); the layout is that file's).  The host keeps the bits since the reset and hands a launch `total`
 * (what the streams had before this push: a wave adds a relative position to it for the `pos` it stores, and takes its bit phase total & 7
 * from it) and the call's buffers: bits rows bits_pitch bytes apart; words [nstreams][max_words][word_pitch], pos and wflags
 * [nstreams][max_words], info [nstreams][4], each of these four or NULL; count [nstreams] */
constexpr int OUTER_POLARITY = 1, OUTER_MSB_FIRST = 2;
constexpr int OUTER_MAX_BITS = 1 << 20;
struct OuterArgs {
    int n, branches, sync, lock, drop, flags;
    uint8_t *state;
    size_t state_stride;
    long long total;
    const uint8_t *bits;
    size_t bits_pitch;
    int nbits, max_words;
    int32_t *count;
    uint8_t *words;
    size_t word_pitch;
    long long *pos;
    uint8_t *wflags;
    int32_t *info;
    int group;                    /* 0, or G = 3..16: group sync (qpsk_outer_reset_group); behind the fields the ungrouped kernel reads */
};
size_t outer_state_stride(int n, int branches, int lock);
int launch_outer_init(const OuterArgs &a, int nstreams, hipStream_t s);
int launch_outer_push(const OuterArgs &a, int nstreams, hipStream_t s);
/* outer_interleave_kernel: words / out [nrows][nwords][n]; hist_in / hist_out [nrows][branches - 1][n] or NULL */
int launch_outer_interleave(const uint8_t *words, int nrows, int nwords, int n, int branches, const uint8_t *hist_in, uint8_t *hist_out,
                            uint8_t *out, hipStream_t s);
/* dispersal.hip: DVB's energy dispersal over rows of len bytes (DVB TRANSPORT in include/qpsk_hip.h).  table [group][table_pitch]: what is
 * xored onto byte q of a row of group index k, table_pitch = dispersal_table_pitch(len) a multiple of 4 so that every table row is dword
 * aligned (api_dispersal.cpp builds it on the host); wflags [nrows] (the index of row r is wflags[r] >> 4, a row with an index >= group is
 * copied) or NULL (the index is (first + r) mod group).  Pitches in bytes, never 0 */
constexpr int DISPERSAL_MSB_FIRST = 1;
constexpr int DISPERSAL_MAX_GROUP = 16;
constexpr int dispersal_table_pitch(int len) { return (len + 3) & ~3; }
int launch_dispersal(const uint8_t *in, size_t in_pitch, int nrows, int len, int group, const uint8_t *table, const uint8_t *wflags, int first,
                     uint8_t *out, size_t out_pitch, hipStream_t s);
/* nodesync.hip: the node sync in front of the streaming decoder (NODE SYNC in include/qpsk_hip.h).  One wave per link over NODESYNC_STRIDE bytes
 * of state each (the layout is that file's).  The host keeps the dibits since the reset and hands a launch `have` = min(total, nshift - 1), the
 * dibits of history that are real.  soft_in / soft_out rows in_pitch / out_pitch dibits apart; vinfo [nlinks][4] or NULL (no tick); info
 * [nlinks][8] or NULL */
constexpr int NODESYNC_MAX_SHIFT = 32;
constexpr int NODESYNC_MAX_NTX = 1 << 20;
constexpr size_t NODESYNC_STRIDE = 96;
struct NodeSyncArgs {
    int nrot, nshift, span, settle, thr_num, thr_den, drop;
    uint8_t *state;
    int have;
    const int8_t *soft_in;
    size_t in_pitch;
    int ntx;
    const int32_t *vinfo;
    int8_t *soft_out;
    size_t out_pitch;
    int32_t *info;
};
/* nodesync_init_kernel: a reset's state (keep = false), or qpsk_nodesync_set (keep = true: the history and `switches` stay); cand [nlinks] or NULL */
int launch_nodesync_init(const NodeSyncArgs &a, int nlinks, const int32_t *cand, bool keep, hipStream_t s);
int launch_nodesync_push(const NodeSyncArgs &a, int nlinks, hipStream_t s);
/* conv_encode_stream_kernel: nbits whole periods with an even number of sent bits; state_in / state_out [nrows] or NULL */
int launch_conv_encode_stream(const uint8_t *bits, int nrows, int nbits, const Puncture &p, const uint8_t *state_in, uint8_t *state_out,
                              uint8_t *dibits, hipStream_t s);
/* deframe.hip: qpsk_deframer_push.  Per stream, state_stride bytes of state: the header, the carried tail (the ring values of the last
 * min(len, nsync-1) dibits) at DEFRAME_TAIL_OFFSET, the pending packet's received payload (ring values) at DEFRAME_PEND_OFFSET */
struct DeframeHeader {
    long long len;          /* dibits pushed since the reset */
    long long h;            /* the hunt resumes at this position */
    long long ppos;         /* the pending packet: its sync word's position, rotation, score, payload dibits received */
    int pending, have, prot, pscore;
};
constexpr int DEFRAME_TAIL_OFFSET = 64, DEFRAME_PEND_OFFSET = 192;
constexpr int DEFRAME_MAX_BYTES = 1024, DEFRAME_MAX_PACKETS = 64, DEFRAME_MAX_NSYM = 1 << 21;
/* what the one hunt (deframe_hunt.h) reads, the base of both pushes' arguments (api_packets.cpp, deframer_push_begin) */
struct DeframeHuntArgs {
    int nstreams, nsym;
    int nsync, min_score;
    uint8_t *state;
    size_t state_stride;
    unsigned long long sync_lo[2], sync_hi[2];   /* bit i % 64 of word i / 64: bit 0 / bit 1 of ring(sync[i]) */
    long long *pos;
    int32_t *rot, *score;
    int32_t *count;               /* last, with bytes first behind it: the decode kernels fetch the two with one scalar load */
};
/* a packet's record r = stream * max_packets + slot, by lane 0 */
__device__ __forceinline__ void report(const DeframeHuntArgs &a, size_t r, long long pos, int rot, int score, int lane)
{
    if (a.pos) {                  /* the pointer tests stay scalar branches around lane 0's stores */
        if (lane == 0) a.pos[r] = pos;
    }
    if (a.rot) {
        if (lane == 0) a.rot[r] = rot;
    }
    if (a.score) {
        if (lane == 0) a.score[r] = score;
    }
}
struct DeframeArgs : DeframeHuntArgs {
    uint8_t *bytes;
    const uint8_t *data;          /* exactly one of data [nstreams][nsym] / costas [nstreams][nsym] */
    const float2 *costas;
    int nbytes, max_packets;
    int bytes_per_lane;           /* ceil((nbytes + 2) / 64): the packet bytes one lane builds */
    const uint8_t *keystream;     /* [nbytes + 2]: the scrambler's keystream packed four dibits to the byte */
    const uint16_t *crc_adv;      /* [64]: x^(8 k) mod the CRC-16 polynomial, k = the data bytes behind lane l's chunk */
    uint8_t *crc_ok;
};
int launch_deframe(const DeframeArgs &a, hipStream_t s);
/* deframe_coded.hip: qpsk_deframer_push_coded.  The same per-stream state, with the pending packet's received body as int8 soft pairs
 * (2 nbody bytes) at DEFRAME_PEND_OFFSET.  Two launches: the hunt, which quantises the body symbols of this push and leaves every
 * packet it completes as a soft row in the staging buffer -- row stream * per_stream + slot, slot = the packet's output row -- and the
 * decode, one wave per staging row (rows at or beyond the stream's count retire at once) */
constexpr int DEFRAME_CODED_MAX_STEPS = 8 * (DEFRAME_MAX_BYTES + 2) + 6;
struct DeframeCodedArgs : DeframeHuntArgs {
    uint8_t *bytes;
    const float2 *costas;         /* [nstreams][nsym] */
    const float *gain;            /* [nstreams]: this push's gain per stream */
    int check_gain;               /* the gains are the caller's: flag a NaN / Inf one */
    int nbytes, max_packets;
    int nsteps;                   /* trellis steps of a packet: 8 (nbytes + 2) + 6 */
    int per_stream;               /* staging rows per stream: min(max_packets, nsym / (nsync + Nc) + 1), the most a push completes */
    int8_t *stage;                /* [nstreams * per_stream][stage_pitch][2] (DeframeCodedBody) */
    const uint8_t *flip;          /* [nbody]: the scrambler's keystream dibits, over the body on air */
    const uint16_t *crc_adv;      /* [nbytes]: x^(8 m) mod the CRC-16 polynomial */
    unsigned crc_init;            /* crc16()'s register after nbytes zero bytes from 0xFFFF */
    uint8_t *crc_ok;
    int32_t *info;
    int *status;
};
/* the body on air and its layout as the decode kernels take it, a kernel argument of its own beside the hunt's */
struct DeframeCodedBody {
    int nbody;                    /* Nc, the dibits of a body on air: coded_ndibits(layout, nsteps) */
    int stage_pitch;              /* dibits between staging rows: nbody rounded up to even, so that every row is 4-byte aligned */
    int kind;                     /* PADDING that keeps punct where it was: its four words come with one aligned scalar load.  Holds the layout's
                                   * CodedKind for a reader of a dump; no kernel reads it (they are instances by kind): do not branch on it */
    Puncture punct;               /* CODED_PUNCT, CODED_ILV: the pattern */
    /* the stride's IlvMul is the decode kernels' own trailing argument, not a field here: see deframe_coded_decode_kernel */
};
int launch_deframe_coded_hunt(const DeframeCodedArgs &a, const DeframeCodedBody &b, hipStream_t s);
/* rows [row0, row0 + nrows) of the staging buffer through deframe_coded_decode_kernel<lds, kind>; lds: the decision words in LDS
 * (viterbi_scratch_bytes_per_row(nsteps) <= VITERBI_LDS_MAX_BYTES), otherwise in scratch ([nrows] rows of that many bytes) */
int launch_deframe_coded_decode(const DeframeCodedArgs &a, DeframeCodedBody b, const CodedLayout &layout, int row0, int nrows,
                                unsigned long long *scratch, bool lds, hipStream_t s);
/* frame.hip: qpsk_frame_batch (the definition: include/qpsk_hip.h, FRAMER).  One wave per packet; the caller has checked every bound */
constexpr int FRAME_MAX_BYTES = DEFRAME_MAX_BYTES, FRAME_MAX_PER_ROW = 64, FRAME_MAX_ROW = DEFRAME_MAX_NSYM;
struct FrameArgs {
    const uint8_t *payload;       /* [npackets] payloads of nbytes bytes, pitch bytes apart */
    size_t pitch;
    uint8_t *out;                 /* [npackets / per_row][row_len] dibits */
    uint16_t *crc;                /* [npackets] or NULL */
    const uint8_t *ks;            /* [max(row_len, nbody)]: the scrambler's keystream dibits */
    int npackets, per_row, nbytes, nsync;
    int nbody;                    /* B, the dibits of a body on air */
    int lead, gap, row_len;
    int bytes_per_lane;           /* ceil(nbytes / 64): the payload bytes one lane's CRC share covers */
    int coded;                    /* the body is convolutionally coded; nsent and punct are then the layout's, set by launch_frame */
    unsigned nsent;
    Puncture punct;
};
/* h_sync [nsync] dibits (taken & 3); h_crc_adv [65]: x^(8 k_l) mod the CRC-16 polynomial, k_l = the payload bytes behind lane l's chunk, then
 * the init value's share 0xFFFF x^(8 nbytes).  Both travel in the kernel arguments */
/* frame_kernel<uncoded> (a.coded = 0; the layout is not looked at), frame_kernel<coded> (CODED_PUNCT: the framer's coded body always lies behind a pattern,
 * (1, 1, 1) included) or frame_ilv_kernel (CODED_ILV); a.nbody = coded_ndibits(layout, 8 (a.nbytes + 2) + 6) */
int launch_frame(const FrameArgs &a, const CodedLayout &layout, const uint8_t *h_sync, const uint16_t *h_crc_adv, hipStream_t s);
/* rs.hip: the Reed-Solomon outer code (the definition: include/qpsk_hip.h, REED-SOLOMON).  One wave per codeword; pitches in bytes, never 0
 * here; the caller has checked every bound and every overlap.  erase [nrows][n] or NULL; out or info may be NULL, not both */
constexpr int RS_MAX_ROOTS = 64;
void rs_generator(int nroots, uint8_t *g);      /* host: nroots + 1 coefficients, highest first; 1 <= nroots <= RS_MAX_ROOTS */
int launch_rs_encode(const uint8_t *data, size_t data_pitch, int nrows, int k, int nroots, uint8_t *out, size_t out_pitch, hipStream_t s);
int launch_rs_decode(const uint8_t *in, size_t in_pitch, int nrows, int n, int nroots, const uint8_t *erase, uint8_t *out, size_t out_pitch,
                     int32_t *info, hipStream_t s);
/* rs_cross.hip: the packet erasure code (the definition: include/qpsk_hip.h, PACKET ERASURE CODE).  One workgroup per group, a lane per byte
 * column; pitches in bytes, never 0 here; the caller has checked every bound and every overlap.  out or info may be NULL, not both; out may
 * be `in` with the same pitch; colfail and base may be NULL */
int launch_rs_cross_encode(uint8_t *group, size_t pitch, int ngroups, int k, int nroots, int len, int skip, hipStream_t s);
int launch_rs_cross_decode(const uint8_t *in, size_t pitch, int ngroups, int n, int nroots, int len, int skip, const uint8_t *have,
                           uint8_t *out, size_t out_pitch, int32_t *info, uint8_t *colfail, hipStream_t s);
int launch_rs_cross_place(const uint8_t *bytes, size_t byte_pitch, const int32_t *count, const uint8_t *crc_ok, int nstreams, int max_packets,
                          int len, int n, int ngroups, const int32_t *base, uint8_t *group, size_t pitch, uint8_t *have, hipStream_t s);
/* channel.hip: the polyphase channeliser (the definition: include/qpsk_hip.h, CHANNELISER).  A workgroup of channel_threads(M) threads takes
 * channel_tile(M) consecutive output times: 16384 complex values of LDS image from M = 1024 on (one workgroup of 1024 threads per compute
 * unit), 8192 below (256 threads), at most 128 times.  x [T M]; proto [P M]; tw [M / 2]; hist [(P - 1) M] (NULL at P = 1); chan [nsel], every
 * entry in [0, M): the caller has checked them, and every overlap; out rows pitch >= T elements apart */
constexpr int CHANNEL_MAX_M = 4096, CHANNEL_MAX_P = 32, CHANNEL_MAX_SEL = 1 << 16;
constexpr long long CHANNEL_MAX_SAMPLES = 1ll << 30;      /* T M of one push */
/* log2 M of a power of two in 2..CHANNEL_MAX_M, -1 for any other M: both banks' test of M, on the host and in the launchers */
constexpr int channel_log2(int M)
{
    if (M < 2 || M > CHANNEL_MAX_M || (M & (M - 1))) return -1;
    int l = 1;
    while ((1 << l) < M) l++;
    return l;
}
constexpr int channel_threads(int M) { return M >= 1024 ? 1024 : 256; }
constexpr int channel_tile(int M) { return M >= 1024 ? 16384 / M : M >= 64 ? 8192 / M : 128; }
/* the LDS image of tb rows: element e of a row at e + (e >> 5), rows M + (M >> 5) + 1 elements apart (channel_fft.h) */
constexpr size_t channel_lds_bytes(int M, int tb) { return (size_t)(M + (M >> 5) + 1) * (size_t)tb * sizeof(float2); }
int prepare_channel();
int launch_channel_push(const float2 *x, int T, int M, int P, const float *proto, const float2 *tw, const float2 *hist, const int32_t *chan, int nsel,
                        float2 *out, size_t pitch, hipStream_t s);
/* polyphase.hip: the history of all three polyphase stages moves on.  polyphase_history_kernel: next [rows][n] = per row the last n values
 * of hist [n] followed by in [K], the rows of `in` in_pitch >= K >= 1 elements apart; next is neither of them.  K < n shifts the history.
 * The banks' is one row: n = (P - 1) M, K = T M */
int launch_polyphase_history(const float2 *hist, const float2 *in, size_t in_pitch, size_t K, int rows, size_t n, float2 *next, hipStream_t s);
/* synth.hip: the polyphase synthesis bank (the definition: include/qpsk_hip.h, SYNTHESIS BANK), two launches through the scratch V [T][M] of
 * transformed vectors.  synth_transform_kernel has the channeliser's geometry (channel_tile, channel_threads): in [nsel] rows pitch >= T
 * elements apart; chan [nsel], DISTINCT entries in [0, M): the caller has checked them, and every overlap.  synth_filter_kernel: a lane
 * takes SYNTH_RUN consecutive times of one branch; hist [P - 1][M] (NULL at P = 1) = the vectors before the push; x [T M].  The history
 * moves on with launch_polyphase_history(hist, V, T M, T M, 1, (P - 1) M, next) */
constexpr long long SYNTH_MAX_SAMPLES = 1ll << 27;      /* T M of one push: a scratch of 1 GiB */
constexpr int SYNTH_RUN = 16;
int prepare_synth();
int launch_synth_transform(const float2 *in, size_t pitch, int T, int M, const float2 *tw, const int32_t *chan, int nsel, float2 *V, hipStream_t s);
int launch_synth_filter(const float2 *V, const float2 *hist, int T, int M, int P, const float *proto, float2 *x, hipStream_t s);
/* resample.hip: the batched polyphase rational resampler (the definition: include/qpsk_hip.h, RESAMPLER).  A workgroup of RESAMPLE_TILE
 * threads takes one stream and RESAMPLE_TILE consecutive outputs; the L P taps lie in LDS (64 KiB at most).  A tile's input window is at
 * most resample_window(L, D, P) samples; where that is no more than RESAMPLE_WIN_MAX (32 KiB behind the taps) it is staged in LDS, otherwise
 * every lane loads its own samples.  in [nstreams] rows of nin, in_pitch elements apart (may be NULL at nin = 0); hist [nstreams][P]; r the
 * carried position, 0 or in [D - L, D); nin must be the K the position gives for nout: the launcher refuses any other.  The caller has checked
 * the extents and every overlap.  The history moves on with launch_polyphase_history(hist, in, in_pitch, nin, nstreams, P, next) where nin > 0 */
constexpr int RESAMPLE_MAX_L = 512, RESAMPLE_MAX_D = 4096, RESAMPLE_MAX_P = 32, RESAMPLE_MAX_STREAMS = 1 << 16, RESAMPLE_MAX_OUT = 1 << 24;
constexpr int RESAMPLE_TILE = 256, RESAMPLE_WIN_MAX = 4096;
constexpr long long resample_window(int L, int D, int P) { return (long long)(RESAMPLE_TILE - 1) * D / L + 1 + P; }
constexpr bool resample_staged(int L, int D, int P) { return resample_window(L, D, P) <= RESAMPLE_WIN_MAX; }
/* the taps, padded to a whole float2, then the window where it is staged */
constexpr size_t resample_lds_bytes(int L, int D, int P, bool staged)
{
    return (size_t)((L * P + 1) & ~1) * sizeof(float) + (staged ? (size_t)resample_window(L, D, P) * sizeof(float2) : 0);
}
int prepare_resample();
int launch_resample_push(const float2 *in, size_t in_pitch, int nin, const float2 *hist, const float *proto, int nstreams, int L, int D, int P, int r,
                         int nout, float2 *out, size_t out_pitch, hipStream_t s);
/* txchain.hip */
int tx_history_symbols(void);        /* symbols of state per transmitter (uint8 each, 4 = none yet) */
int launch_tx_shape(const uint8_t *sym, uint8_t *hist, const float *taps, float *sig, int nstreams, int nsym,
                    int cycles, hipStream_t s);   /* shaped baseband of nsym symbols per transmitter; updates hist */
int launch_tx_upmix(const float *sig, int16_t *pcm, float *state, int nstreams, int length, hipStream_t s);
int launch_fill_i32(int32_t *p, int n, int32_t v, hipStream_t s);
int launch_sincos_hash(uint32_t first, uint32_t count, unsigned long long *acc, hipStream_t s);

} // namespace qpsk
#endif
