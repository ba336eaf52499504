/*
 * qpsk_hip.h -- C ABI of libqpsk_hip.so, the MI355X (gfx950) implementation of
 * the MonsieurETM/QPSK receive path:
 *
 *     rrc_fir()  ->  timing estimate  ->  Costas loop  ->  symbol slicer
 *     (reference qpsk.c:88-218, rrc_fir.c:17-30, costas_loop.c:44-74)
 *
 * Two layers, both plain C (pointers and sizes only, no C++/torch types):
 *
 *  1. qpsk_dropin.h -- the reference's own function signatures (rrc_fir,
 *     rrc_make, the costas_loop.h API, fft/fftn/ifft/ifftn, rx_frame,
 *     qpsk_demod) as process-wide singletons, exactly as the reference has
 *     them; they run on the GPU through layer 2.
 *
 *  2. this file -- context-carrying BATCHED entry points, the form in which
 *     the path is fast: many independent frames (or streams) per call, data
 *     already resident in HBM, one HIP stream per context.
 *
 * Conventions
 *   - complex float  == float[2]  (re, im) == HIP float2   (rrc_fir.h:16)
 *   - complex double == double[2]                          (fft.h:46-49)
 *   - every "d_" pointer is DEVICE memory on the context's GPU; "h_" is host.
 *   - every function returns QPSK_OK (0) or a negative qpsk_status; the text
 *     of the last error of the calling thread is qpsk_last_error().
 *     The reference itself has no error paths (all void); anything that could
 *     only fail here (no GPU, bad shape, HIP error) is reported, never
 *     silently computed on the CPU: there is NO host fallback in this library.
 *   - calls on one context are ordered on its stream; outputs are valid after
 *     qpsk_ctx_sync() (or after synchronising the stream the caller supplied).
 *
 * Stream ordering (the contract)
 *   The library enqueues every kernel and copy of a context on THAT context's stream and on nothing else; it does
 *   not order its work against any other stream of the caller.  So:
 *     - a buffer handed to a call must have been produced on the context's stream, or the caller must have ordered
 *       its producer before the call (event / synchronisation);
 *     - memory that a stream-ordered allocator (PyTorch's caching allocator, hipMallocAsync pools) recycles must be
 *       recycled in the context's stream order too: give the library the allocator's stream (qpsk_ctx_create /
 *       qpsk_ctx_set_stream), or synchronise before handing over recycled memory.  A library stream that the
 *       allocator does not know writes into memory whose previous contents queued kernels of the allocator's stream
 *       still have to read (this build's round-1 abort: DESIGN.md section 1);
 *     - outputs may be read by other streams only after an event / synchronisation on the context's stream.
 *   NULL means the HIP default stream, with its usual implicit ordering against blocking streams.
 */
#ifndef QPSK_HIP_H
#define QPSK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPSK_NTAPS 127 /* rrc_fir.h:13 */

typedef enum {
    QPSK_OK = 0,
    QPSK_ERR_NO_DEVICE = -1, /* no HIP device / device index out of range */
    QPSK_ERR_ARG = -2,       /* null pointer, non-positive size, frame_size % cycles != 0, ...; also, from the next synchronising
                                call, an external timing offset (qpsk_rx_batch_ext d_index_in) outside 0..7 */
    QPSK_ERR_HIP = -3,       /* a HIP runtime call or a kernel launch failed */
    QPSK_ERR_ALLOC = -4,
    QPSK_ERR_STATE = -5,     /* call sequence error (e.g. stream call on a context made for 0 streams) */
    QPSK_ERR_RANGE = -6      /* a Costas loop phase left the range the bounded 2 pi wrap covers (|phase| > ~25,000 rad:
                                input some 10^5 times the modem's working amplitude, or non-finite).  The reference's
                                phase_wrap() (costas_loop.c:61-67) spins |phase| / 2 pi times there and never returns once
                                |phase| >= 2^27; a GPU wave must not, so the call fails instead */
} qpsk_status;

/* How the decimation offset ("index", qpsk.c:105,173-180,190) is chosen. */
typedef enum {
    QPSK_TIMING_HIST = 0,  /* the reference's amplitude-histogram heuristic, qpsk.c:127-180 */
    QPSK_TIMING_FIXED = 1, /* caller-supplied offset: the bandwidth-bound fused kernel */
    QPSK_TIMING_FFT = 2    /* symbol-rate spectral line of |y|^2 via the radix-2 FFT (new design, no
                              reference counterpart: SURVEY section 0, 8(a) A7) */
} qpsk_timing_mode;

/* The reference's compile-time #defines and main()'s literals as run-time
 * parameters (qpsk.h:16-23, qpsk.c:302,308). */
typedef struct {
    double fs;          /* FS, sample rate in Hz                        qpsk.h:16 */
    double rs;          /* RS, symbol rate in Hz; CYCLES = (int)(fs/rs) qpsk.h:17,21 */
    int frame_size;     /* FRAME_SIZE, complex samples per frame/block  qpsk.h:23 */
    float rrc_alpha;    /* third argument of rrc_make()                 qpsk.c:308 */
    float loop_bw;      /* create_control_loop(loop_bw, min, max)       qpsk.c:302 */
    float min_freq;
    float max_freq;
    int timing_mode;    /* qpsk_timing_mode */
    int fixed_index;    /* used by QPSK_TIMING_FIXED, 0 <= fixed_index */
} qpsk_params;

typedef struct qpsk_ctx qpsk_ctx;

const char *qpsk_last_error(void);
const char *qpsk_version(void);
int qpsk_device_count(void);

/* main()'s defaults: FS 9600, RS 2400, FRAME_SIZE 512, alpha .35, loop TAU/100, clamp +-1 (qpsk.c:302,308) */
void qpsk_params_default(qpsk_params *p);

/* device < 0: current HIP device.  stream: the hipStream_t every call of this context is enqueued on;
 * NULL = the HIP default stream (the caller owns the stream and keeps it alive). */
int qpsk_ctx_create(qpsk_ctx **out, int device, const qpsk_params *p, void *stream);
void qpsk_ctx_destroy(qpsk_ctx *ctx);
int qpsk_ctx_sync(qpsk_ctx *ctx);
/* the kernels' status word WITHOUT a synchronisation: QPSK_OK, or what a kernel that has completed so far flagged (as qpsk_ctx_sync()
 * would report it).  For callers that order their own streams and events against the context's (include below: MULTI does). */
int qpsk_ctx_check(qpsk_ctx *ctx);
int qpsk_ctx_set_stream(qpsk_ctx *ctx, void *stream);
/* Kernel-geometry selection for tests and measurements (never needed for results: every geometry computes the same
 * bits).  Names: "QPSK_PIPE_V", "QPSK_PIPE_G", "QPSK_PIPE_NF", "QPSK_PIPE_LAYOUT_LO", "QPSK_PIPE_LAYOUT_HI", "QPSK_PIPE_DBG" (layout
 * bits, csrc/kernels.h), "QPSK_FUSED_G", "QPSK_FUSED_S", "QPSK_FUSED_LDS", "QPSK_FUSED_GENERIC", "QPSK_HIST_GENERIC" (1: histogram
 * timing through the rrc_fir + scan kernels instead of the fused scan kernel, 2: with the any-CYCLES scan), "QPSK_FIR_GENERIC" (1: the
 * compiler-scheduled full-rate filter and LDS-tap streams also for symmetric taps), "QPSK_FFT_FUSED" (0: the FFT timing estimate always as
 * a launch of its own), "QPSK_STREAM_BLOCK" (0: streams never take the one-launch-per-block kernel, 1: whenever the shape allows),
 * "QPSK_STREAM_POLL" (0: qpsk_streams_rx_pcm_host waits with hipStreamSynchronize), "QPSK_STREAM_SCAN" (streams with histogram
 * timing: 1 = mixer + filter + scan as one kernel whatever the stream count, 0 = never), "QPSK_STREAM_CARRIER" (0: that kernel runs every
 * stream's carrier recurrence although all streams share one), "QPSK_LEAN_DMA" (0: rx_lean_kernel stages its filter windows through
 * registers even where it would use LDS-DMA: frames with an even timing offset; 2: LDS-DMA, but one window per FIR wave even where the LDS
 * has room for one per two-frame unit), "QPSK_HIST_ONEPASS" (histogram timing: 0 = always the two-launch route -- timing scan, then the receive kernel -- 1 = the one-pass
 * route, rx_hist_kernel on the previous batch's majority index plus a fall-back pass over the frames it missed, whenever a guess exists;
 * unset: that route only while every frame of the context's last histogram-mode batch sat on that batch's majority index -- a missed
 * frame costs more than the route saves), "QPSK_EST_WAVES" (hardware waves that share the
 * in-launch FFT timing estimate), "QPSK_LEAN_PAIR" (rx_lean_kernel's serial wave: 0 = one lane per Costas loop, 1 = two lanes per
 * loop -- they share the step's sine / cosine polynomial chains -- in workgroups of up to 16 frames, 2 = up to 32; the library's own choice is up to 24),
 * "QPSK_VITERBI_LDS" (qpsk_viterbi_batch: 0 = the decision words always wait in the context's scratch buffer, 1 = in LDS whenever a row's
 * fit -- up to 8192 steps; the library's own choice is LDS where every row of the call is resident at once), "QPSK_VITERBI_CHUNK_ROWS"
 * (qpsk_viterbi_batch, qpsk_viterbi_punct_batch, qpsk_viterbi_ilv_batch and the decode of qpsk_deframer_push_coded off the LDS route: v >= 1 = at most v rows per
 * launch where that is fewer than the scratch buffer's 1 GiB cap allows -- the key only lowers the cap, and the buffer is sized for the
 * smaller chunk; 0 is refused with QPSK_ERR_ARG, here and as an environment value by qpsk_ctx_create(), where text that is not an
 * integer leaves the key unset; no effect on the LDS route);
 * value < 0 = back to the library's own choice.
 * Environment variables of the same names are read once, by qpsk_ctx_create(), as the context's initial values;
 * no other call reads the environment, and none of them can change a result. */
int qpsk_ctx_set_tuning(qpsk_ctx *ctx, const char *name, int value);
int qpsk_ctx_cycles(const qpsk_ctx *ctx);   /* CYCLES */
int qpsk_ctx_nsym(const qpsk_ctx *ctx);     /* FRAME_SIZE / CYCLES */
/* Name of the receive kernel the context's last qpsk_rx_batch() / qpsk_rx_batch_bw() launched ("" before the first
 * call): which of the library's geometries served that batch shape.  For measurement records (bench.py), not
 * results -- every geometry computes the same bits.  The string is static storage. */
const char *qpsk_ctx_last_kernel(const qpsk_ctx *ctx);

/* Host-side copies of what rrc_make() / create_control_loop() produced for this context. */
int qpsk_ctx_get_taps(const qpsk_ctx *ctx, float h_taps[QPSK_NTAPS]);
int qpsk_ctx_get_gains(const qpsk_ctx *ctx, float *h_alpha, float *h_beta);
/* Replace them (the reference lets the caller do both: rrc_make(), set_alpha()/set_beta()). */
int qpsk_ctx_set_taps(qpsk_ctx *ctx, const float h_taps[QPSK_NTAPS]);
int qpsk_ctx_set_loop(qpsk_ctx *ctx, float alpha, float beta, float min_freq, float max_freq);

/* -------------------------------------------------------------------------
 * Batch of INDEPENDENT frames -- the hot path.
 *
 * For each of nframes frames of frame_size complex samples this is, bit for
 * bit, what the reference computes with a fresh process:
 *       rx_frame(frame); rx_frame(zeros);      (qpsk.c:88-218; complex input
 * enters at the rrc_fir() call, qpsk.c:125; the second call is the flush that
 * the one-block pipeline delay of qpsk.c:186-197 needs)
 * taking costas_frame[], the slicer bits and the loop state after the second
 * call.
 *
 *   d_in      [nframes][frame_size] complex float
 *   d_sym     [nframes][nsym] uint8   (bits[1]<<1)|bits[0] of qpsk_demod(), qpsk.c:74-79,270
 *   d_freq    [nframes] float         get_frequency() after the frame  (rad/symbol)
 *   d_phase   [nframes] float         get_phase()
 *   d_costas  [nframes][nsym] complex float, costas_frame[] (qpsk.c:197)   -- may be NULL
 *   d_index   [nframes] int32, the decimation offset used                  -- may be NULL
 *   d_hz      [nframes] float, fbb_offset_freq = freq*RS/TAU (qpsk.c:217)  -- may be NULL
 * ------------------------------------------------------------------------- */
int qpsk_rx_batch(qpsk_ctx *ctx, const float *d_in, int nframes, uint8_t *d_sym, float *d_freq,
                  float *d_phase, float *d_costas, int32_t *d_index, float *d_hz);

/* The same with the frames frame_pitch complex samples apart in d_in (frame_pitch >= frame_size, even; the samples between
 * two frames are never read).  Why a caller would: with frames a power of two apart (16384 samples = 128 KB) every frame's
 * sample n sits in the same HBM channel group, and a batch kernel streams sample n of ALL its frames at about the same time --
 * measured on MI355X, the memory side then delivers 4.4 TB/s to this access pattern against 5.2 TB/s at a pitch of
 * frame_size + 512 samples.  Every timing mode. */
int qpsk_rx_batch_pitched(qpsk_ctx *ctx, const float *d_in, long long frame_pitch, int nframes, uint8_t *d_sym,
                          float *d_freq, float *d_phase, float *d_costas, int32_t *d_index, float *d_hz);

/* The same with nbw Costas loops per frame sharing one FIR pass (loop
 * bandwidth sweep, README.md:12).  Outputs are [nframes][nbw][...]. */
int qpsk_rx_batch_bw(qpsk_ctx *ctx, const float *d_in, int nframes, const float *h_loop_bw, int nbw,
                     uint8_t *d_sym, float *d_freq, float *d_phase, int32_t *d_index);

/* -------------------------------------------------------------------------
 * The same batch with the acquisition supplied from OUTSIDE ("ext"): the caller's own timing offsets and / or a coarse carrier
 * estimate per loop, on the same kernels (qpsk_ctx_last_kernel() names them as for qpsk_rx_batch).  Per frame this is, bit for bit,
 * the reference with a fresh process:
 *       rx_frame(frame)            with index = d_index_in[f] at qpsk.c:190
 *       set_phase(seed[f][0]); set_frequency(seed[f][1]);      (costas_loop.c:117-132: phase_wrap, then the [min_freq, max_freq] clamp)
 *       rx_frame(zeros)
 * results taken after the second call as qpsk_rx_batch() takes them.
 *
 *   frame_pitch  samples between frames as qpsk_rx_batch_pitched() (0 = frame_size)
 *   d_index_in   [nframes] int32 decimation offsets 0..7 (the range fixed_index accepts; with CYCLES = 4, offsets 4..7 pick past the
 *                block, read as 0 as the fixed mode does) -- every timing estimate is skipped, the in-launch FFT estimate included.
 *                NULL = the context's timing mode, exactly as qpsk_rx_batch_pitched() computes it.  An offset outside 0..7 is not read
 *                as an address (the frame is demodulated at 0) and the context's NEXT SYNCHRONISING call returns QPSK_ERR_ARG
 *   d_seed       [nframes][2] float (phase, freq) the loop starts from; NULL = (0, 0).  A non-finite seed or a phase beyond the
 *                bounded 2 pi wrap fails like a non-finite input: QPSK_ERR_RANGE at the next synchronisation
 *   outputs      as qpsk_rx_batch(); d_index receives the offsets used (d_index may be d_index_in)
 * Both NULL: the results of qpsk_rx_batch_pitched().  Ext calls neither read nor update the histogram mode's one-pass guess (with
 * d_index_in NULL in QPSK_TIMING_HIST the batch takes the two-launch route).  A caller that estimates offsets once
 * (qpsk_timing_fft_batch, qpsk_timing_scan_batch, or its own estimator) and reuses them for later batches pays for no estimate there.
 * ------------------------------------------------------------------------- */
int qpsk_rx_batch_ext(qpsk_ctx *ctx, const float *d_in, long long frame_pitch, int nframes, const int32_t *d_index_in,
                      const float *d_seed, uint8_t *d_sym, float *d_freq, float *d_phase, float *d_costas, int32_t *d_index,
                      float *d_hz);
/* -------------------------------------------------------------------------
 * DATA: the same batch with the transmitter's dibits as an output.  d_sym is the reference's slicer bit for bit, and the reference's
 * loop parks the constellation on the diagonals, which qpsk_demod() turns another 45 degrees onto its own decision boundaries: d_sym
 * is half noise by construction.  d_data takes the decision the loop's constellation supports.  Per symbol i, with
 * z = costas_frame[i] exactly as qpsk.c:197 forms it:
 *       bits[0] = z.re < 0.0f;  bits[1] = z.im < 0.0f;  d_data = (bits[1] << 1) | bits[0]
 * i.e. qpsk_demod() WITHOUT its ROT45 step.  At the loop's rotation 0 this is the dibit qpsk_tx_symbols() sent (qpsk.c:58-63:
 * 1 -> 0, j -> 1, -j -> 2, -1 -> 3); the loop may settle on any of four quarter turns, which qpsk_sync_batch() resolves.  The "< 0.0f"
 * test does not see the sign of a zero, so every kernel route gives the same bits.
 *
 *   every argument it shares with qpsk_rx_batch_ext: the same meaning, the same error contract (the histogram mode's guess left alone)
 *   d_data   [nframes][nsym] uint8, required
 *   d_sym    [nframes][nsym] uint8 or NULL: the slicer's decisions as well
 * Every output other than d_data is bit for bit what qpsk_rx_batch_ext() returns for the same arguments.  With d_sym NULL the batch runs
 * on rx_lean_kernel wherever qpsk_rx_batch_ext() would (qpsk_ctx_last_kernel() says so), at the same speed; other shapes, and d_sym
 * requested as well, dump costas_frame[] into a context buffer (8 bytes per symbol) and take the rule from it.
 * ------------------------------------------------------------------------- */
int qpsk_rx_batch_data(qpsk_ctx *ctx, const float *d_in, long long frame_pitch, int nframes, const int32_t *d_index_in,
                       const float *d_seed, uint8_t *d_data, uint8_t *d_sym, float *d_freq, float *d_phase, int32_t *d_index,
                       float *d_hz);

/* -------------------------------------------------------------------------
 * SYNC: a caller's sync word places the payload in each row of data decisions and resolves the loop's quarter-turn ambiguity.
 * ring = {0, 1, 3, 2} is a dibit's place on the circle in quarter turns (its own inverse); only the low two bits of d_data are read.
 * For every lag L in [lag_min, lag_max] and rotation r in 0..3:
 *       score(L, r) = #{ i < nsync : ring[(ring[data[L+i]] - r) & 3] == sync[i] }
 * (L*, r*) has the largest score; ties go to the smallest L, then the smallest r.  Per frame f:
 *       d_out[f][i] = ring[(ring[data[L*+nsync+i]] - r*) & 3], i < nout      (the payload de-rotated into the transmitter's dibits)
 *       d_lag[f] = L*,  d_rot[f] = r*,  d_score[f] = score(L*, r*)
 *
 *   d_data       [nframes][nsym] uint8 (qpsk_rx_batch_data's d_data; nsym is the row length)
 *   h_sync       [nsync] dibits 0..3 on the host, 1 <= nsync <= 128: it travels in the kernel arguments, so it may be freed on return
 *   lag window   0 <= lag_min <= lag_max, lag_max + nsync + nout <= nsym (a window as large as the whole row works)
 *   outputs      d_out [nframes][nout] uint8 (must not overlap d_data), d_lag, d_rot, d_score [nframes] int32; each may be NULL, not all
 * QPSK_ERR_ARG at the call for a bad argument.  A sync word equal to one of its own rotations -- as a rotated, shifted copy of itself,
 * e.g. a periodic word -- cannot resolve the ambiguity: the tie rule then picks the smallest lag and rotation.  The call does not check
 * for this; choose a word whose rotations match it poorly at every shift.  Stream-ordered.
 * ------------------------------------------------------------------------- */
int qpsk_sync_batch(qpsk_ctx *ctx, const uint8_t *d_data, int nframes, int nsym, const uint8_t *h_sync, int nsync, int lag_min,
                    int lag_max, int nout, uint8_t *d_out, int32_t *d_lag, int32_t *d_rot, int32_t *d_score);

/* -------------------------------------------------------------------------
 * DEFRAMER: packets out of continuous streams of data decisions -- the stream calls' costas_frame[] block after block, or any rows
 * of dibits.  One state per stream, independent of the receive streams' state.  For one stream let D be the concatenation of every
 * row pushed since the reset, d[i] = ring[D[i] & 3] (ring as in SYNC), n = nsync and N = 4 (nbytes + 2).  Then, from h = 0:
 *       score(p, r) = #{ i < n : (d[p+i] - ring[sync[i]]) & 3 == r }                 (qpsk_sync_batch's score)
 *       p* = the smallest p >= h with p + n <= len(D) and max_r score(p, r) >= min_score;  r* = the smallest r attaining the max
 *       the packet is complete once p* + n + N <= len(D), and reported by the push during which that happens:
 *       u[i] = ring[(d[p*+n+i] - r*) & 3] ^ keystream[i], i < N    (de-rotated, then descrambled as qpsk_scramble_batch: SEED reloaded at
 *                                                                   the payload's first dibit)
 *       b[k] = u[4k] | u[4k+1] << 2 | u[4k+2] << 4 | u[4k+3] << 6  (qpsk_pack_symbols' packing)
 *       crc_ok = crc16(b[0 .. nbytes-1]) == b[nbytes] << 8 | b[nbytes+1]
 *       h = p* + n + N                                             (hunting resumes behind the packet, CRC pass or fail)
 * The result depends only on D, not on how it is cut into pushes (apart from which push reports a packet).
 *
 * qpsk_deframer_reset: 1 <= nsync <= 128 dibits h_sync on the host (copied: it may be freed on return), 1 <= min_score <= nsync,
 *   1 <= nbytes <= 1024, 1 <= max_packets <= 64.  Allocates and zeroes every stream's state; a second reset replaces everything.
 * qpsk_deframer_push: exactly one input -- d_costas [nstreams][nsym][2] float (the stream calls' d_costas; qpsk_rx_batch_data's data
 *   rule is applied on load) or d_data [nstreams][nsym] uint8 (only the low two bits are read); 1 <= nsym <= 2^21, any size per push.
 *   Per stream s, the packets completed in this push:
 *       d_count  [nstreams] int32             how many (the true number, also beyond max_packets)    -- required
 *       d_bytes  [nstreams][max_packets][nbytes + 2] uint8   the payload and the received CRC        -- each of these may be NULL;
 *       d_pos    [nstreams][max_packets] int64               p*, counted from the reset                 only the first min(count,
 *       d_rot, d_score [nstreams][max_packets] int32          r*, score(p*, r*)                          max_packets) rows of a stream
 *       d_crc_ok [nstreams][max_packets] uint8                                                           are written
 * QPSK_ERR_ARG at the call for a bad argument (no input or both, an input overlapping an output); QPSK_ERR_STATE for a push before a
 * reset.  Stream-ordered on the context's stream; touches neither the receive streams nor the batch paths.  A push that fails after
 * it enqueued work leaves the deframer's state undefined: later pushes return QPSK_ERR_STATE until a reset has succeeded.
 * ------------------------------------------------------------------------- */
int qpsk_deframer_reset(qpsk_ctx *ctx, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets);
int qpsk_deframer_push(qpsk_ctx *ctx, const float *d_costas, const uint8_t *d_data, int nsym, int32_t *d_count, uint8_t *d_bytes,
                       long long *d_pos, int32_t *d_rot, int32_t *d_score, uint8_t *d_crc_ok);

/* -------------------------------------------------------------------------
 * CODED DEFRAMER: the same hunt on streams whose packets carry the K = 7 rate-1/2 code (CONVOLUTIONAL CODE below).  On air:
 *       [sync: n = nsync dibits, uncoded][body: Nc = 8 (nbytes + 2) + 6 dibits]
 *       body = keystream (qpsk_scramble_batch's, SEED reloaded at the body's first dibit) xor
 *              qpsk_conv_encode_batch(payload ++ crc16 big-endian, QPSK_CONV_TAIL)          (the bytes' bits low bit first)
 * The library's own definition (the reference has no FEC; parity unpinned), restated in numpy by
 * tests/test_deframe_coded_cpu.py.  A context holds ONE deframer, in one mode: either reset replaces the other's state, and a push of
 * the other kind returns QPSK_ERR_STATE, as a push before any reset does.  Per stream, with D, d, score, p*, r* exactly as DEFRAMER
 * defines them on the data rule of the pushed costas_frame[]:
 *       HUNT    identical with N replaced by Nc: a packet is complete once p* + n + Nc <= len(D), reported by the push during which that
 *               happens, and h = p* + n + Nc, CRC pass or fail.  The hunt never depends on the decoder's result.
 *       SOFT    body symbol i is z = costas at stream position p* + n + i; g = the gain of the push during which that symbol arrived;
 *               (u, v) = z (-j)^r* and q(x) exactly as qpsk_soft_batch defines them with that g;  s[i] = (q(u), q(v))
 *       GAIN    one float per stream and push: d_gain [nstreams] when given (a caller's AGC, or one value held over blocks); with
 *               d_gain NULL the gain qpsk_soft_batch defines for this push's row with skip = 0 and the reset's mode / scale (the same
 *               sums in the same order).  With a constant d_gain the result depends only on D, not on the cuts (apart from which push
 *               reports a packet); with per-push gains each symbol takes the gain of the push that brought it.
 *       DECODE  qpsk_viterbi_batch's decoder on s[0 .. Nc-1] with d_flip = the keystream dibits and flags 0;  b[k] = byte k of its
 *               d_bits, k < nbytes + 2;  crc_ok = crc16(b[0 .. nbytes-1]) == b[nbytes] << 8 | b[nbytes+1]
 *
 * qpsk_deframer_reset_coded: nsync, min_score, nbytes, max_packets as qpsk_deframer_reset; mode, scale as qpsk_soft_batch (checked
 *   also where d_gain makes them unused).
 * qpsk_deframer_push_coded: d_costas [nstreams][nsym][2] float, 8-byte aligned (soft values need amplitudes: there is no d_data form);
 *   1 <= nsym <= 2^21; d_gain [nstreams] float or NULL.  Outputs shaped and ruled as qpsk_deframer_push's -- d_count required and the
 *   true number, only the first min(count, max_packets) rows of a stream written, packets beyond max_packets counted and not decoded --
 *   plus
 *       d_info   [nstreams][max_packets][4] int32   the decoder's four info words (path metric, end state, start state, channel bit errors)
 *   Every output other than d_count may be NULL.
 * QPSK_ERR_ARG at the call for a bad argument, nothing launched.  A NaN / Inf among the body symbols of a decoded packet, in the summed
 * row (d_gain NULL) or in d_gain gives QPSK_ERR_RANGE at the next synchronisation, as qpsk_soft_batch.  The staging rows and the
 * decoder's scratch grow on demand: a failed allocation returns QPSK_ERR_ALLOC, launches nothing and leaves the context and the
 * deframer usable.  Stream-ordered; touches neither the receive streams, the histogram mode's guess nor the batch paths.
 * qpsk_ctx_last_kernel() names the kernels and the decoder's route (decision words in LDS or in the scratch buffer, by
 * qpsk_viterbi_batch's rule on the rows a push can complete).  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_deframer_reset_coded(qpsk_ctx *ctx, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes,
                              int max_packets, int mode, float scale);
int qpsk_deframer_push_coded(qpsk_ctx *ctx, const float *d_costas, int nsym, const float *d_gain, int32_t *d_count,
                             uint8_t *d_bytes, long long *d_pos, int32_t *d_rot, int32_t *d_score, uint8_t *d_crc_ok,
                             int32_t *d_info);

/* The coded deframer behind a puncturing pattern (PUNCTURING below).  On air:
 *       [sync: n dibits, uncoded][body: Nc = ntx(8 (nbytes + 2) + 6) dibits]
 *       body = keystream xor qpsk_conv_encode_punct_batch(payload ++ crc16 big-endian, QPSK_CONV_TAIL, pattern)
 * HUNT, SOFT and GAIN are exactly CODED DEFRAMER's with this Nc.  DECODE is qpsk_viterbi_punct_batch's decoder on the Nc staged dibits
 * with nsteps = 8 (nbytes + 2) + 6, d_flip = the keystream dibits (over the transmitted dibits) and flags 0.  The pattern lives in the
 * deframer's state: qpsk_deframer_push_coded is the push of both resets, unchanged.  qpsk_deframer_reset_coded is the pattern (1, 1, 1)
 * and the two agree bit for bit.  Arguments and errors as qpsk_deframer_reset_coded; a bad pattern gives QPSK_ERR_ARG and resets
 * nothing.  qpsk_ctx_last_kernel() names deframe_coded_decode_punct_kernel<lds> or <global> after a push.  Restated in numpy by
 * tests/test_punct_cpu.py (deframe_coded_punct_ref). */
int qpsk_deframer_reset_coded_punct(qpsk_ctx *ctx, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes,
                                    int max_packets, int mode, float scale, int period, uint32_t keep0, uint32_t keep1);

/* qpsk_rx_batch_bw() the same way: d_seed [nframes][nbw][2] (one seed per loop) or NULL; d_index_in [nframes] or NULL */
int qpsk_rx_batch_bw_ext(qpsk_ctx *ctx, const float *d_in, int nframes, const float *h_loop_bw, int nbw, const int32_t *d_index_in,
                         const float *d_seed, uint8_t *d_sym, float *d_freq, float *d_phase, int32_t *d_index);

/* -------------------------------------------------------------------------
 * A coarse carrier estimate per frame, in the form the ext calls take as a seed: the Costas loop (costas_loop.c) matched bit for bit
 * only pulls in small offsets within a frame; a Doppler offset beyond its pull-in range is acquired by seeding the loop's frequency.
 * Per frame x, with the context's taps, CYCLES = C and loop clamp [min_freq, max_freq] (qpsk_ctx_set_loop):
 *   y  = rrc_fir() of x[0 .. start+n-1] with a fresh delay line          (bit for bit qpsk_rrc_fir_batch)
 *   z[m] = y[start+m]^4 in fp64, m < n: with a = y.re, b = y.im: s = (a*a - b*b, 2.0*(a*b)), z = (s.re*s.re - s.im*s.im, 2.0*(s.re*s.im))
 *   X  = fftn(z, n)                                                       (fft.c:110-120; bit for bit qpsk_fft_batch)
 *   S  = { integer k : |k| < n / (2 C), min_freq <= w(k) <= max_freq },  w(k) = (float)(TAU * (double)(k*C) / (double)(4*n)) rad/symbol
 *   k* = the k in S with the largest X.re*X.re + X.im*X.im of X[k mod n] (fp64); ties: the smallest |k|, then the smaller k
 * A signal rotating as e^{+j 2 pi df t} gives w(k*) ~ +2 pi df / RS (the sign of get_frequency()).  RANGE: |df| < RS / 8 (+-300 Hz at
 * 2400 baud): S is limited to |w| < pi / 4 because y^4 also carries symbol-rate sidebands at 4 df +- RS, which an offset inside the range
 * never puts into S.  RESOLUTION: one bin = 2 pi C / (4 n) rad/symbol (0.0123 at C = 8, n = 1024).  No phase estimate: the seed's
 * phase is 0.  The definition has no counterpart in the reference beyond the filter and the transform (parity unpinned).
 *
 *   frame_pitch  as qpsk_rx_batch_ext (0 = frame_size; otherwise even and >= frame_size)
 *   start, n     the window: start >= 0, n a power of two in 64..8192, start + n <= frame_size
 *   d_seed       [nframes][2] float (0, w(k*)): pass it unchanged to qpsk_rx_batch_ext as d_seed
 *   d_freq       [nframes] float w(k*);  d_bin [nframes] int32 k*;  d_line [nframes][2] double X[k*]
 * Each output may be NULL, not all.  QPSK_ERR_ARG at the call for a bad argument or an empty S; a NaN / Inf sample the estimate reads
 * (x[max(0, start-126) .. start+n-1]) gives QPSK_ERR_RANGE at the next synchronisation.  Stream-ordered; qpsk_ctx_last_kernel() names
 * the kernel; the histogram mode's one-pass guess is neither read nor updated.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_carrier_est_batch(qpsk_ctx *ctx, const float *d_in, long long frame_pitch, int nframes, int start, int n,
                           float *d_seed, float *d_freq, int32_t *d_bin, double *d_line);

/* -------------------------------------------------------------------------
 * SOFT DECISIONS AND SIGNAL QUALITY per row of costas_frame[] (what qpsk_rx_batch* with d_costas, qpsk_streams_rx_* and
 * qpsk_costas_batch write).  The reference has no counterpart: this is the library's own definition (parity unpinned),
 * restated in numpy by tests/test_soft_cpu.py.  Per symbol z = (a, b) of a row.
 *
 * SUMS.  IEEE fp64 on the float inputs widened to double, nothing fused, over the symbols skip <= i < nsym; k = i - skip, m = nsym - skip:
 *       p = a*a + b*b;   s = (a*a - b*b, 2.0*(a*b))                                  (qpsk_carrier_est_batch's squaring)
 *       t1 = |a| + |b|;  t2 = p;  t4 = p*p;  tq = s.re*s.re - s.im*s.im              ( = Re z^4 )
 * The ORDER of summation is part of the definition.  There are 256 partial sums P[l], l = k mod 256; each starts from +0.0 and takes
 * its terms in increasing k.  They are folded: for h = 128, 64, ..., 1: P[l] += P[l+h] for every l < h.  S1, S2, S4, SQ are the four P[0].
 *
 * QUALITY, d_quality [nrows][4] float, each figure computed in fp64 and rounded once:
 *       M2 = S2/m;  M4 = S4/m;  D = 2*M2*M2 - M4;  Ps = D > 0 ? sqrt(D) : 0;  Pn = M2 - Ps
 *                                                     (the M2M4 estimator: a constant-modulus signal in Gaussian noise)
 *       [0] amp  = S1 / (2m)                 mean |component|: where the loop parks the constellation on each axis
 *       [1] snr  = Pn > 0 ? Ps / Pn : 0      Es/N0 as a ratio (dB is left to the caller: a device log10 would not be bit-exact)
 *       [2] lock = S4 > 0 ? -SQ / S4 : 0     +1: locked on the diagonals (z^4 = -|z|^4); ~0: noise, or a carrier the loop does not follow
 *       [3] nvar = max(Pn, 0) / 2            noise variance per component
 * d_sums [nrows][4] double receives S1, S2, S4, SQ, for callers that average over rows or blocks themselves.
 *
 * SOFT DECISIONS, d_soft [nrows][nout][2] int8.  The gain g is one float per row, always finite; amp_d is the fp64 S1 / (2m):
 *       QPSK_SOFT_UNIT   g = amp_d > 0 ? (float)min((double)scale / amp_d, FLT_MAX) : 0
 *                        the constellation lands at +-scale whatever the input level (scale = 64 leaves headroom)
 *       QPSK_SOFT_LLR    g = Pn > 0 ? (float)min(2.0*sqrt(Ps/2) / (Pn/2) / (double)scale, FLT_MAX) : the UNIT rule with 127 for scale
 *                        the output is the bit's log-likelihood ratio in steps of scale
 *       d_gain_in [nrows] float, when not NULL, replaces both: the caller's own gain (e.g. one held over several blocks of a stream)
 * The payload is placed per row by lag[row] + first: d_lag and d_rot are qpsk_sync_batch's outputs, first is its nsync; d_lag NULL
 * means 0 and d_rot NULL means 0.  For i < nout, with z = row[lag + first + i] and r = rot & 3:
 *       (u, v) = z * (-j)^r:   r=0 (a, b)   r=1 (b, -a)   r=2 (-a, -b)   r=3 (-b, a)          (swaps and sign flips: exact)
 *       q(x)   = (int8) min(127, max(-127, rintf(x * g)))                                      (fp32 multiply, round half to even)
 *       d_soft[row][i][0] = q(u)  (bit 0 of the dibit)     d_soft[row][i][1] = q(v)  (bit 1)     positive <=> the bit is 0
 * Wherever q != 0, (q < 0) is the corresponding bit of qpsk_sync_batch's de-rotated d_out; at an exact zero component q is 0.
 *
 *   d_costas     [nrows][nsym] complex float, rows row_pitch symbols apart (0 = nsym; otherwise >= nsym), 8-byte aligned;
 *                1 <= nsym <= 2^21; what lies between the rows is never read
 *   skip         0 .. nsym-1: leaves the loop's acquisition transient out of the sums
 *   mode, scale  QPSK_SOFT_UNIT / QPSK_SOFT_LLR; scale finite and > 0 (checked also where d_gain_in makes them unused)
 *   first, nout  first >= 0, nout >= 0, first + nout <= nsym; ignored when d_soft is NULL
 *   outputs      d_soft (2-byte aligned, must not overlap the input), d_quality, d_sums: each may be NULL, not all.  With d_gain_in and
 *                neither d_quality nor d_sums nothing is summed and only the payload is read
 * QPSK_ERR_ARG at the call for a bad argument.  A device-side lag with lag < 0 or lag + first + nout > nsym is never used as an address:
 * that row's soft output is zeros and the context's next synchronising call returns QPSK_ERR_ARG.  A NaN / Inf sample among those a
 * row's sums (skip <= i < nsym, when anything is summed) or soft output (the payload) use, or a NaN / Inf entry of d_gain_in, gives
 * QPSK_ERR_RANGE at the next synchronisation.  Stream-ordered on the context's stream; neither reads nor updates the histogram mode's
 * guess, the receive streams or the deframer; qpsk_ctx_last_kernel() names the kernel: rows of up to 4096 symbols are read once
 * (soft_onepass_kernel), longer ones twice (sums, then soft).  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
enum { QPSK_SOFT_UNIT = 0, QPSK_SOFT_LLR = 1 };
int qpsk_soft_batch(qpsk_ctx *ctx, const float *d_costas, long long row_pitch, int nrows, int nsym, int skip, int mode, float scale,
                    const float *d_gain_in, const int32_t *d_lag, const int32_t *d_rot, int first, int nout, int8_t *d_soft,
                    float *d_quality, double *d_sums);

/* -------------------------------------------------------------------------
 * CONVOLUTIONAL CODE AND VITERBI DECODER: constraint length 7, rate 1/2, generators 171 / 133 octal, on the int8 soft decisions
 * qpsk_soft_batch writes.  One QPSK symbol carries the two coded bits of one trellis step, so d_soft[row][t][0..1] is step t's input as
 * it lies in memory.  The reference has no FEC: this is the library's own definition (parity unpinned), restated in
 * numpy by tests/test_viterbi_cpu.py.  Everything is integer arithmetic; there is no tolerance anywhere.
 *
 * CODE.  Register r of 7 bits, r = ((r << 1) | bit) & 127 (newest bit in bit 0), starting from 0.  Per input bit the coded pair is
 *       c0 = parity(r & 0x79)   c1 = parity(r & 0x5B)          (171, 133 octal; neither output inverted)
 * sent as the dibit c0 | c1 << 1: c0 rides on bit 0 of the dibit (the real axis, d_soft[..][0]), c1 on bit 1.  The state is r & 63.
 * QPSK_CONV_TAIL appends six zero bits: nsteps = nbits + 6; without it nsteps = nbits.
 *
 * DECODER.  Input per step t: (s0, s1) = d_soft[row][t][0..1], int8, positive <=> the bit is 0; 0 is an erasure and needs no special
 * case.  A -128 is taken as -127 before anything else.  If d_flip is given ([nsteps] uint8, one array for all rows), bit j of d_flip[t]
 * negates s_j first: this undoes an additive scrambler (qpsk_scramble_batch's keystream dibits) on soft values.
 *   branch metric of a transition into register value r:   bm(r) = (c0(r) ? -s0 : s0) + (c1(r) ? -s1 : s1)      (the decoder maximises)
 *   path metrics pm[64], int32.  Start: pm[0] = 0, every other state NEG = -2^30; with QPSK_VITERBI_OPEN_START all 64 start at 0
 *   step, for every new state ns (input bit ns & 1):  p0 = ns >> 1,  p1 = p0 | 32,
 *       m0 = pm[p0] + bm(ns);  m1 = pm[p1] + bm(ns | 64);  d[t][ns] = (m1 > m0)  (A TIE KEEPS p0);  pm'[ns] = d ? m1 : m0
 *       No normalisation: with nsteps <= 131072, |metric| <= 254 * 131072 < 2^26, and NEG plus that stays below every reachable metric
 *   end: state 0; with QPSK_VITERBI_OPEN_END the state of the largest pm, TIES TO THE LOWEST STATE NUMBER
 *   trace-back over the WHOLE row (no truncation window): from the end state st, for t = nsteps-1 .. 0:
 *       bit[t] = st & 1;   st = (st >> 1) | (d[t][st] << 5)
 *   d_bits [nrows][ceil(nsteps/8)] uint8: bit t in byte t >> 3 at position t & 7 (low bits first, the packing of qpsk_pack_symbols;
 *       tail bits included, padding bits 0)
 *   d_info [nrows][4] int32 = { the end state's path metric, the end state, the state the trace-back arrives at (0 unless open start),
 *       the number of non-zero soft values whose sign disagrees with the re-encoded path: a channel bit-error count for free }
 * Decisions of states that no path from the start reaches do not influence any output.  (Every state is reachable from every state in
 * six steps, hence max(pm) - min(pm) over reachable states <= 12 * 254 = 3048 at every step, and any finite start penalty > 3048 gives
 * the same outputs as NEG.)
 *
 *   qpsk_conv_encode_batch   d_bits [nrows][ceil(nbits/8)] packed as above -> d_dibits [nrows][nsteps] uint8, ready for
 *                qpsk_scramble_batch and qpsk_tx_symbols; nrows >= 1, 1 <= nbits, nsteps <= 131072; flags 0 or QPSK_CONV_TAIL
 *   qpsk_viterbi_batch       d_soft rows row_pitch steps apart (0 = nsteps; otherwise >= nsteps; what lies between rows is never read),
 *                2-byte aligned; 1 <= nsteps <= 131072; nrows >= 1; d_flip may be NULL; d_bits or d_info may be NULL, not both
 * QPSK_ERR_ARG at the call for a bad argument, nothing launched.  Stream-ordered on the context's stream like qpsk_soft_batch; neither
 * reads nor updates the histogram mode's guess, the receive streams or the deframer.  qpsk_ctx_last_kernel() names the kernel: the
 * decision words of a row (8 bytes per step) wait for the trace-back in LDS (viterbi_lds_kernel: rows of up to 8192 steps, where every
 * row of the call is resident at once) or in a per-context scratch buffer that grows on demand (viterbi_kernel; a failed allocation
 * returns QPSK_ERR_ALLOC and leaves the context usable).  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
enum { QPSK_CONV_TAIL = 1 };
enum { QPSK_VITERBI_OPEN_START = 1, QPSK_VITERBI_OPEN_END = 2 };
int qpsk_conv_encode_batch(qpsk_ctx *ctx, const uint8_t *d_bits, int nrows, int nbits, int flags, uint8_t *d_dibits);
int qpsk_viterbi_batch(qpsk_ctx *ctx, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, const uint8_t *d_flip,
                       int flags, uint8_t *d_bits, int32_t *d_info);

/* -------------------------------------------------------------------------
 * PUNCTURING: the rates 2/3, 3/4, 5/6, 7/8 (and any other pattern of period <= 32) of the code above, by not sending some of the coded
 * bits.  The library's own definition, integers only (the reference has no FEC; parity unpinned), restated in numpy by
 * tests/test_punct_cpu.py.
 *
 * PATTERN (period, keep0, keep1): 1 <= period <= 32; keep0, keep1 uint32 with no bit set at or above period and keep0 | keep1 != 0.
 *   Coded bit j (0 is c0, 1 is c1) of trellis step t is SENT iff bit r = t mod period of keep_j is set.  K = popc(keep0) + popc(keep1).
 *   A period position where neither bit is sent is legal.
 * NUMBERING of the sent bits, in the order (t, j).  With low(r) = (1u << r) - 1:
 *       idx(t, 0) = (t / period) K + popc(keep0 & low(r)) + popc(keep1 & low(r))
 *       idx(t, 1) = idx(t, 0) + ((keep0 >> r) & 1)
 *       nsent(nsteps) = idx(nsteps, 0)            ntx(nsteps) = ceil(nsent / 2) dibits
 * PACKING.  Sent bit k rides on bit k & 1 of transmitted dibit k >> 1.  When nsent is odd, bit 1 of the last dibit is a pad bit: the
 *   encoder sends 0, the receiver never reads its soft value.  This serial packing IS the definition: the mapping of the sent bits
 *   onto I and Q that DVB-S prescribes for its punctured rates is NOT reproduced.
 * NAMED PATTERNS, as macros that expand to the three arguments; bit r of a mask is step r of the period.  They are the usual X / Y
 *   patterns for 171 / 133 (X 10, Y 11; X 101, Y 110; X 10101, Y 11010; X 1000101, Y 1111010).
 * DECODER INPUT.  v(k) = flat int8 number k of the row = d_soft[row][k >> 1][k & 1], what qpsk_soft_batch writes for the transmitted
 *   symbols.  -128 is taken as -127; then v(k) is negated iff bit k & 1 of d_flip[k >> 1] is set: d_flip is [ntx] and runs over the
 *   TRANSMITTED dibits, because the scrambler acts on what is on air.  Step t's input is
 *       s_j = sent(t, j) ? v(idx(t, j)) : 0
 *   and everything after that is word for word qpsk_viterbi_batch: start, step, tie rule, end, whole-row trace-back, d_bits and the four
 *   d_info words (the error count ignores zeros, so it counts over the sent bits).  nsteps <= 131072 and the metric bound are unchanged.
 * Hence, and tested:  (1) the punctured call equals qpsk_viterbi_batch with d_flip NULL on the zero-filled row (s_j above, after the
 *   -128 rule and the flip) in d_bits and all four d_info words;  (2) the pattern (1, 1, 1) equals qpsk_viterbi_batch with the same d_flip.
 *
 *   qpsk_punct_ntx                host only, no context: ntx(nsteps), 1 <= nsteps <= 131072, or QPSK_ERR_ARG.  May be 0 when every
 *                step of so short a row is deleted.
 *   qpsk_conv_encode_punct_batch  as qpsk_conv_encode_batch -> d_dibits [nrows][ntx(nsteps)] uint8
 *   qpsk_viterbi_punct_batch      as qpsk_viterbi_batch; d_soft rows row_pitch TRANSMITTED symbols apart (0 = ntx; otherwise >= ntx; what
 *                lies between rows, and the pad value, is never read); d_flip [ntx] or NULL
 * Arguments and errors as the unpunctured twins; a bad pattern gives QPSK_ERR_ARG at the call with nothing launched.  Where the
 * decision words wait (LDS or the scratch buffer) goes by nsteps, as in qpsk_viterbi_batch; qpsk_ctx_last_kernel() names
 * viterbi_punct_lds_kernel, viterbi_punct_kernel or conv_encode_punct_kernel.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
#define QPSK_PUNCT_1_2 1, 0x1u, 0x1u
#define QPSK_PUNCT_2_3 2, 0x1u, 0x3u
#define QPSK_PUNCT_3_4 3, 0x5u, 0x3u
#define QPSK_PUNCT_5_6 5, 0x15u, 0x0Bu
#define QPSK_PUNCT_7_8 7, 0x51u, 0x2Fu
int qpsk_punct_ntx(int nsteps, int period, uint32_t keep0, uint32_t keep1);
int qpsk_conv_encode_punct_batch(qpsk_ctx *ctx, const uint8_t *d_bits, int nrows, int nbits, int flags, int period, uint32_t keep0,
                                 uint32_t keep1, uint8_t *d_dibits);
int qpsk_viterbi_punct_batch(qpsk_ctx *ctx, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, int period, uint32_t keep0,
                             uint32_t keep1, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info);

/* -------------------------------------------------------------------------
 * FRAMER: the transmit twin of the three deframers -- payloads in, rows of on-air dibits out, ready for qpsk_tx_symbols, in one launch.
 * A composition of definitions pinned above (crc16, qpsk_scramble_batch's keystream, qpsk_pack_symbols' packing, CONVOLUTIONAL CODE,
 * PUNCTURING): integers only, no tolerance anywhere.  Restated in numpy by tests/test_frame_cpu.py (frame_ref).
 *
 *       n = nsync;   pkt = payload[0 .. nbytes) ++ (crc >> 8) ++ (crc & 255),  crc = crc16(payload)               (CRC big-endian)
 *       ks[i] = dibit i of qpsk_scramble_batch's keystream from SEED (the keystream of a longer frame extends a shorter one's)
 * BODY, B dibits:
 *       QPSK_FRAME_UNCODED   B = 4 (nbytes + 2);   body[i] = ((pkt[i >> 2] >> 2 (i & 3)) & 3) ^ ks[i]              (bits low first)
 *       QPSK_FRAME_CODED     with the pattern (period, keep0, keep1):   B = qpsk_punct_ntx(8 (nbytes + 2) + 6, pattern);
 *                            body[i] = ks[i] ^ E[i],  E = qpsk_conv_encode_punct_batch(pkt, nbits = 8 (nbytes + 2), QPSK_CONV_TAIL, pattern)
 *                            The keystream runs over the TRANSMITTED dibits; the pad bit of an odd nsent is 0 before the xor.  The pattern
 *                            (1, 1, 1) -- QPSK_PUNCT_1_2 -- is the rate-1/2 format of qpsk_deframer_reset_coded.
 *       Either way the keystream is reloaded at the body's first dibit.
 * PACKET  [h_sync[0 .. n) & 3][body]:  P = n + B dibits -- what qpsk_deframer_push, qpsk_deframer_push_coded and the deframer of
 *       qpsk_deframer_reset_coded_punct receive.
 * ROWS  row r < nrows holds per_row packets, numbers r per_row + j, j < per_row; packet j starts at column lead + j (P + gap).  Every column
 *       i < row_len outside a packet is IDLE FILL ks[i]: scrambled zeros with the keystream started at column 0 of each row -- transitions
 *       for the timing estimate and the loop, and no sync word for a deframer to find (checked for the shapes of tests/test_frame_cpu.py at
 *       min_score = nsync; no guarantee for every word).  Rows lie row_len bytes apart and nothing else is written; every value is 0..3.
 *
 *   qpsk_frame_len     host only, no context: P = nsync + B, or QPSK_ERR_ARG
 *   qpsk_frame_batch
 *       d_payload      [nrows * per_row][nbytes] uint8, rows payload_pitch bytes apart (0 = nbytes; otherwise >= nbytes; what lies between
 *                      rows is never read)
 *       h_sync         [nsync] dibits on the host, taken & 3: it travels in the kernel arguments as in qpsk_sync_batch
 *       coding         QPSK_FRAME_UNCODED (the pattern is ignored) or QPSK_FRAME_CODED (the pattern is checked as
 *                      qpsk_conv_encode_punct_batch checks it)
 *       d_out          [nrows][row_len] uint8, must not overlap d_payload
 *       d_crc          [nrows * per_row] uint16, the CRC sent, or NULL
 *       limits         1 <= nsync <= 128, 1 <= nbytes <= 1024 (the deframers'), nrows >= 1, 1 <= per_row <= 64, nrows * per_row < 2^31,
 *                      lead, gap >= 0, lead + per_row P + (per_row - 1) gap <= row_len <= 2^21
 * QPSK_ERR_ARG at the call for a bad argument, nothing launched.  The call keeps a keystream table of max(row_len, B) dibits of its own
 * per context, which only grows: when it cannot, QPSK_ERR_ALLOC, nothing launched, the context usable.  Stream-ordered on the context's
 * stream; neither reads nor updates the receive streams, the transmitters, the deframer, the histogram mode's guess or
 * qpsk_scramble_batch's cached keystream.  qpsk_ctx_last_kernel() names frame_kernel<uncoded> or frame_kernel<coded>.  Not built: a
 * streaming framer with state across calls, qpsk_multi, host-pointer payloads; interleaving is qpsk_frame_batch_ilv (INTERLEAVING below).  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
enum { QPSK_FRAME_UNCODED = 0, QPSK_FRAME_CODED = 1 };
int qpsk_frame_len(int nsync, int nbytes, int coding, int period, uint32_t keep0, uint32_t keep1);
int qpsk_frame_batch(qpsk_ctx *ctx, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                     const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, int lead, int gap,
                     int row_len, uint8_t *d_out, uint16_t *d_crc);

/* -------------------------------------------------------------------------
 * INTERLEAVING: the coded bits of a body spread over the body on air, so that a burst of bad symbols -- a fade, an interferer, a Costas
 * loop that slips a quarter turn for a few symbols -- meets the decoder as isolated errors instead of a run, which a convolutional code
 * does not survive.  The library's own definition, integers only (parity unpinned like PUNCTURING), restated in numpy
 * by tests/test_ilv_cpu.py.  Everything is stated on PUNCTURING's terms idx(t, j), nsent, ntx; rate 1/2 is the pattern QPSK_PUNCT_1_2.
 * (qpsk_interleave_batch below is the reference's byte interleaver and another thing: packed bytes, a prime table that ends at 347 bits.)
 *
 * DOMAIN.  n = 2 ntx(nsteps) bits: the transmitted body's bits, the pad bit of an odd nsent included.
 * STRIDE.  stride = s with 1 <= s < max(n, 2) and gcd(s, n) = 1.  n is even, so s is odd.  s = 1 is the identity.
 * PERMUTATION.  pi(k) = (k s) mod n for k in 0 .. n-1, the product formed in 64 bits (n reaches 2^18).  A bijection, since gcd(s, n) = 1.
 * ENCODER.  On-air bit pi(k) is sent bit k, for k < nsent.  When nsent is odd, on-air bit pi(nsent) is the pad, 0.  On-air dibit
 *   i = air[2 i] | air[2 i + 1] << 1.  A scrambler then acts on the on-air dibits exactly as before.
 * DECODER INPUT.  v(a) = flat int8 number a of the transmitted row after the -128 rule, negated iff bit a & 1 of d_flip[a >> 1] is set: d_flip
 *   still runs over the transmitted dibits.  Step t's input is
 *       s_j = sent(t, j) ? v(pi(idx(t, j))) : 0
 *   and everything after that is word for word qpsk_viterbi_batch.  The pad position is never read.
 * Hence, and tested:  (1) the interleaved call equals qpsk_viterbi_punct_batch on the row gathered on the host, row'[k] = row[pi(k)], with
 *   the flip bits gathered the same way, in d_bits and all four d_info words;  (2) stride 1 equals the punctured twin bit for bit, in every
 *   call below.
 * BURSTS.  On-air bits a and a + d carry coded bits that lie d s^-1 mod n apart; adjacent coded bits lie s apart on air.  A stride near
 *   n / 16, qpsk_ilv_stride(n, n / 16), is a starting point, not a claim of optimality.
 *
 *   qpsk_ilv_stride                host only, no context: the smallest s >= min(want, nbits - 1) with gcd(s, nbits) = 1 (the search ends by
 *                nbits - 1); nbits >= 2 and want >= 1, or QPSK_ERR_ARG
 *   qpsk_conv_encode_ilv_batch     as qpsk_conv_encode_punct_batch -> d_dibits [nrows][ntx] on-air dibits
 *   qpsk_viterbi_ilv_batch         as qpsk_viterbi_punct_batch in arguments, limits, row_pitch, where the decision words wait and the chunks
 *   qpsk_frame_batch_ilv           qpsk_frame_batch with the stride, honoured for QPSK_FRAME_CODED (E above is then
 *                qpsk_conv_encode_ilv_batch's output); with QPSK_FRAME_UNCODED a stride other than 1 is QPSK_ERR_ARG.  qpsk_frame_len is
 *                unchanged: the length does not change
 *   qpsk_deframer_reset_coded_ilv  qpsk_deframer_reset_coded_punct with the stride, kept in the deframer's state; qpsk_deframer_push_coded
 *                stays the one push of all coded resets.  A bad stride resets nothing: the deframer stays as it was
 * A bad stride (0, negative, even with n > 2, >= n, not coprime to n), or ntx = 0, gives QPSK_ERR_ARG at the call with nothing launched.
 * qpsk_ctx_last_kernel() names conv_encode_ilv_kernel, viterbi_ilv_lds_kernel / viterbi_ilv_kernel, frame_kernel<coded,ilv> (stride 1 takes
 * frame_kernel<coded>) and deframe_coded_decode_ilv_kernel<lds> / <global>.  Not built: interleaving for the uncoded format, for qpsk_multi,
 * or across packets.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_ilv_stride(int nbits, int want);
int qpsk_conv_encode_ilv_batch(qpsk_ctx *ctx, const uint8_t *d_bits, int nrows, int nbits, int flags, int period, uint32_t keep0,
                               uint32_t keep1, int stride, uint8_t *d_dibits);
int qpsk_viterbi_ilv_batch(qpsk_ctx *ctx, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, int period, uint32_t keep0,
                           uint32_t keep1, int stride, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info);
int qpsk_frame_batch_ilv(qpsk_ctx *ctx, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                         const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, int stride, int lead,
                         int gap, int row_len, uint8_t *d_out, uint16_t *d_crc);
int qpsk_deframer_reset_coded_ilv(qpsk_ctx *ctx, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes,
                                  int max_packets, int mode, float scale, int period, uint32_t keep0, uint32_t keep1, int stride);

/* -------------------------------------------------------------------------
 * REED-SOLOMON: a byte-oriented outer code behind the convolutional code.  A Viterbi decoder that loses the path emits a run of wrong
 * bytes; the outer code repairs up to nroots / 2 wrong bytes per codeword wherever they lie, or up to nroots bytes whose places are known
 * (erasures), and says so per codeword when it cannot.  The library's own definition, integers only (the reference has no FEC; parity
 * unpinned), restated in numpy by tests/test_rs_cpu.py and pinned there to a codebook decoder that enumerates every
 * codeword of four small codes.  There is no tolerance anywhere.
 *
 * FIELD.  GF(256) modulo x^8 + x^4 + x^3 + x^2 + 1 (0x11D), alpha = 0x02.  Addition is xor.
 * CODE (n, k), nroots = n - k:  1 <= k, 1 <= nroots <= 64, n <= 255.  A code shorter than 255 is the shortened code: the missing leading
 *   bytes are zeros that are neither stored nor sent.
 *       g(x) = prod_{i = 0}^{nroots - 1} (x - alpha^i)                                   (the first root is alpha^0)
 *   With (204, 188) these are the field and generator polynomials ETSI EN 300 421 names for its outer code; conformity is by construction
 *   (no outside test vector is pinned).
 * ROW.  A codeword is n bytes, c(x) = sum_j row[j] x^(n - 1 - j).  row[0 .. k) is the data, unchanged (systematic); row[k .. n) is the
 *   parity, (d(x) x^nroots) mod g(x) with d(x) = sum_{j < k} row[j] x^(k - 1 - j).  Hence c(alpha^i) = 0 for every i < nroots.
 * DECODER, as a result.  Input: the received row r and, optionally, an erasure flag per byte (non-zero = erased); f = the number of
 *   flagged positions.  For a codeword c let e = #{j not flagged : c[j] != r[j]}.
 *       If f <= nroots and a codeword c with 2 e + f <= nroots exists, the output row is c.  Such a c is unique: the minimum distance is
 *       nroots + 1.
 *       Otherwise -- f > nroots included -- the output row is r, byte for byte, and the row's status is -1.
 *   Consequence: a word beyond the radius of the codeword that was sent, but within the radius of ANOTHER codeword, decodes to that other
 *   codeword, without a sign of it.  A caller who wants an end check puts a CRC of their own inside the data.
 *   d_info [nrows][4] int32:
 *       [0] the number of positions whose byte changed (flagged or not), or -1 on failure
 *       [1] f
 *       [2] e, or -1 on failure
 *       [3] 1 if r as received already had all nroots syndromes r(alpha^i) zero, else 0
 *   An erased position whose byte happens to be right counts in f and not in [0].
 *
 *   qpsk_rs_generator      host only, no context: the nroots + 1 coefficients of g into h_g, highest first, so h_g[0] = 1; nroots outside
 *                1 .. 64, or h_g NULL, is QPSK_ERR_ARG
 *   qpsk_rs_encode_batch   d_data [nrows][k] uint8, rows data_pitch bytes apart -> d_out [nrows][k + nroots], rows out_pitch bytes apart: the
 *                data, then the parity.  d_out must not overlap d_data
 *   qpsk_rs_decode_batch   d_in [nrows][n], rows in_pitch bytes apart; d_erase [nrows][n] uint8, tight, or NULL (nothing erased);
 *                d_out [nrows][n], rows out_pitch bytes apart; d_info [nrows][4] int32, 4-byte aligned.  d_out or d_info may be NULL, not
 *                both.  d_out may be exactly d_in with the same pitch (in place); any other overlap between d_out and d_in, and any
 *                overlap of d_info or d_erase with an output, is QPSK_ERR_ARG
 *   pitches      0 = tight (the row length); otherwise at least the row length; what lies between rows is never read or written
 *   limits       nrows >= 1 and CODE's
 * QPSK_ERR_ARG at the call for any bad argument, nothing launched.  Both batch calls are stream-ordered on the context's stream and touch
 * neither the receive streams, the deframer, the histogram mode's guess nor the Viterbi scratch.  qpsk_ctx_last_kernel() names
 * rs_encode_kernel / rs_decode_kernel.  A decode failure is a row's status: it is never a call error and never raises the context's status
 * word.
 * COMPOSITION.  in_pitch exists so that the d_bytes [nstreams][max_packets][nbytes + 2] of qpsk_deframer_push / _push_coded is decoded where
 * it lies: n = nbytes, in_pitch = nbytes + 2, nrows = nstreams * max_packets.  The packet's CRC is then over the codeword.
 * Not built: other field polynomials or first roots (CCSDS's dual-basis code among them), nroots > 64, the outer code inside the deframer's own launch, qpsk_multi.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_rs_generator(int nroots, uint8_t *h_g);
int qpsk_rs_encode_batch(qpsk_ctx *ctx, const uint8_t *d_data, long long data_pitch, int nrows, int k, int nroots, uint8_t *d_out,
                         long long out_pitch);
int qpsk_rs_decode_batch(qpsk_ctx *ctx, const uint8_t *d_in, long long in_pitch, int nrows, int n, int nroots, const uint8_t *d_erase,
                         uint8_t *d_out, long long out_pitch, int32_t *d_info);

/* -------------------------------------------------------------------------
 * PACKET ERASURE CODE: REED-SOLOMON's code laid across the packets of a group, against packets that are lost whole -- a sync word that was
 * not found, a fade longer than a codeword's radius, a body whose CRC fails behind every decoder.  The code is REED-SOLOMON's (field, g,
 * limits, c(x) = sum_p w[p] x^(n - 1 - p)) and nothing new; the library's own definition, integers only, no tolerance anywhere (parity
 * unpinned), restated in numpy by tests/test_cross_cpu.py (cross_encode_ref, cross_decode_ref, cross_place_ref).
 *
 * GROUP.  n = k + nroots packets of len bytes, pitch bytes apart (0 = len; otherwise >= len); ngroups groups lie n pitch bytes apart.
 *   Packets 0 .. k-1 are data, k .. n-1 parity.  The first skip bytes (0 <= skip < len) of EVERY packet are the caller's header -- the
 *   place of a sequence number, which a parity packet needs too: never coded, never changed.  For every column j in [skip, len) the word
 *   W_j[p] = byte j of packet p is one REED-SOLOMON word of (n, k).
 *   qpsk_rs_cross_encode_batch   in place on d_group [ngroups][n][pitch]: reads bytes [skip, len) of packets 0 .. k-1 and writes bytes
 *                [skip, len) of packets k .. n-1 so that every column is a codeword.  Nothing else is touched: not a header byte, not a
 *                byte between packets.  With payload_pitch = pitch the buffer is qpsk_frame_batch's d_payload of ngroups n packets as it lies.
 * DECODER, as a result.  d_have [ngroups][n] uint8: zero = packet p is missing and its bytes mean nothing; f = the zeros of a group.  Per
 *   column:  if f <= nroots and a codeword c exists that equals the column in every place that is NOT missing, the output column is c
 *   (unique, since f <= nroots < the minimum distance);  otherwise the output column is the input column byte for byte and the column has
 *   FAILED.  This is REED-SOLOMON's DECODER restricted to e = 0: where that decoder, on the column with the same flags, reports e = 0, the
 *   outputs are equal; where it reports e > 0 or fails, the column fails here.  So a wrong byte in a PRESENT packet is detected while
 *   f < nroots (through the nroots - f spare syndromes) and is invisible at f = nroots, where any k bytes determine a codeword.  A caller
 *   who wants such columns corrected gathers them and runs qpsk_rs_decode_batch on them.
 *   A missing packet's bytes decide nothing and never reach an output of a decoded column; they are read only to count [2] below and to
 *   copy a failed column.  Header bytes [0, skip) of every packet are copied to d_out as they are.
 *   qpsk_rs_cross_decode_batch   d_group as above (read only unless d_out is d_group); d_out [ngroups][n][out_pitch] may be exactly d_group
 *                with the same pitch (in place: only bytes that change are written), otherwise it must not overlap d_group; bytes between
 *                packets are never written
 *       d_info   [ngroups][4] int32, 4-byte aligned = { columns failed, f, places where the output differs from the input (all columns),
 *                1 if no column failed else 0 }
 *       d_colfail  [ngroups][len - skip] uint8, 1 = that column failed; may be NULL
 *                d_out or d_info may be NULL, not both.  A failed column is a group's result: never a call error, never the status word
 * PLACE: the bookkeeping between qpsk_deframer_push / _push_coded and the decoder.  Byte 0 of a packet is its sequence number q (so
 *   len >= 1, and the coding above uses skip >= 1).  Per stream the window is the ngroups n <= 256 numbers from d_base[stream] & 255 on
 *   (d_base int32 [nstreams], NULL = 0).  The packets i < min(d_count[stream], max_packets) are taken in index order: d = (q - base) & 255;
 *   a packet with d_crc_ok == 0 or d >= ngroups n is ignored; otherwise its len bytes go to d_group[stream][d / n][d % n] and
 *   d_have[stream][d] becomes 1.  Of two packets with the same d the later index wins.  The call never clears d_have and writes no slot
 *   it does not fill: a caller accumulates over as many pushes as a window spans and clears between windows.  Deterministic.
 *   qpsk_rs_cross_place_batch    d_bytes [nstreams][max_packets][byte_pitch] (0 = len; the deframers': nbytes + 2), d_count [nstreams]
 *                int32 and d_crc_ok [nstreams][max_packets] as the push left them -> d_group [nstreams][ngroups][n][pitch],
 *                d_have [nstreams][ngroups n]; no output may overlap an input or the other output
 * QPSK_ERR_ARG at the call, nothing launched, for: a bad (n, k, nroots), len < 1, skip outside [0, len), a pitch below len, ngroups < 1,
 * ngroups n > 256 or n > 255 in place, max_packets or nstreams < 1, overlapping buffers, NULL where a pointer is required, a misaligned int32
 * array.  The three calls are stream-ordered on the context's stream and touch no other state of the context.  qpsk_ctx_last_kernel() names
 * rs_cross_encode_kernel, rs_cross_decode_kernel or rs_cross_place_kernel.
 * Not built: errors and erasures per column (qpsk_rs_decode_batch on the failed columns is the way), a stateful collector that carries
 * windows across pushes, sequence numbers wider than a byte, qpsk_multi.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_rs_cross_encode_batch(qpsk_ctx *ctx, uint8_t *d_group, long long pitch, int ngroups, int k, int nroots, int len, int skip);
int qpsk_rs_cross_decode_batch(qpsk_ctx *ctx, const uint8_t *d_group, long long pitch, int ngroups, int n, int nroots, int len, int skip,
                               const uint8_t *d_have, uint8_t *d_out, long long out_pitch, int32_t *d_info, uint8_t *d_colfail);
int qpsk_rs_cross_place_batch(qpsk_ctx *ctx, const uint8_t *d_bytes, long long byte_pitch, const int32_t *d_count, const uint8_t *d_crc_ok,
                              int nstreams, int max_packets, int len, int n, int ngroups, const int32_t *d_base, uint8_t *d_group,
                              long long pitch, uint8_t *d_have);

/* -------------------------------------------------------------------------
 * VITERBI STREAM: the decoder of CONVOLUTIONAL CODE for a code that runs continuously -- no packets, no tails, no row that ends (the inner
 * code of DVB-S behind REED-SOLOMON's (204, 188) is one).  It carries its path metrics and a ring of decision words from call to call and
 * emits every bit once it is `depth` steps old.  The library's own definition, integers only, no tolerance anywhere (parity unpinned,
 * DESIGN.md 4.4.13), restated in numpy by tests/test_viterbi_stream_cpu.py (viterbi_stream_ref, conv_encode_stream_ref).  Code, branch
 * metric, step, the tie rule (A TIE KEEPS p0), the -128 -> -127 rule and the erasure 0 are word for word qpsk_viterbi_batch's.
 *
 * RESET (nstreams, depth D, window W, pattern).  nstreams >= 1; D and W multiples of 64, both >= 64, D + W <= 8192; (period, keep0, keep1) a
 *   pattern under PUNCTURING's rules, (1, 1, 1) = rate 1/2, K = popc(keep0) + popc(keep1).
 * PUSH.  Every stream gets the same number ntx of transmitted dibits, rows row_pitch dibits apart in the layout qpsk_soft_batch writes
 *   (0 = ntx; otherwise >= ntx; what lies between rows is never read).  A push carries WHOLE PATTERN PERIODS: 2 ntx must be a multiple of K,
 *   and the push holds n = (2 ntx / K) period trellis steps, 1 <= n <= 131072; anything else is QPSK_ERR_ARG with nothing launched and the
 *   state untouched.  At rate 1/2 every ntx >= 1 is legal; for the four named patterns every multiple of 12 dibits is.  So the pattern's
 *   phase is 0 at a push's first step, and within a push the sent bits are numbered as PUNCTURING does with nsteps = n:
 *       s_j of the push's step u = sent(u, j) ? v(idx(u, j)) : 0          (after the -128 rule)
 * FORWARD.  t = the step's absolute number since the reset (or the last flush), 64-bit, the same for every stream.
 *   start: pm[0] = 0, the 63 others NEG = -2^30.
 *   NORMALISATION: before every step with t % 64 == 0, max(pm) is subtracted from all 64 metrics.  (At t = 0 that is 0.  Every state is
 *   reachable by t = 6, so from t = 64 on max - min <= 3048 and the int32 metrics stay bounded for ever; a common offset changes no
 *   decision and no argmax.)  The step itself is qpsk_viterbi_batch's.
 * DECISION POINTS: at every T = k W, k >= 1, after step T - 1:
 *       st = the state of the largest pm, TIES TO THE LOWEST STATE NUMBER
 *       for t = T-1 down to max(0, T-D-W):   bit[t] = st & 1;   st = (st >> 1) | (d[t][st] << 5)
 *   Bits t in [T-D-W, T-D) with t >= 0 are FINAL and emitted, in ascending order; if T <= D nothing is.  Emitted counts are therefore
 *   multiples of 64 bits.  NOTHING DEPENDS ON HOW THE STEPS WERE CUT INTO PUSHES: any partition of the same steps gives the same
 *   concatenated bits, the same summed counts and the same state and spread at every decision point.
 *   A decision walks D + W steps to emit W: that cost is part of the definition and the caller's choice of W against latency.
 * FLUSH (flags).  With `total` steps in: st = 0 with QPSK_VITERBI_STREAM_TERMINATED, otherwise the argmax as above (the reported spread is
 *   the metrics' either way); trace back from total - 1 down to e = max(0, floor(total / W) W - D), e = 0 while total < W -- the first bit
 *   not yet emitted -- and emit [e, total): fewer than D + W bits.  Afterwards the streams are as after a reset with the same parameters.
 * CHANNEL ERRORS.  The emitted bit sequence of a stream is re-encoded (register fed by all earlier emitted bits, zeros before bit 0); for
 *   every emitted step, a non-zero soft value whose sign disagrees with the re-encoded bit is an error (qpsk_viterbi_batch's rule).
 * OUTPUTS of a push or a flush:
 *   d_bits [nstreams][bits_pitch bytes] uint8: bit j of THIS CALL's emitted bits in byte j >> 3 at position j & 7; bytes beyond
 *       ceil(nbits / 8) are not written.  bits_pitch 0 = ceil(nbits / 8); one too small for this call's bits is QPSK_ERR_ARG, nothing launched
 *   *h_nbits (may be NULL) = the bits each stream emits in this call: host arithmetic on total, D and W, handed back without a
 *       synchronisation.  qpsk_viterbi_stream_emits(ntx) = what a push of ntx would emit now (< 0: an error code), to size d_bits by
 *   d_info [nstreams][4] int32, for this call = { channel errors among the emitted steps, non-zero soft values among the emitted steps,
 *       the state the call's last decision traced from (a flush: its st) or -1 if it had none, max(pm) - min(pm) at that decision or 0 }
 *   Either output may be NULL, not both.
 * Hence, and tested:  (1) partition independence, above;  (2) if floor(N / W) W <= D nothing is emitted before the flush, whose bits equal
 *   qpsk_viterbi_batch / _punct_batch on the N-step row with QPSK_VITERBI_OPEN_END (flags 0 with TERMINATED) and whose error count is that
 *   call's d_info[3];  (3) on noise-free input (+-64, any named pattern, D = W = 64) the output is the data.
 *
 *   qpsk_viterbi_stream_reset   one decoder per context; a refused reset leaves an armed one as it was, a failed allocation
 *                (QPSK_ERR_ALLOC) the context usable
 *   qpsk_viterbi_stream_push / _flush   QPSK_ERR_STATE before a reset; d_soft 2-byte, d_info 4-byte aligned
 *   qpsk_conv_encode_stream_batch   the transmit twin: qpsk_conv_encode_punct_batch without a tail over a register that is carried.  The six
 *                bits before the row come from d_state_in[row] (uint8, bit k = the bit of step -1 - k; NULL = 0), the register's low six
 *                bits after the row go to d_state_out[row] (may be NULL; must not overlap d_state_in).  nbits covers whole periods that send
 *                whole dibits (nbits % period == 0, an even number of sent bits); d_dibits [nrows][nbits / period * K / 2]
 * The calls are stream-ordered on the context's stream and touch neither the deframer, the receive streams, the histogram mode's guess
 * nor the Viterbi scratch buffer: qpsk_viterbi_batch may be called between pushes.  qpsk_ctx_last_kernel() names viterbi_stream_kernel,
 * viterbi_stream_punct_kernel (any pattern but (1, 1, 1)), viterbi_stream_flush_kernel, viterbi_stream_init_kernel or
 * conv_encode_stream_kernel.
 * Not built: d_flip (a descrambler on the soft values) and an interleaver in front of the stream decoder; streams pushed with different
 * step counts; qpsk_multi.  The quarter-turn (90 degrees) and pattern-phase ambiguity of a continuous link is resolved in front of the
 * decoder by NODE SYNC, which reads this call's d_info[0] / d_info[1] on the device; the half turn is resolved behind the decoder, by OUTER
 * LINK's word sync, and the byte interleaver of a continuous link is OUTER LINK's too.
 * ------------------------------------------------------------------------- */
enum { QPSK_VITERBI_STREAM_TERMINATED = 1 };
int qpsk_viterbi_stream_reset(qpsk_ctx *ctx, int nstreams, int depth, int window, int period, uint32_t keep0, uint32_t keep1);
int qpsk_viterbi_stream_emits(qpsk_ctx *ctx, int ntx);
int qpsk_viterbi_stream_push(qpsk_ctx *ctx, const int8_t *d_soft, long long row_pitch, int ntx, uint8_t *d_bits, long long bits_pitch,
                             int32_t *d_info, int *h_nbits);
int qpsk_viterbi_stream_flush(qpsk_ctx *ctx, int flags, uint8_t *d_bits, long long bits_pitch, int32_t *d_info, int *h_nbits);
int qpsk_conv_encode_stream_batch(qpsk_ctx *ctx, const uint8_t *d_bits, int nrows, int nbits, int period, uint32_t keep0, uint32_t keep1,
                                  const uint8_t *d_state_in, uint8_t *d_state_out, uint8_t *d_dibits);

/* -------------------------------------------------------------------------
 * OUTER LINK: what stands between VITERBI STREAM and REED-SOLOMON on a continuously coded link -- word sync with carried state, polarity
 * (half-turn) resolution, a convolutional (Forney) byte deinterleaver, and aligned words out, ready for qpsk_rs_decode_batch through a
 * pitch; and the interleaver that is its transmit twin.  The library's own definition, integers only, no tolerance anywhere (parity
 * unpinned: the reference has no FEC), restated in numpy by tests/test_outer_cpu.py (outer_ref, outer_interleave_ref).
 *
 * RESET (nstreams >= 1; n = 2..255 bytes a word; branches I = 1..32 with n % I == 0, the cell is M = n / I so that M I = n, as in DVB-S:
 *   204 = 12 * 17; sync = one byte value; lock L = 1..16; drop = 0..16, 0 = never drop; flags of QPSK_OUTER_POLARITY | QPSK_OUTER_MSB_FIRST).
 * BYTES.  For one stream let B be the concatenation of every bit pushed since the reset.
 *       V(u) = sum_{i<8} B[u+i] << i          the first bit in bit 0: the packing of qpsk_viterbi_stream_push's d_bits and qpsk_pack_symbols
 *       with MSB_FIRST                << (7-i)   DVB's order
 *       m(u) = +1 if V(u) == sync;  -1 if POLARITY is set and V(u) == sync ^ 0xFF;  0 otherwise
 * HUNT, from h (0 after a reset):  u* = the smallest u >= h with m(u) != 0 and m(u + 8 n i) == m(u) for every i < L.  The lock is declared by
 *   the push that delivers bit u* + 8 n (L-1) + 7; every smaller candidate is decidable by then.  After it: u0 = u*, s = m(u*), c = 0, run = 0.
 * LOCKED.  Raw word c is the bits [u0 + 8 n c, u0 + 8 n (c+1));  Y[c][q] = V(u0 + 8 (n c + q)) ^ (s < 0 ? 0xFF : 0).  Words are handled in
 *   order of c, each by the push that delivers its last bit:
 *     1. miss = (Y[c][0] != sync);  run = miss ? run + 1 : 0
 *     2. if drop > 0 and run == drop: the lock is lost, nothing is emitted for c, HUNT resumes at h = u0 + 8 n c + 1, the words in flight
 *        are gone
 *     3. otherwise, if c >= I - 1, one word is emitted:  Z[q] = Y[c - (I - 1 - q mod I)][q], q < n, with pos = u0 + 8 n c (int64, counted
 *        from the reset) and flags: bit 0 = (Z[0] != sync), bit 1 = (s < 0)
 *     4. c += 1
 *   The state machine runs as far as the bits that have arrived allow and no further; nothing is pending at an end: a word whose last bit
 *   never comes is not emitted, and there is no flush.  THE RESULT DEPENDS ONLY ON B, NOT ON HOW B WAS CUT INTO PUSHES, except for which push
 *   reports a word.
 * WORD BOUND.  A push of nbits emits at most L + ceil(nbits / 8 n) words per stream; qpsk_outer_max_words(nbits) returns that by host
 *   arithmetic (< 0: an error code).  (The tightest push -- one that completes a lock with L - 1 whole words behind it -- emits one word
 *   fewer: emitted words end at least 8 n bits apart, and only a lock declared in the push adds words that ended before it, L - 1 of them.)
 * PUSH.  Every stream gets the same nbits, 1..2^20, any value, not only multiples of 8.
 *   d_bits [nstreams][bits_pitch bytes]: bit j of this call in byte j >> 3 at position j & 7 -- exactly what qpsk_viterbi_stream_push /
 *       _flush write.  bits_pitch 0 = ceil(nbits / 8), otherwise >= that; what lies beyond a row's bits is never read
 *   d_count [nstreams] int32, required: the true number of words of this call, also beyond max_words
 *   d_words [nstreams][max_words][word_pitch]: word_pitch 0 = n, otherwise >= n; bytes between words are never written.  It is then
 *       qpsk_rs_decode_batch's d_in with in_pitch = word_pitch and nrows = nstreams * max_words
 *   d_pos [nstreams][max_words] int64, d_flags [nstreams][max_words] uint8: as above.  Each of these three may be NULL; only the first
 *       min(count, max_words) entries of a stream are written
 *   d_info [nstreams][4] int32 (may be NULL) = { 1 if locked after the call else 0, s or 0, locks declared in this call, locks lost in
 *       this call }
 *   No output may share a byte with the input or another output.  d_count and d_info 4-byte, d_pos 8-byte aligned.
 * THE TRANSMIT TWIN.  qpsk_outer_interleave_batch:  Y[c][q] = X[c - q mod I][q] over d_words / d_out [nrows][nwords][n].  The I - 1 source
 *   words before the call come from d_hist_in [nrows][I-1][n], the last I - 1 source words, oldest first (NULL = zeros); the last I - 1
 *   source words after the call go to d_hist_out (may be NULL; must not overlap any input, nor may d_out).  This is Forney's interleaver with
 *   I branches of j M cells, the sync byte on the undelayed branch, and the receiver's Z is then X delayed by I - 1 words.  A caller puts
 *   `sync` into byte 0 of every word BEFORE RS-encoding it: the sync byte is data of the codeword, as in DVB.
 *
 * GROUP SYNC.  qpsk_outer_reset_group(..., group): group = 0 is qpsk_outer_reset.  Otherwise every G-th word, G = group = 3..16, carries the
 *   complement of the sync byte (DVB: G = 8, 0xB8 for 0x47), and lock L = G..16: a look-ahead over one whole group determines the polarity
 *   and the group phase uniquely (by enumeration for every such G and L); with L < G - 1, or with G = 2, two (s, g) share a sign pattern,
 *   and L = G - 1 would take L sync bytes with no complement among them for a lock.  Anything else is QPSK_ERR_ARG.  With  e(k) = -1 if k = 0, else +1  and  m(u) = +1 if V(u) == sync, -1 if V(u) == sync ^ 0xFF, 0 otherwise  (both signs
 *   are always formed in group mode, whatever POLARITY says):
 *   HUNT, from h:  u* = the smallest u >= h with m(u + 8 n i) != 0 for every i < L, for which there are an s in {+1, -1} (s = +1 only, if
 *     POLARITY is not set) and a g in 0..G-1 with m(u + 8 n i) = s e((i + g) mod G) for every i < L.  A candidate whose L bytes all match but
 *     whose signs fit no (s, g) is not a lock.  The lock is declared by the push that delivers bit u* + 8 n (L-1) + 7, as above.  After it:
 *     u0 = u*, s and g as found, c = 0, run = 0.
 *   LOCKED.  Raw word c has the group index k(c) = (g + c) mod G and the expected first byte E(c) = sync ^ (k(c) == 0 ? 0xFF : 0).  Steps 1
 *     to 4 as above, except:  miss = (Y[c][0] != E(c));  the emitted word Z is as above, bytes as received -- the sync byte is data of the
 *     codeword, 0xB8 stays 0xB8 --;  flags bit 0 = (Z[0] != E(c - (I - 1))), bit 1 = (s < 0), bits 4..7 = k(c - (I - 1)), bits 2 and 3 zero;
 *     a lost lock forgets g, and HUNT resumes at u0 + 8 n c + 1.
 *   The word bound, qpsk_outer_max_words, d_info, d_pos and THE RESULT DEPENDS ONLY ON B hold as above.  d_flags is then the d_flags of
 *   qpsk_dispersal_batch (DVB TRANSPORT).  Restated in numpy by tests/test_dvb_cpu.py (outer_group_ref).
 *
 *   qpsk_outer_reset / _reset_group   one link per context; a refused reset leaves an armed one as it was, a failed allocation
 *                (QPSK_ERR_ALLOC) the context usable.  qpsk_outer_reset knows no flag beyond the two below
 *   qpsk_outer_push / _max_words   QPSK_ERR_STATE before a reset; anything outside the rules above is QPSK_ERR_ARG with nothing launched
 *                and the state untouched
 * The calls are stream-ordered on the context's stream and touch no other state of the context.  qpsk_ctx_last_kernel() names
 * outer_push_kernel, outer_init_kernel or outer_interleave_kernel.
 * Built since: DVB's inverted sync byte in every eighth word is GROUP SYNC above, and its energy dispersal is DVB TRANSPORT below.
 * Not built: cells other than n / I; streams pushed with different
 * lengths; qpsk_multi.  The quarter-turn (90 degrees) search is NODE SYNC's, in front of the decoder.
 * ------------------------------------------------------------------------- */
enum { QPSK_OUTER_POLARITY = 1, QPSK_OUTER_MSB_FIRST = 2 };
int qpsk_outer_reset(qpsk_ctx *ctx, int nstreams, int n, int branches, int sync, int lock, int drop, int flags);
int qpsk_outer_reset_group(qpsk_ctx *ctx, int nstreams, int n, int branches, int sync, int lock, int drop, int flags, int group);
int qpsk_outer_max_words(qpsk_ctx *ctx, int nbits);
int qpsk_outer_push(qpsk_ctx *ctx, const uint8_t *d_bits, long long bits_pitch, int nbits, int max_words, int32_t *d_count, uint8_t *d_words,
                    long long word_pitch, long long *d_pos, uint8_t *d_flags, int32_t *d_info);
int qpsk_outer_interleave_batch(qpsk_ctx *ctx, const uint8_t *d_words, int nrows, int nwords, int n, int branches, const uint8_t *d_hist_in,
                                uint8_t *d_hist_out, uint8_t *d_out);

/* -------------------------------------------------------------------------
 * DVB TRANSPORT: the energy dispersal of ETSI EN 300 421 over groups of G transport packets, the stage behind REED-SOLOMON on the way in and
 * in front of it on the way out.  The library's own definition, integers only, on a keystream that is pinned: K[j], j >= 0, are the bits
 * scramble() (bit-scramble.c:57-68) xors onto successive input bits from SEED 0x4A80 -- the generator 1 + x^14 + x^15 loaded with
 * 100101010000000 -- so dibit d of qpsk_scramble_batch's keystream is K[2 d] | K[2 d + 1] << 1.  Restated in numpy by tests/test_dvb_cpu.py
 * (dispersal_ref).
 *       PR[t] = sum_{i<8} K[8 t + i] << i,  t = 0 .. G len - 2;  with QPSK_DISPERSAL_MSB_FIRST  << (7 - i), DVB's order: PR = 03 F6 08 34 30
 *               B8 A3 93 ..., the sequence the standard prints; G = 8, len = 188 gives its period of 1503 bytes
 *       a row of len bytes with group index k:   out[0] = in[0] ^ (k == 0 ? 0xFF : 0);   out[q] = in[q] ^ PR[k len + q - 1], 1 <= q < len
 * The generator runs through the sync bytes of packets 1 .. G-1 and is not applied to them.  The map is an involution: the same call
 * randomises on the way out and de-randomises on the way in.
 *   qpsk_dispersal_batch     nrows >= 1 rows of len = 2..255 bytes, group = 1..16, flags 0 or QPSK_DISPERSAL_MSB_FIRST; d_in / d_out rows
 *                in_pitch / out_pitch bytes apart, 0 = len, otherwise >= len; bytes between rows are neither read nor written.
 *                d_flags == NULL: row r has the index (first + r) mod group, first = 0..group-1 -- the transmitter's case.  Otherwise the
 *                index of row r is d_flags[r] >> 4, exactly the array qpsk_outer_push writes under GROUP SYNC, and first must be 0; a row
 *                whose index is >= group is copied unchanged (rows beyond a stream's d_count hold whatever was in memory; their index is
 *                never used as an address).  d_out == d_in with equal pitches is allowed (in place); otherwise no two of d_in, d_out and
 *                d_flags may overlap, a pitched buffer counting from its first row's first byte to its last row's last.  The table of a
 *                (len, group, flags) is built on the host and kept in the context; a call that names another triple waits for the
 *                context's stream once and replaces it
 *   qpsk_dispersal_sequence  host only, no context, no device: writes PR[0 .. group len - 2] to out and returns group len - 1, or < 0: an
 *                error code
 * QPSK_ERR_ARG at the call for a bad argument, decided before the context is looked at, nothing launched.  qpsk_dispersal_batch is
 * stream-ordered on the context's stream and touches no other state of the context; qpsk_ctx_last_kernel() names dispersal_kernel.
 * Not built: a fused RS-decode + dispersal; qpsk_multi; DVB's I/Q mapping of the punctured code.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
enum { QPSK_DISPERSAL_MSB_FIRST = 1 };
int qpsk_dispersal_batch(qpsk_ctx *ctx, const uint8_t *d_in, long long in_pitch, int nrows, int len, int group, int flags, const uint8_t *d_flags,
                         int first, uint8_t *d_out, long long out_pitch);
int qpsk_dispersal_sequence(int len, int group, int flags, uint8_t *out);

/* -------------------------------------------------------------------------
 * CHANNELISER: a critically sampled polyphase analysis filter bank, the stage in front of qpsk_streams_rx_cplx -- one wideband complex
 * capture that carries M carriers side by side comes out as M channel rows, each at 1 / M of the wideband rate, laid out as that call takes
 * them.  State (the filter's history) is carried from push to push.  The library's own definition, every operation in fp32 and in a stated
 * order (the reference has no channeliser; parity unpinned), restated in numpy by tests/test_channel_cpu.py (channel_ref)
 * and compared with the kernel bit for bit.  There is no tolerance anywhere.
 *
 * M   channels, a power of two, 2 <= M <= 4096.   P   taps per branch, 1 <= P <= 32.
 * h[0 .. M P)   the caller's real prototype low-pass, finite floats (the library designs no filter).
 * s   the history followed by the pushed samples; the history is (P - 1) M samples, all zero after a reset.  block(b) = s[b M .. b M + M).
 *   Output time m of a push is the block that holds the push's samples [m M, m M + M); block(m - q) is the block q blocks before it.
 * BRANCH SUMS, p = 0 .. M - 1, real and imaginary part separately, fp32, no contraction:
 *       u_m[p] = sum_{q = 0}^{P - 1} h[q M + p] block(m - q)[M - 1 - p]
 *   acc = fl(h[p] x_0), then acc = acc + fl(h[q M + p] x_q) for q = 1 .. P - 1 in that order.
 * TRANSFORM, fp32: the butterfly network of the library's radix-2 transform with the inverse sign.  v = u_m in bit-reversed order
 *   (v[bitrev(p)] = u_m[p]); then stages s = 1 .. log2 M, half = 2^(s - 1): for every lo whose bit s - 1 is clear, k = lo mod half,
 *   hi = lo + half, e = v[lo], o = v[hi], w = tw[k (M >> s)]:
 *       z = (w.re o.re - w.im o.im, w.re o.im + w.im o.re),   v[lo] = e + z,   v[hi] = e - z
 *   tw[j] = ((float)cos(TAU j / M), (float)sin(TAU j / M)), j < M / 2, computed in double with libm on the host, TAU = 2 * 3.14159265358979323846
 *   (qpsk_channel_twiddles writes the table: it is part of the definition).  No scaling.
 *       y_k[m] = v[k] is channel k: the band centred at +k / M cycles per wideband sample (k > M / 2: at k / M - 1), with the gain
 *       sum h at its centre, up to a fixed rotation per channel that the Costas loop absorbs.
 *   The kernel keeps two stages in registers per pass; it performs exactly these operations on these operands.
 * OUTPUT.  d_out[i][m] = y_{chan[i]}[m], rows out_pitch complex samples apart (0 = tight, T), the unit of frame_pitch.
 * NaN, Inf.  A non-finite sample propagates as IEEE arithmetic says (0 * Inf = NaN included, -0.0 as the operations give it); the call
 *   raises no status -- the stream call behind it has the fence.
 * HISTORY.  After a push the history is the last (P - 1) M samples of s: a push of T < P - 1 blocks shifts the old history.
 *
 *   qpsk_channel_twiddles  host only, no context: tw[M / 2][2] into h_tw.  QPSK_ERR_ARG for an M outside M's rule or a NULL h_tw
 *   qpsk_channel_reset     (M, P, h_proto [M P]); h_chan [nsel] host channel numbers in [0, M), any order, repeats allowed,
 *                1 <= nsel <= 65536; NULL = all M channels in order (nsel is then not looked at).  Copies both, zeroes the history,
 *                replaces a channeliser the context has (behind a synchronisation of the context's stream); a refused reset leaves it
 *   qpsk_channel_push      d_x [T M][2] -> d_out [nsel] rows of [T][2].  T >= 1, T M <= 2^30; out_pitch 0 or >= T; d_out must not
 *                overlap d_x.  QPSK_ERR_STATE before a reset
 * QPSK_ERR_ARG at the call for a bad argument -- a non-finite tap among them -- nothing launched.  A push is stream-ordered on the
 * context's stream and touches neither the receive streams, the deframers, the histogram mode's guess, the Viterbi scratch, the outer link
 * nor the node sync.  qpsk_ctx_last_kernel() names channel_push_kernel (polyphase_history_kernel, the launch behind it, moves the history
 * into the second of two buffers, so that no launch reads what it writes).
 * Not built: oversampled banks; M that is no power of two; PCM or int16 wideband input; qpsk_multi; routing inside bench.py.  The
 * transmit twin is SYNTHESIS BANK below.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_channel_twiddles(int M, float *h_tw);
int qpsk_channel_reset(qpsk_ctx *ctx, int M, int P, const float *h_proto, const int32_t *h_chan, int nsel);
int qpsk_channel_push(qpsk_ctx *ctx, const float *d_x, int T, float *d_out, long long out_pitch);

/* -------------------------------------------------------------------------
 * SYNTHESIS BANK: the channeliser's transmit twin, a critically sampled polyphase synthesis filter bank -- nsel channel rows, each at 1 / M
 * of the wideband rate (the shaped baseband qpsk_tx_symbols hands out, for one), come out as ONE wideband complex capture with row i in
 * channel chan[i]: what CHANNELISER takes.  State (the last transformed vectors) is carried from push to push.  The library's own definition,
 * every operation in fp32 and in a stated order (the reference has no filter bank; parity unpinned), restated in numpy by
 * tests/test_synth_cpu.py (synth_ref) and compared with the kernels bit for bit.  There is no tolerance anywhere.
 *
 * M   channels, a power of two, 2 <= M <= 4096.   P   taps per branch, 1 <= P <= 32.
 * g[0 .. M P)   the caller's real prototype low-pass, finite floats.  The library applies no scaling: the interpolation gain M is the
 *   caller's (M h for a prototype h of unit gain is exact in fp32, M being a power of two).
 * c_i[m], i < nsel, m < T   the input rows; row i feeds channel chan[i].  The channel numbers are DISTINCT (a repeat is QPSK_ERR_ARG), so
 *   nsel <= M; a channel nobody names is +0.0.
 * TRANSFORM, fp32: CHANNELISER's butterfly network and its table (qpsk_channel_twiddles), the same inverse sign, the same operands, the
 *   same order.  For every time m: v[bitrev(chan[i])] = c_i[m], +0.0 elsewhere; then the stages s = 1 .. log2 M exactly as written under
 *   CHANNELISER; V_m[r] = v[r], r = 0 .. M - 1.
 * BRANCH FILTER, r = 0 .. M - 1, real and imaginary part separately, fp32, no contraction:
 *       x[m M + r] = sum_{q = 0}^{P - 1} g[q M + r] V_{m - q}[r]
 *   acc = fl(g[r] V_m[r]), then acc = acc + fl(g[q M + r] V_{m - q}[r]) for q = 1 .. P - 1 in that order.
 * HISTORY.  The last P - 1 transformed vectors V, (P - 1) M complex values, all zero after a reset; a push of T < P - 1 times shifts it.
 * NaN, Inf.  A non-finite sample propagates as IEEE arithmetic says (0 * Inf = NaN included, -0.0 as the operations give it); no status
 *   is raised.
 * WITH THE ANALYSIS BANK BEHIND IT (prototype h there, g here, both of M P taps, exact arithmetic): channel k of CHANNELISER on x is
 *       y_k[m'] = e^{j TAU k (M - 1) / M} sum_m c_k[m] (h * g)[(m' - m) M + M - 1]       (h * g: the convolution of the two prototypes)
 *   plus what the other channels leak through the two stop bands.  For symmetric prototypes (h * g) peaks at M P - 1, so the row comes back
 *   delayed by exactly P - 1 channel samples and turned by a fixed -k / M of a circle per channel, which the Costas loop and the deframer's
 *   rotation search absorb.
 *
 *   qpsk_synth_reset   (M, P, h_proto [M P] = g); h_chan [nsel] host channel numbers in [0, M), any order, DISTINCT, 1 <= nsel <= M; NULL =
 *                all M channels in order (nsel is then not looked at).  Copies both, zeroes the history, replaces a bank the context has
 *                (behind a synchronisation of the context's stream); a refused reset leaves it
 *   qpsk_synth_push    d_in [nsel] rows of [T][2], in_pitch complex samples apart (0 = tight, T) -> d_x [T M][2].  T >= 1, T M <= 2^27 (the
 *                scratch of transformed vectors between the bank's two launches is then 1 GiB); in_pitch 0 or >= T; d_x must not overlap
 *                the rows.  QPSK_ERR_STATE before a reset.  The scratch is the context's, sized by the largest push so far: a push that
 *                needs a larger one waits for the context's stream once and reallocates (QPSK_ERR_ALLOC leaves bank and history as they
 *                were); any other push is three launches and no synchronisation
 * QPSK_ERR_ARG at the call for a bad argument -- a non-finite tap and a channel named twice among them -- decided before the context is
 * looked at, nothing launched.  A push is stream-ordered on the context's stream.  The bank is state of its own: its calls touch neither
 * the channeliser, the receive streams, the deframers, the histogram mode's guess, the Viterbi scratch, the outer link nor the node sync,
 * and none of those calls touches the bank.  qpsk_ctx_last_kernel() names synth_filter_kernel (synth_transform_kernel runs in front of
 * it, polyphase_history_kernel behind it, into the second of two buffers, so that no launch reads what it writes).
 * Not built: a fused single-launch bank for small M; oversampled banks; M that is no power of two; real or int16 output; qpsk_multi; routing
 * inside bench.py.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_synth_reset(qpsk_ctx *ctx, int M, int P, const float *h_proto, const int32_t *h_chan, int nsel); /* h_chan NULL = all M in order */
int qpsk_synth_push(qpsk_ctx *ctx, const float *d_in, long long in_pitch, int T, float *d_x);

/* -------------------------------------------------------------------------
 * RESAMPLER: a batched polyphase rational resampler, the stage between a capture's rate and the modem's -- both banks above are critically
 * sampled, so their rows run at exactly 1 / M of the capture rate, and the modem behind them at exactly FS = CYCLES RS; a front end that was
 * not made for this modem delivers FS D / L.  nstreams rows go in at one rate and come out at L / D of it, laid out as qpsk_streams_rx_cplx
 * (or, on the transmit side, qpsk_synth_push) takes them.  State is carried from push to push.  Input and output lengths differ per push,
 * so the interface is driven from the OUTPUT: the caller names the outputs it wants, qpsk_resample_need says how many inputs they consume.
 * The library's own definition, every operation in fp32 and in a stated order (the reference has no resampler; parity unpinned, DESIGN.md
 * 4.4.20), restated in numpy by tests/test_resample_cpu.py (resample_ref) and compared with the kernel bit for bit.  There is no tolerance
 * anywhere.
 *
 * L   interpolation factor, 1 <= L <= 512.   D   decimation factor, 1 <= D <= 4096; gcd(L, D) need not be 1.
 * P   taps per branch, 1 <= P <= 32.   h[0 .. L P)   the caller's real prototype, finite floats.  The library designs no filter and applies
 *   no scaling: the interpolation gain L is the caller's.
 * nstreams rows, 1 <= nstreams <= 65536; all share L, D, P, h and the position, so the rows stay aligned.
 * s   per stream, every complex sample pushed since the reset, preceded by zeros.
 * OUTPUT n, counted from the reset: t = n D, i = t div L, b = t mod L,
 *       y[n] = sum_{q = 0}^{P - 1} h[q L + b] s[i - q]
 *   real and imaginary part separately, fp32, no contraction: acc = fl(h[b] s[i]), then acc = acc + fl(h[q L + b] s[i - q]) for
 *   q = 1 .. P - 1 in that order.  This is v = h * (s zero-stuffed by L), y[n] = v[n D].
 * POSITION.  After the outputs [0, n0) a stream has consumed c0 = (the input index of output n0 - 1) + 1 inputs.  The whole carried position
 *   is the one integer r = n0 D - c0 L: 0 after a reset, in [D - L, D) after every push; no counter grows.  A push of N outputs uses t = r + n D, n < N,
 *   relative to its first new input (floor division: i = t div L >= -1), consumes K = (r + (N - 1) D) div L + 1 inputs -- K may be 0 when
 *   L > D and N is small -- and leaves r += N D - K L.
 * HISTORY.  The last P consumed samples per stream (not P - 1: with L > D an output may use no new input at all, i = -1), all zero after a
 *   reset.  A push with K < P shifts it, a push with K = 0 leaves it.
 * NaN, Inf.  A non-finite sample propagates as IEEE arithmetic says (0 * Inf = NaN included, -0.0 as the operations give it); the call
 *   raises no status -- the stream call behind it has the fence.
 *
 *   qpsk_resample_reset  (nstreams, L, D, P, h_proto [L P]).  Copies the taps, zeroes the history and r, replaces a resampler the context
 *                has (behind a synchronisation of the context's stream); a refused reset leaves it
 *   qpsk_resample_need   host only: the K the NEXT push of nout outputs consumes; < 0 on error (QPSK_ERR_STATE before a reset)
 *   qpsk_resample_push   d_in [nstreams] rows of [nin][2], in_pitch complex samples apart (0 = tight, nin) -> d_out [nstreams] rows of
 *                [nout][2], out_pitch apart (0 = tight, nout: with nout = frame_size exactly the block qpsk_streams_rx_cplx takes; with
 *                in_pitch = qpsk_channel_push's out_pitch the channeliser's rows are read where they lie).  1 <= nout <= 2^24 and
 *                nout D + L < 2^31; nin must equal qpsk_resample_need(ctx, nout), and nin = 0 is legal (d_in may then be NULL); a pitch is 0
 *                or at least its row; d_out must not overlap d_in.  QPSK_ERR_STATE before a reset
 * QPSK_ERR_ARG at the call for a bad argument -- a non-finite tap and an nin other than the need among them -- nothing launched, state
 * untouched; what the arguments alone decide is decided before the context is looked at.  A push is stream-ordered on the context's stream
 * with no host synchronisation.  The resampler is state of its own: its calls touch neither the two banks, the receive streams, the
 * transmitters, the deframers, the Viterbi scratch, the outer link nor the node sync, and none of those calls touches it.
 * qpsk_ctx_last_kernel() names resample_push_kernel (polyphase_history_kernel, the launch behind it when K > 0, moves the history into the
 * second of two buffers, so that no launch reads what it writes).
 * Not built: per-stream ratios; a ratio that changes while running (clock-drift tracking); irrational ratios and Farrow structures; real or
 * int16 rows; qpsk_multi; routing inside bench.py.  Usage: INTEGRATION.md 2.0.
 * ------------------------------------------------------------------------- */
int qpsk_resample_reset(qpsk_ctx *ctx, int nstreams, int L, int D, int P, const float *h_proto);
int qpsk_resample_need(qpsk_ctx *ctx, int nout);   /* host only: the K the NEXT push of nout outputs consumes; < 0 on error */
int qpsk_resample_push(qpsk_ctx *ctx, const float *d_in, long long in_pitch, int nin, int nout, float *d_out, long long out_pitch);

/* -------------------------------------------------------------------------
 * NODE SYNC: what stands between qpsk_soft_batch and VITERBI STREAM on a continuously coded link -- the quarter turn the Costas loop may
 * have locked on and the phase of the puncturing pattern are unknown, and a loop that slips changes both mid-stream.  Per link a CANDIDATE
 * (quarter turn r, delay h in dibits) is applied to the soft rows, and a MONITOR judges it by the error count the stream decoder reported for
 * the previous block and moves to the next candidate when it is bad; one launch per block does both, with no host synchronisation and no
 * decoder reset.  The library's own definition, integers only, no tolerance anywhere (parity unpinned: the reference has no FEC), restated
 * in numpy by tests/test_nodesync_cpu.py (nodesync_ref).  The code is transparent to the half turn (r and r + 2 decode alike, the data
 * inverted), so two rotation candidates, r = 0 and r = 1, suffice and the half turn stays OUTER LINK's.
 *
 * RESET (nlinks >= 1; nrot in {1, 2, 4}; nshift = 1..32; span = 1..2^24; settle = 0..2^24; thr_num = 0..65535; thr_den = 1..65535; drop =
 *   1..16).  There are C = nrot nshift candidates; candidate c means r = c mod nrot, h = c div nrot: nrot = 2 tries r = 0 and r = 1, one of
 *   which is right or the half-turn twin of the right one; nrot = 4 tries all four and locks on the first of {r, r + 2} it meets.  After a reset
 *   every link has c = 0, locked = 0, run = 0, err = cnt = 0, settle_left = 0, switches = 0 and no input history.
 *   qpsk_nodesync_shifts(period, keep0, keep1) = the delays a pattern needs, by host arithmetic: K / 2 for even K, K for odd K, K =
 *   popc(keep0) + popc(keep1) (a delay of h dibits moves the pattern by 2 h sent bits); < 0: the error code of a bad pattern (PUNCTURING's
 *   rules).  1 for (1, 1, 1), 3 for 2/3, 2 for 3/4, 3 for 5/6, 4 for 7/8.
 * INPUT.  For one link X is the concatenation of every soft pair pushed since the reset, in qpsk_soft_batch's layout; -128 IS TAKEN AS -127
 *   BEFORE ANYTHING ELSE, so every negation is exact and -128 never appears in the output.  turn_r is qpsk_soft_batch's rule, same signs:
 *       r=0 (a, b)   r=1 (b, -a)   r=2 (-a, -b)   r=3 (-b, a)
 * PUSH (ntx dibits for every link, max(1, nshift - 1) <= ntx <= 2^20) does two things, in this order:
 *   1. TICK, only if d_vinfo is not NULL.  d_vinfo [nlinks][4] int32 = what qpsk_viterbi_stream_push wrote into its d_info for this link's
 *      previous block; e = word 0 (channel errors), n = word 1 (non-zero soft values).
 *          verdict = 0
 *          if n > 0:
 *              if settle_left > 0:   settle_left = max(0, settle_left - n);  verdict = 3
 *              else:
 *                  err += e;  cnt += n
 *                  if cnt >= span:
 *                      bad = (int64) err * thr_den > (int64) thr_num * cnt;   err = cnt = 0
 *                      if not bad:   run = 0;  locked = 1;  verdict = 1
 *                      else:
 *                          verdict = 2;  run += 1
 *                          if not locked or run >= drop:
 *                              c = (c + 1) mod C;  locked = 0;  run = 0;  settle_left = settle;  switches += 1
 *      All accumulators fit int32 (cnt < span + 2^19 on a decoder's counts).  A hunting link moves on after ONE bad span; a locked one after
 *      `drop` bad spans in a row.  settle covers the decoder's latency: the counts of the first depth + window steps behind a switch still
 *      belong to the old candidate.
 *   2. TRANSFORM with the candidate now in force.  With `total` = the dibits pushed before this call, for j < ntx and i = total + j:
 *          out[j] = turn_r(X[i - h])   if i - h >= 0
 *          out[j] = (0, 0)             otherwise (an erasure)
 *      The state keeps the last nshift - 1 input dibits of a link, so any h is available at the next push whatever the candidate was.
 *      Every link gets ntx dibits in and ntx out, so a push of whole pattern periods stays one and d_soft_out goes into
 *      qpsk_viterbi_stream_push as it is.  WITH d_vinfo NULL IN EVERY PUSH NOTHING DEPENDS ON HOW THE DIBITS WERE CUT INTO PUSHES.
 * OUTPUTS.
 *   d_soft_out [nlinks][out_pitch dibits][2] int8, required; the span of its rows must not share a byte with the span of the input's
 *   d_info [nlinks][8] int32 (may be NULL) = { r, h, locked, switches since the reset, verdict of this call, run, err, cnt }, after the call
 *   in_pitch / out_pitch: 0 = ntx, otherwise >= ntx; what lies between rows is neither read nor written.  Both soft pointers are 2-byte
 *   aligned and nothing more, any pitch is legal; d_vinfo and d_info 4-byte aligned.
 * SET.  qpsk_nodesync_set(d_cand): d_cand [nlinks] int32 on the device, NULL = all zero; c = d_cand[l] as an unsigned number mod C; err =
 *   cnt = run = 0, locked = 0, settle_left = settle; the history and `switches` stay.  Stream-ordered, no synchronisation: how a caller who
 *   searched the candidates in parallel hands over the winner.
 * Hence, and tested:  (1) with nrot = nshift = 1 the output is the input after the -128 rule;  (2) partition independence, above;  (3)
 *   turn_r equals qpsk_soft_batch with d_rot = r on the same costas_frame[] rows wherever both are defined;  (4) with d_vinfo given the state
 *   after each push is a function of the old state and (e, n) alone.
 *
 *   qpsk_nodesync_reset   one node sync per context; a refused reset leaves an armed one as it was, a failed allocation (QPSK_ERR_ALLOC)
 *                the context usable
 *   qpsk_nodesync_push / _set   QPSK_ERR_STATE before a reset; anything outside the rules above is QPSK_ERR_ARG with nothing launched and the
 *                state untouched
 * The calls are stream-ordered on the context's stream and touch no other state of the context: the decoder's d_info is only ever a pointer
 * handed in.  qpsk_ctx_last_kernel() names nodesync_push_kernel or nodesync_init_kernel (a reset, a set).  How to choose thr and span from
 * the measured error ratios of right and wrong candidates: INTEGRATION.md 2.0.  No test hook: the only position the definition uses is
 * min(total, nshift - 1).
 * Not built: fan-out of all candidates into rows of one launch; a per-link ntx; qpsk_multi; a monitor fed by anything but the decoder's
 * error count, such as metric growth; a transform fused into the stream decoder's loader.
 * ------------------------------------------------------------------------- */
int qpsk_nodesync_reset(qpsk_ctx *ctx, int nlinks, int nrot, int nshift, int span, int settle, int thr_num, int thr_den, int drop);
int qpsk_nodesync_shifts(int period, uint32_t keep0, uint32_t keep1);
int qpsk_nodesync_push(qpsk_ctx *ctx, const int8_t *d_soft_in, long long in_pitch, int ntx, const int32_t *d_vinfo, int8_t *d_soft_out,
                       long long out_pitch, int32_t *d_info);
int qpsk_nodesync_set(qpsk_ctx *ctx, const int32_t *d_cand);

/* -------------------------------------------------------------------------
 * The stages on their own (each is what the corresponding reference function
 * computes, batched).
 * ------------------------------------------------------------------------- */

/* rrc_fir() (rrc_fir.c:17-30) on nframes independent delay lines.
 *   d_memory [nframes][127] complex float  in/out (may be NULL: zero history, not written back)
 *   d_in, d_out [nframes][length] complex float; d_out may equal d_in only if nframes*length
 *   fits the library's staging (it copies first); prefer separate buffers.
 *   qpsk_ctx_last_kernel() names the filter kernel afterwards: rrc_fir_stream_kernel (symmetric taps) or rrc_fir_kernel. */
int qpsk_rrc_fir_batch(qpsk_ctx *ctx, float *d_memory, const float *d_in, float *d_out, int nframes, int length);

/* The same filter by overlap-save with 512-point FFTs (algorithms/fft.h:44) -- FAST, NOT EXACT: the
 * transform changes the summation order of rrc_fir.c:22-26, so the output agrees with qpsk_rrc_fir_batch to ~1e-6 of the
 * frame's peak (bounds asserted in tests/test_gpu_parity.py::test_rrc_fir_fast_error_bounds), not bit for bit.  The
 * library itself never uses it: qpsk_rx_batch and the streams keep the exact kernels, whose symbols sit on decision
 * boundaries.  d_out must not alias d_in; d_memory as above (updated exactly: it is a copy of input samples). */
int qpsk_rrc_fir_batch_fast(qpsk_ctx *ctx, float *d_memory, const float *d_in, float *d_out, int nframes, int length);

/* timing histogram (qpsk.c:127-180) of nframes filtered blocks -> d_index[nframes]; d_hist, if not NULL,
 * receives hist_i[k] + hist_q[k], k = 0..7 (qpsk.c:175, locals of rx_frame) as [nframes][8] */
int qpsk_timing_hist_batch(qpsk_ctx *ctx, const float *d_filtered, int nframes, int32_t *d_index, int32_t *d_hist);

/* The histogram timing estimate (qpsk.c:127-180) straight from UNFILTERED frames: rrc_fir() with a fresh delay line
 * and the scan fused in one kernel, the filtered samples never leaving the CU (what qpsk_rx_batch runs in
 * QPSK_TIMING_HIST mode).  Needs CYCLES = 8, frame_size a multiple of 256, 16-byte aligned input; same results as
 * qpsk_rrc_fir_batch() followed by qpsk_timing_hist_batch().  d_index [nframes]; d_hist [nframes][8] or NULL. */
int qpsk_timing_scan_batch(qpsk_ctx *ctx, const float *d_in, int nframes, int32_t *d_index, int32_t *d_hist);

/* The FFT timing estimate alone (QPSK_TIMING_FFT; NEW DESIGN, the reference never calls fft.c: SURVEY section 0).
 *   d_index     [nframes] int32
 *   d_filtered  [nframes][512] complex float, may be NULL: the 512 rrc_fir() outputs (samples 128..639 of the frame,
 *               fresh delay line) the estimator looks at -- bit for bit what qpsk_rrc_fir_batch() returns there
 *   d_spectrum  [nframes][512] complex double, may be NULL: fftn(|y|^2, 512) as fft.c:110-120 returns it -- bit for
 *               bit qpsk_fft_batch() of the same 512 values
 * so that everything below the final argmax rule is reference-pinned code (rrc_fir.c:17-30, fft.c:98-120). */
int qpsk_timing_fft_batch(qpsk_ctx *ctx, const float *d_in, int nframes, int32_t *d_index, float *d_filtered,
                          double *d_spectrum);

/* The same estimate by the kernel qpsk_rx_batch() runs in QPSK_TIMING_FFT mode: of the 512-point transform only the
 * butterflies the symbol-rate bin X[512 / CYCLES] depends on are evaluated (511 of the recursion's fft.c:55-63 steps,
 * each with the full transform's operands, twiddle and order).
 *   d_bin  [nframes] complex double, may be NULL: that bin -- bit for bit d_spectrum[f][512 / CYCLES] above. */
int qpsk_timing_fft_bin_batch(qpsk_ctx *ctx, const float *d_in, int nframes, int32_t *d_index, float *d_filtered,
                              double *d_bin);

/* Costas loop + slicer (qpsk.c:196-212) over already decimated symbols.
 *   d_symbols_in [nframes][nsym] complex float;  d_state [nframes][2] float (phase, freq) in/out,
 *   NULL = start from (0,0) and do not write back. */
int qpsk_costas_batch(qpsk_ctx *ctx, const float *d_symbols_in, int nframes, int nsym, float *d_state,
                      uint8_t *d_sym, float *d_costas);

/* fftn()/ifftn() (fft.c:110-136) on nbatch independent length-n transforms, n a power of two up to 2^21 (one
 * workgroup per transform in LDS up to 8192 points, two passes over global memory above).
 *   d_in, d_out [nbatch][n] complex double, may be the same array; forward is scaled by 1/n, inverse is not
 *   (fft.c:105-107). */
int qpsk_fft_batch(qpsk_ctx *ctx, const double *d_in, double *d_out, int nbatch, int n, int inverse);

/* -------------------------------------------------------------------------
 * STREAMS: nstreams modems advancing one block per call with all state
 * carried, i.e. consecutive rx_frame() calls (qpsk.c:344-354): FIR delay
 * line, previous block's symbols, Costas phase/frequency, mixer phase.
 * Results are those of the PREVIOUS block (qpsk.c:186-197), as in the
 * reference.
 *
 * Error contract (all-or-poisoned).  A stream call enqueues several kernels.  If it fails between its launches (QPSK_ERR_HIP,
 * QPSK_ERR_ALLOC), or a kernel of a stream call reports that it gave up a bounded wait (QPSK_ERR_HIP from the call that
 * synchronises next), the carried state of ALL the context's streams is undefined: every later stream call -- the three
 * qpsk_streams_rx_*() and qpsk_streams_set/get_loop_state() -- returns QPSK_ERR_STATE until qpsk_streams_reset() has
 * completed successfully (a reset that itself fails leaves them refused).  Argument errors and QPSK_ERR_RANGE (a NaN / Inf
 * sample, a loop phase beyond the bounded wrap: flagged NUMBERS, the kernels completed) do not poison, and neither does a
 * failing batch call while no stream work is in flight.
 * ------------------------------------------------------------------------- */
int qpsk_streams_reset(qpsk_ctx *ctx, int nstreams, double mixer_hz);
/* the carried Costas state, h_state[nstreams][2] = (phase, freq): set_phase()/set_frequency() and
 * get_phase()/get_frequency() for every stream at once (costas_loop.c:117-132,148-150) */
int qpsk_streams_set_loop_state(qpsk_ctx *ctx, const float *h_state);
int qpsk_streams_get_loop_state(qpsk_ctx *ctx, float *h_state);
/* complex input (enters at qpsk.c:125) */
int qpsk_streams_rx_cplx(qpsk_ctx *ctx, const float *d_in, uint8_t *d_sym, float *d_freq, float *d_phase,
                         float *d_costas, int32_t *d_index);
/* int16 PCM input, mixed to complex on the GPU (qpsk.c:114-120) */
int qpsk_streams_rx_pcm(qpsk_ctx *ctx, const int16_t *d_pcm, uint8_t *d_sym, float *d_freq, float *d_phase,
                        float *d_costas, int32_t *d_index);
/* The same with HOST buffers on both sides -- the reference's call pattern (qpsk.c:344-354: fread a block, rx_frame()):
 * one pinned copy up (PCM + loop state), the kernels, one copy down (symbols, costas_frame[], loop state, index), ONE
 * synchronisation.  h_pcm [nstreams][frame_size]; h_loop_io [nstreams][2] (phase, freq), read before and written
 * after the block, NULL = the carried state; h_sym [nstreams][nsym]; h_costas [nstreams][nsym][2] or NULL;
 * h_index [nstreams] or NULL.  This is what the drop-in rx_frame() runs on. */
int qpsk_streams_rx_pcm_host(qpsk_ctx *ctx, const int16_t *h_pcm, float *h_loop_io, uint8_t *h_sym, float *h_costas,
                             int32_t *h_index);

/* -------------------------------------------------------------------------
 * TRANSMITTERS: nstreams independent modulators advancing
 * one block per call with the reference's carried state -- the tx_filter
 * delay line (rrc_fir.c:17, qpsk.c:243) and the carrier phase fbb_tx_phase
 * (qpsk.c:45,249-253).  One call = one qpsk_packet_mod() (qpsk.c:273-285)
 * per transmitter.
 * ------------------------------------------------------------------------- */
/* fbb_tx_phase = cmplx(0.0f); fbb_tx_rect = cmplx(TAU * tx_hz / FS); tx_filter zeroed (qpsk.c:316,320;
 * the shipped main() uses tx_hz = CENTER + 50.0) */
int qpsk_tx_reset(qpsk_ctx *ctx, int nstreams, double tx_hz);
/* d_symbols [nstreams][nsym] uint8, the dibit (tx_bits[s] << 1) | tx_bits[s+1] of qpsk.c:277-281 (the value
 * qpsk_rx_batch writes for the same symbol); d_pcm [nstreams][nsym*CYCLES] int16 as tx_frame() returns them
 * (qpsk.c:259-261), may be NULL; d_baseband [nstreams][nsym*CYCLES][2] float, the shaped complex signal
 * before the up-mix (qpsk.c:243), may be NULL -- not both */
int qpsk_tx_symbols(qpsk_ctx *ctx, const uint8_t *d_symbols, int nsym, int16_t *d_pcm, float *d_baseband);

/* -------------------------------------------------------------------------
 * Bit-level stages after the slicer (algorithms/ of the reference, which its qpsk.c does
 * not call yet), batched over independent packets.
 * ------------------------------------------------------------------------- */

/* crc16() (crc16.c:11-23: init 0xFFFF, polynomial 0x1021, no reflection, no final xor) of npackets packets of
 * nbytes bytes each: d_data [npackets][nbytes] -> d_crc [npackets] uint16 */
int qpsk_crc16_batch(qpsk_ctx *ctx, const uint8_t *d_data, int npackets, int nbytes, uint16_t *d_crc);

/* interleave() (interleave.c:33-78), in place on each packet of nbytes bytes: bit i goes to bit (b*i) mod nbits,
 * b = the largest table prime below nbits (the table ends at 347); dir 0 = INTERLEAVE, 1 = DEINTERLEAVE
 * (interleave.h:10-11).  nbytes*8 must be < 65536 as in the reference (uint16_t nbits). */
int qpsk_interleave_batch(qpsk_ctx *ctx, uint8_t *d_data, int npackets, int nbytes, int dir);

/* scramble() (bit-scramble.c:57-84) on every 2-bit symbol of npackets frames of nsym symbols, in place, the
 * 15-bit register reloaded with SEED 0x4A80 at the start of each frame (bit-scramble.c:11-13 "The Sync Seed is
 * reset at the start of each frame"); additive, so scrambling twice restores the input. */
int qpsk_scramble_batch(qpsk_ctx *ctx, uint8_t *d_sym, int npackets, int nsym);

/* -------------------------------------------------------------------------
 * MULTI: a batch of independent frames sharded over the GPUs of one node
 * (SURVEY.md 8(e)).  It stands where the reference has
 *     while (fread(frame, ...)) rx_frame(frame);                 qpsk.c:344-354
 * over process-global per-frame state (qpsk.c:36-53, costas_loop.c:13-23):
 * every frame is its own modem here, shard r of N takes the contiguous
 * frames [r F / N, (r + 1) F / N), one qpsk_ctx + one host thread + two
 * streams per shard, NO collective and no traffic between devices.  Results
 * (1 byte per symbol, freq and phase per frame) come back per device over
 * PCIe into pinned memory on the shard's second stream -- while the next
 * step's kernel runs -- and are written at the shard's place of the caller's
 * host arrays.
 *
 *   devices[ndev]   HIP ordinals, one shard each; repeats are allowed (two
 *                   shards on one GPU: a rehearsal on a one-GPU box)
 *   qpsk_multi_load total_frames frames of frame_size complex samples;
 *                   h_in = [total_frames][frame_size][2] float on the host
 *                   (uploaded, shard by shard) or NULL = the shards' device
 *                   buffers are allocated and left to the caller
 *                   (qpsk_multi_shard returns them; or
 *                   qpsk_multi_use_device_input lends one of the caller's)
 *   rx_begin(slot)  every shard: qpsk_rx_batch into result slot 0 / 1, then
 *                   its copy-back; returns once everything is ENQUEUED
 *   rx_end(slot, h_sym [total][nsym], h_freq [total], h_phase [total])
 *                   waits for that slot's copy-back on every device, checks
 *                   the kernels' status, concatenates (any of the three may
 *                   be NULL)
 * Pipelined: begin(0); begin(1); end(0); begin(0); end(1); ... -- the
 * copy-back of a step overlaps the kernel of the next.  A 16384-sample
 * frame returns 2056 bytes: 16.1 MiB per 8192-frame step, ~0.3 ms over PCIe
 * Gen5 x16 -- as long as the step's kernel; the copy-back, not the kernel,
 * bounds a host that wants every step's symbols (examples/shard_devices.c,
 * bench.py `gather`).  One caller thread at a time per qpsk_multi (the
 * object runs its own thread per shard; its entry points are not reentrant).
 * The entry points leave the caller's current HIP device as they found it.
 *
 * The verdict, per slot.  A shard's context has ONE kernel status word, which
 * the kernels of either slot's step may set.  A non-zero kernel status seen
 * by qpsk_multi_rx_end(k) on a shard fails that call.  It also fails the
 * rx_end of every other slot that was in flight on that shard at that
 * moment, with the same code and text.  On a failing rx_end the caller's
 * arrays are unspecified.  The slot is free afterwards.  (Conservative: a
 * good step may be reported bad next to a bad one; a bad step is never
 * reported good.  Once both slots have ended nothing stays behind.)
 *
 * A failed rx_begin.  When rx_begin(slot) fails on any shard -- a geometry
 * the context's tuning keys make rx_batch refuse, a HIP error -- it returns
 * the first failing shard's code and text, and the shards that did enqueue
 * are waited for and disarmed: the slot is free on EVERY shard, rx_end(slot)
 * answers "nothing in flight", rx_begin(slot) may be called again.  The
 * other slot is not touched.  (A rx_begin refused because the slot is still
 * in flight -- QPSK_ERR_STATE -- leaves that earlier step in flight.)
 *
 * A load with a step in flight.  qpsk_multi_load waits for every step in
 * flight and DROPS it, results and verdict: both slots are free afterwards,
 * rx_end for the dropped step answers "nothing in flight", and the new job
 * starts clean.
 * ------------------------------------------------------------------------- */
typedef struct qpsk_multi qpsk_multi;
int qpsk_multi_create(qpsk_multi **out, const int *devices, int ndev, const qpsk_params *p);
void qpsk_multi_destroy(qpsk_multi *mj);
int qpsk_multi_shards(const qpsk_multi *mj);
/* (a failed load -- QPSK_ERR_ALLOC -- frees what it had allocated and leaves the job without frames: rx_begin then returns QPSK_ERR_ARG) */
int qpsk_multi_load(qpsk_multi *mj, long long total_frames, const float *h_in);
/* shard r: its device, first frame and frame count, context and device input buffer (any pointer may be NULL) */
int qpsk_multi_shard(qpsk_multi *mj, int r, int *device, long long *first, long long *count, qpsk_ctx **ctx, float **d_in);
int qpsk_multi_use_device_input(qpsk_multi *mj, int r, const float *d_in);
/* Direct mode for a slot: its copy-back goes by DMA straight to the caller's arrays (each shard at its place) instead of to the library's
 * pinned staging, and qpsk_multi_rx_end(slot, NULL, NULL, NULL) only waits -- no concatenating memcpy on the host (16 MiB per 8192-frame
 * step: ~1.4 ms of one host core, five times the kernel).  The arrays must be page-locked (qpsk_host_alloc) and stay valid while the
 * slot is used; all NULL = back to staging.  QPSK_ERR_STATE while the slot is in flight on any shard, and then no shard is changed. */
int qpsk_multi_set_direct_output(qpsk_multi *mj, int slot, uint8_t *h_sym, float *h_freq, float *h_phase);
/* Packed mode: the symbols come back FOUR PER BYTE -- h_sym rows of ceil(nsym / 4) bytes, byte k = sym[4k] | sym[4k+1] << 2 | sym[4k+2] << 4 |
 * sym[4k+3] << 6 (qpsk_pack_symbols on the device, 16 MiB -> 4 MiB per 8192-frame step): the copy-back drops under the kernel's time and
 * a gathered step costs what the kernel costs.  qpsk_unpack_symbols_host() gives a byte per symbol again where a caller wants it. */
int qpsk_multi_set_packed(qpsk_multi *mj, int on);
int qpsk_pack_symbols(qpsk_ctx *ctx, const uint8_t *d_sym, long long nrows, int nsym, uint8_t *d_packed);
int qpsk_unpack_symbols_host(const uint8_t *h_packed, long long nrows, int nsym, uint8_t *h_sym);
int qpsk_host_alloc(void **h_ptr, size_t bytes);      /* page-locked host memory, usable from every device */
int qpsk_host_free(void *h_ptr);
/* The job's acquisition from outside: every later rx_begin runs qpsk_rx_batch_ext on each shard's slice of h_index [total_frames]
 * int32 and h_seed [total_frames][2] float (phase, freq) -- either may be NULL; both NULL = back to the context's timing.  The slices
 * are uploaded once, here (no slot may be in flight).  A call that fails on any shard leaves every shard with its previous setting;
 * a later qpsk_multi_load clears it. */
int qpsk_multi_set_acquisition(qpsk_multi *mj, const int32_t *h_index, const float *h_seed);
/* Data mode: while on, every rx_begin runs qpsk_rx_batch_data (with the acquisition above, if set) and the rows it gathers (h_sym of
 * rx_end, direct or packed as before) hold the data rule's decisions instead of the slicer's.  No slot may be in flight (QPSK_ERR_STATE). */
int qpsk_multi_set_data(qpsk_multi *mj, int on);
int qpsk_multi_rx_begin(qpsk_multi *mj, int slot);
int qpsk_multi_rx_end(qpsk_multi *mj, int slot, uint8_t *h_sym, float *h_freq, float *h_phase);

/* -------------------------------------------------------------------------
 * Small helpers so that a C host needs nothing but this library.
 * ------------------------------------------------------------------------- */
int qpsk_dev_alloc(qpsk_ctx *ctx, void **d_ptr, size_t bytes);
int qpsk_dev_free(qpsk_ctx *ctx, void *d_ptr);
int qpsk_dev_upload(qpsk_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int qpsk_dev_download(qpsk_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* Self-test hook: order-independent 64-bit hash of the device sin/cos (the glibc-exact routine the
 * Costas kernel uses) over the float bit patterns [first, first+count) in both signs; tests compare
 * it with the same hash of the CPU oracle over the same range. */
int qpsk_selftest_sincos_hash(qpsk_ctx *ctx, uint32_t first, uint32_t count, unsigned long long *h_out);

/* Test hook (the stream error paths, tests/test_gpu_parity.py): stores `code` in the context's kernel status word, as a kernel that gave
 * up (1), left the bounded phase range (2) or ended on a non-finite loop state (3) would; the context's next synchronising call reports it. */
int qpsk_test_inject_status(qpsk_ctx *ctx, int code);
/* Test hook (the one-pass histogram route): synchronises, then out[5] = {the guess the next histogram-mode call will take (-1: none), frames
 * the last one-pass call's guess missed, and the statistics the host steers by: majority index, frames, frames off the majority or missed by the guess} */
int qpsk_test_hist_state(qpsk_ctx *ctx, int32_t *out);
/* Test hook (the full-rate filter's multi-tile runs, tests/test_fir_runs_gpu.py): out[3] = {ntiles, parts, tpp} -- how rrc_fir_stream_kernel, the
 * kernel behind qpsk_rrc_fir_batch for a symmetric filter, would cut nframes delay lines of `length` samples on this context's device: a frame
 * is ntiles 512-output tiles in parts runs of tpp consecutive tiles, one wave per run.  Host arithmetic only: no device work, and
 * qpsk_ctx_last_kernel() stays.  QPSK_ERR_ARG for a NULL pointer, nframes < 1 or length < 1. */
int qpsk_test_fir_runs(qpsk_ctx *ctx, int nframes, int length, int32_t out[3]);
/* Test hook (the chunk loops of the decoder's scratch route): *out = the decode launches of the context's last qpsk_viterbi_batch,
 * qpsk_viterbi_punct_batch, qpsk_viterbi_ilv_batch or qpsk_deframer_push_coded call -- 1 with the decision words in LDS, 0 for a push whose bytes, crc_ok and
 * info were all NULL, or for a call that was refused.  Host bookkeeping only: no synchronisation, no device work. */
int qpsk_test_viterbi_launches(qpsk_ctx *ctx, int *out);
/* Test hook (stream positions beyond 32 bits): synchronises the context's stream, then adds delta to every stream's position counters
 * (dibits pushed, where the hunt resumes, the pending packet's position) in either deframer mode; the carried tail, the pending body and
 * the pending packet's rotation, score and fill stay.  Later packets are reported with pos + delta, everything else as without the
 * call.  QPSK_ERR_ARG for delta < 0 or delta > 2^62; QPSK_ERR_STATE before a reset, after a failed push, or while a stream has seen fewer
 * than nsync - 1 dibits. */
int qpsk_test_deframer_advance(qpsk_ctx *ctx, long long delta);
/* Test hook (stream positions beyond 32 bits, VITERBI STREAM): synchronises the context's stream, then adds delta to the streaming decoder's
 * position counters; metrics, pending pairs and the ring stay.  Everything after it comes out as without the call.  QPSK_ERR_ARG for
 * delta < 0, delta > 2^62 or a delta that is no multiple of the window; QPSK_ERR_STATE before a reset or while total < depth + window. */
int qpsk_test_viterbi_stream_advance(qpsk_ctx *ctx, long long delta);
/* Test hook (positions beyond 32 bits, OUTER LINK): synchronises the context's stream, then moves the outer link's position counter on by
 * delta; the lock, the words in flight and the ring stay.  Later words are reported with pos + delta, everything else as without the call.
 * QPSK_ERR_ARG for delta < 0, delta > 2^62 or a delta that is no multiple of 8; QPSK_ERR_STATE before a reset. */
int qpsk_test_outer_advance(qpsk_ctx *ctx, long long delta);

#ifdef __cplusplus
}
#endif
#endif /* QPSK_HIP_H */
