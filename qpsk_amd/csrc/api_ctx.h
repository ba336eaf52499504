/*
 * api_ctx.h -- what the units of the C ABI layer share: the context, its groups of state, error reporting, the checks of buffer
 * arguments (Span, overlap, rows_extent, first_overlap, pitch_ok) and the few helpers that cross a unit boundary.  Internal: included
 * by api_*.cpp only, never installed.
 *
 *   api_ctx.cpp      contexts, tuning, the status word, setters and getters, device memory
 *   api_rx.cpp       the receive batch calls, their routing and the stage calls
 *   api_streams.cpp  the running streams and the transmit side
 *   api_coded.cpp    soft decisions, the convolutional code, Reed-Solomon
 *   api_packets.cpp  bit stages, the deframers, the framer
 *   api_vstream.cpp  the streaming Viterbi decoder and the encoder that carries its register
 *   api_outer.cpp    the outer link behind it: word sync, the byte deinterleaver and the interleaver
 *   api_dispersal.cpp DVB's energy dispersal behind the Reed-Solomon decoder
 *   api_nodesync.cpp the node sync in front of it: the candidate transform and the monitor on the decoder's error count
 *   api_cross.cpp    the packet erasure code: Reed-Solomon across the packets of a group, and the place call in front of it
 *   api_channel.cpp  the polyphase channeliser in front of the streams: one wideband capture into stream rows; the synthesis bank, its
 *                    transmit twin
 *   api_resample.cpp the batched rational resampler between the capture's rate and the modem's
 *
 * OWNERSHIP: each nested group of qpsk_ctx below names the one unit that reads and writes it; the members outside a group
 * (configuration, scratch buffers) are every unit's.  DESIGN.md, "The host layer", lists the few places that reach across.
 * The entry points take their C linkage from their declarations in include/qpsk_hip.h.
 */
#ifndef QPSK_API_CTX_H
#define QPSK_API_CTX_H

#include "../../include/qpsk_hip.h"
#include "host_math.h"
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <initializer_list>
#include <map>
#include <vector>

struct qpsk_ctx;

namespace qpsk {

/* the calling thread's error text (qpsk_last_error) and the code, for `return fail(...)` */
QPSK_UNIT_LOCAL int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(QPSK_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define KERNEL_TRY(expr)                                                                      \
    do {                                                                                      \
        (void)hipGetLastError(); /* a stale error of an unrelated earlier call must not be blamed on this launch */ \
        int e_ = (expr);                                                                      \
        if (e_ != 0)                                                                          \
            return fail(QPSK_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString((hipError_t)e_), __FILE__, __LINE__); \
    } while (0)

struct QPSK_UNIT_LOCAL DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    void release() { hipFree(p); *this = DevBuf(); }      /* behind a synchronisation of every stream that used it */
};

/*
 * Tuning: choices that select WHICH kernel geometry computes a result, never the result (every geometry is bit-exact
 * against the oracle; tests/test_gpu_parity.py runs them all).  -1 = the library's own choice.  The QPSK_* environment
 * variables of the same names are read ONCE, in qpsk_ctx_create(); qpsk_ctx_set_tuning() overrides them per context.
 * Nothing on a call path reads the environment.
 */
struct Tuning {
    int fused_g = -1, fused_s = -1, fused_lds = -1;   /* generic chunked kernel: frames per workgroup, symbols per chunk, LDS budget */
    int generic = -1;                                 /* 1: the barrier-synchronised generic kernels instead of the pipeline */
    int pipe_nf = -1;                                 /* rx_fused_pipe_kernel: FIR waves per workgroup */
    int pipe_v = -1, pipe_g = -1;                     /* 1: rx_fused_pipe_kernel, 2: rx_pipe2_kernel; frames per workgroup of the latter */
    int layout_lo = -1, layout_hi = -1;               /* rx_pipe2_kernel: units per hardware wave, 4 bits each (waves 1-5 / 6-11) */
    int pipe_variant = -1;                            /* pipeline kernel: layout bits (kernels.h, FusedArgs::dbg) */
    int hist_generic = -1;                            /* histogram estimate: 1 = rrc_fir + scan kernels (no fused scan), 2 = those with the generic scan */
    int fir_generic = -1;                             /* full-rate rrc_fir(): 1 = the compiler-scheduled rrc_fir_kernel also for symmetric taps */
    int stream_scan = -1;                             /* streams from PCM, histogram timing: 1 = stream_scan_kernel (mixer + filter + scan) whatever the stream count, 0 = never */
    int stream_poll = -1;                             /* qpsk_streams_rx_pcm_host on the one-launch kernel: 0 = wait with hipStreamSynchronize instead of watching the kernel's counter */
    int stream_block = -1;                            /* streams: 0 = never the one-launch-per-block kernel (streamblock.hip), 1 = whenever the shape allows, unset: by samples per block of all streams (stream_block_ok: 3.5 M for PCM, 0.4 M for complex input at CYCLES 8) */
    int stream_carrier = -1;                          /* stream_scan_kernel on PCM: 0 = every stream runs its own carrier (mixer wave) even while all streams share one */
    int lean_dma = -1;                                /* rx_lean_kernel: 0 = window staging through registers even where LDS-DMA applies (even decimation offsets), 2 = LDS-DMA with one window per FIR wave */
    int hist_onepass = -1;                            /* histogram timing: 0 = never the one-pass route (rx_hist_kernel on the previous batch's majority index + a fall-back pass), 1 = whenever the shape allows and a guess exists (unset: only while every frame of the last batch sat on its majority index) */
    int est_waves = -1;                               /* rx_lean_kernel, in-launch FFT estimate: hardware waves launched for it */
    int lean_pair = -1;                               /* rx_lean_kernel: 0 = one lane per loop in the serial wave, 1 = two lanes per loop up to 16 frames per workgroup, 2 = up to 32; unset: up to 24, where it pays in steady state (profiles/r06_step_cost.txt) */
    int viterbi_lds = -1;                             /* qpsk_viterbi_batch: 0 = decision words always through the global scratch buffer, 1 = in LDS whenever a row's fit (unset: in LDS where every row of the call is resident at once) */
    int fft_fused = -1;                               /* FFT timing estimate: 0 = always a launch of its own (1 / unset: inside rx_fused_pipe_kernel's launch for full workgroups) */
    int viterbi_chunk_rows = -1;                      /* both Viterbi calls and the coded deframer's decode on the scratch route: at most this many rows per launch, where that is fewer than VITERBI_SCRATCH_MAX allows (>= 1; 0 is refused) */
};

static inline int tuned(int v, int dflt) { return v >= 0 ? v : dflt; }

/* ---- buffer arguments: what the entry points ask of the byte ranges they are handed.  The one place with interval arithmetic on pointers */

/* a byte range of a call under its argument's name; p = NULL is an optional buffer that is absent */
struct Span {
    const void *p;
    size_t bytes;
    const char *name;
};

/* do the two share a byte?  An absent or an empty range shares none */
static inline bool overlap(const Span &a, const Span &b)
{
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && a.bytes && b.bytes && x < y + b.bytes && y < x + a.bytes;
}

/* [rows][pitch] of which row_bytes count: from the first row's first byte to the last row's last; what lies behind that is not the buffer's */
static inline size_t rows_extent(long long rows, size_t pitch, long long row_bytes) { return (size_t)(rows - 1) * pitch + (size_t)row_bytes; }

/* no two of s[0 .. count) may share a byte: the refusal for the first pair that does, the later one named first, or QPSK_OK */
static inline int first_overlap(const char *who, const Span *s, size_t count)
{
    for (size_t i = 0; i < count; i++)
        for (size_t j = i + 1; j < count; j++)
            if (overlap(s[i], s[j])) return fail(QPSK_ERR_ARG, "%s: %s overlaps %s", who, s[j].name, s[i].name);
    return QPSK_OK;
}

/* the Reed-Solomon calls' limit for pitch_ok: the largest pitch with which `rows` rows stay inside 62 bits */
static inline long long rs_pitch_limit(long long rows) { return (LLONG_MAX >> 1) / rows; }

/* a pitch argument: 0 = tight, otherwise at least the row and at most `limit` (the caller's, from its row count; LLONG_MAX where it has its
 * own refusal for that).  *out = the pitch in force, also behind `false`, for the caller's message */
static inline bool pitch_ok(long long pitch, long long row, long long limit, size_t *out)
{
    *out = (size_t)(pitch ? pitch : row);
    return pitch == 0 || (pitch >= row && pitch <= limit);
}

/* ---- the context's groups of state, one per owner.  Plain structs: each frees and clears what it holds in release() */

/* Status word, in pinned host memory that the device can write: a kernel stores a nonzero STATUS_* there when
 * its results are invalid (its in-LDS pipeline exhausted the bounded spins; a loop phase beyond the bounded
 * 2 pi wrap).  The host looks at it after EVERY synchronisation the library performs (check_status), so no
 * entry point that hands results to the caller can return QPSK_OK over invalid ones.  Every unit passes d_status to its launches;
 * api_ctx.cpp allocates, reads and frees it */
struct StatusWord {
    int *h_status = nullptr;     /* host view */
    int *d_status = nullptr;     /* device view of the same word */
};

/* api_rx.cpp.  The one-pass histogram route (rx_hist_kernel): d_hint[0] = the guessed decimation offset = the majority index of the context's last
 * histogram-mode batch (left there by index_majority_kernel, in stream order: no synchronisation), d_hint[1] = the frames the guess
 * missed in the running call; h_hist_stats (pinned, written by that kernel) = {majority, frames, missed} of the last batch whose
 * kernels have completed: the host reads it to stay away from the route while the guess misses many frames */
struct QPSK_UNIT_LOCAL HistGuess {
    int32_t *d_hint = nullptr;
    int32_t *h_hist_stats = nullptr, *d_hist_stats = nullptr;
    bool hint_valid = false;
    void release();
};

/* api_streams.cpp.  The running streams (qpsk_streams_*) */
struct QPSK_UNIT_LOCAL Streams {
    int nstreams = 0;
    float *s_memory = nullptr, *s_dec = nullptr, *s_loop = nullptr, *s_mixer = nullptr;
    /* the streams' carrier while it is ONE carrier (streamscan.hip MODE 2): qpsk_streams_reset() gives every stream the same mixer
     * frequency and starting phase, and the carrier does not depend on the data, so it stays one as long as every PCM block goes
     * through stream_scan_kernel.  s_ctab: two tables of frame_size phases (this block's, the next block's), s_cstate: kernels.h.
     * Any other consumer of s_mixer first gets the per-stream state back (carrier_to_streams) and the sharing ends until the next reset */
    float *s_ctab = nullptr, *s_cstate = nullptr;
    bool carrier_shared = false;
    unsigned carrier_blocks = 0;        /* blocks taken from the tables since the reset (which of the two holds the current one) */
    unsigned carrier_scans = 0;         /* stream_scan_kernel launches among them (its relay counter, kernels.h) */
    float *carrier_pending = nullptr;   /* the table stream_scan_kernel has begun: the loop kernel of the same call finishes it (carrier.h) */
    bool stream_work_unchecked = false; /* a stream call has enqueued kernels whose status word no synchronisation has looked at yet */
    bool streams_poisoned = false;      /* a stream call failed between its launches (or a kernel gave up): carried state is undefined until the next reset */
    /* host-pointer streaming call (qpsk_streams_rx_pcm_host: what the drop-in rx_frame() uses): pinned staging on the
     * host, matching arena on the device; sized for nstreams blocks */
    unsigned char *h_stage = nullptr, *d_stage = nullptr;
    size_t stage_cap = 0;
    /* lives as long as the context (qpsk_ctx_create allocates it, qpsk_ctx_destroy frees it): release() leaves it alone */
    unsigned *h_done = nullptr, *d_done = nullptr;   /* stream_block_kernel's wave counter (mapped pinned memory), host / device view */
    unsigned done_expect = 0;
    /* the carried state is undefined until the next reset: the shared carrier is dropped with it */
    void poison()
    {
        streams_poisoned = true;
        carrier_shared = false;
        carrier_pending = nullptr;      /* points into s_ctab */
    }
    void release();
};

/* api_streams.cpp.  Transmitters (N2) */
struct QPSK_UNIT_LOCAL Transmitters {
    int ntx = 0;
    uint8_t *t_hist = nullptr;    /* [ntx][tx_history_symbols()]: the symbols still inside tx_filter */
    float *t_mixer = nullptr;     /* [ntx][4]: carrier phase and step */
    DevBuf tx_b;                  /* shaped baseband when the caller does not want it */
    void release();
};

/* api_packets.cpp.  Deframer (qpsk_deframer_*): per-stream state (kernels.h, DeframeHeader) and the tables (packed keystream, then the lanes' CRC
 * advance factors at DF_ADV_OFFSET).  Everything but `state` is read only behind the checks of `state`, `coded` and `ready` */
struct QPSK_UNIT_LOCAL Deframer {
    uint8_t *state = nullptr, *tables = nullptr;
    size_t stride = 0;
    int nstreams = 0, nsync = 0, min_score = 0, nbytes = 0, max_packets = 0;
    unsigned long long sync_lo[2] = {0, 0}, sync_hi[2] = {0, 0};
    bool ready = false;           /* a reset has completed and no push has failed since */
    /* the coded mode (qpsk_deframer_reset_coded): the same state with int8 soft pairs as the pending body; the tables are the keystream
     * dibits [nsteps], then the CRC advance factors x^(8 m), m < nbytes, at DFC_ADV_OFFSET.  One deframer per context, in one mode */
    bool coded = false;
    int mode = 0, nsteps = 0;     /* nsteps: the trellis steps of a packet, 8 (nbytes + 2) + 6 */
    int nbody = 0;                /* Nc: a body's dibits on air, coded_ndibits(layout, nsteps) */
    CodedLayout layout;           /* the body's layout; its kind is the reset's (qpsk_deframer_reset_coded / _punct / _ilv), whatever the pattern and the stride */
    float scale = 0.f;
    unsigned crc_init = 0;
    void release();               /* leaves the group value-initialised: no deframer */
};

/* api_packets.cpp.  The framer (qpsk_frame_batch): its own keystream table, ks_len dibits from SEED -- a prefix serves every shorter row and body, so
 * it only ever grows; qpsk_scramble_batch's table (qpsk_ctx::keystream) is another buffer and is left alone */
struct QPSK_UNIT_LOCAL Framer {
    uint8_t *ks = nullptr;
    int ks_len = 0;
    void release();
};

/* api_vstream.cpp.  The streaming Viterbi decoder (qpsk_viterbi_stream_*): per-stream state on the device (viterbi_stream.hip: metrics, pending
 * pairs, the last emitted word, the ring of decision and ballot words); the positions are the same for every stream and are the host's */
struct QPSK_UNIT_LOCAL ViterbiStream {
    uint8_t *state = nullptr;
    size_t stride = 0;
    int nstreams = 0, depth = 0, window = 0;
    Puncture punct = {1, 1u, 1u, 2};
    bool punctured = false;       /* any pattern but (1, 1, 1): viterbi_stream_punct_kernel */
    long long total = 0;          /* trellis steps since the reset or the last flush, qpsk_test_viterbi_stream_advance's delta included */
    long long advanced = 0;       /* the sum of those deltas: the ring is indexed by (total - advanced) / 64 */
    void release();               /* leaves the group value-initialised: no decoder.  Behind a synchronisation of the context's stream */
};

/* api_outer.cpp.  The outer link of a continuous stream (qpsk_outer_*): per-stream state on the device (outer.hip: a header and the ring of raw
 * received bits); every stream is pushed with the same bits, so the bits since the reset are the host's number */
struct QPSK_UNIT_LOCAL OuterLink {
    uint8_t *state = nullptr;
    size_t stride = 0;
    int nstreams = 0, n = 0, branches = 0, sync = 0, lock = 0, drop = 0, flags = 0;
    int group = 0;                /* qpsk_outer_reset_group's G, 0 = no group sync */
    long long total = 0;          /* bits since the reset, qpsk_test_outer_advance's deltas included */
    void release();               /* leaves the group value-initialised: no link.  Behind a synchronisation of the context's stream */
};

/* api_nodesync.cpp.  The node sync in front of the streaming decoder (qpsk_nodesync_*): per-link state on the device (nodesync.hip: the
 * candidate, the monitor's counters and the last nshift - 1 input dibits); every link is pushed with the same dibits, so how many of those
 * history dibits are real is the host's number */
struct QPSK_UNIT_LOCAL NodeSync {
    uint8_t *state = nullptr;
    int nlinks = 0, nrot = 0, nshift = 0, span = 0, settle = 0, thr_num = 0, thr_den = 0, drop = 0;
    int have = 0;                 /* min(dibits since the reset, nshift - 1) */
    void release();               /* leaves the group value-initialised: no node sync.  Behind a synchronisation of the context's stream */
};

/* api_dispersal.cpp.  Energy dispersal (qpsk_dispersal_batch): the table of the last (len, group, flags), group rows of
 * dispersal_table_pitch(len) bytes; rebuilt, behind a synchronisation of the context's stream, when a call names another triple */
struct QPSK_UNIT_LOCAL Dispersal {
    uint8_t *table = nullptr;     /* DISPERSAL_MAX_GROUP * 256 bytes: every triple fits */
    int len = 0, group = 0, flags = 0;
    void release();               /* leaves the group value-initialised: no table.  Behind a synchronisation of the context's stream */
};

/* What the three polyphase stages' groups share: one allocation (`state`) that begins with the taps and holds TWO histories -- a push reads
 * hist[cur] and leaves the next history in the other, so no launch reads what it writes.  polyphase_reset fills one; a push is
 * begin_push(), the stage's launches, polyphase_end_push (below) */
struct QPSK_UNIT_LOCAL PolyphaseState {
    uint8_t *state = nullptr;
    float *proto = nullptr, *hist[2] = {nullptr, nullptr};      /* into state; hist: NULL where the stage has none */
    int cur = 0;
    bool ready = false;           /* a reset has completed and no push has failed since */
    /* a push begins: the history its launches read.  Not ready until polyphase_end_push: a push that fails between the two ends the stage */
    const float2 *begin_push() { ready = false; return reinterpret_cast<const float2 *>(hist[cur]); }
    float2 *flip() { return reinterpret_cast<float2 *>(hist[cur ^= 1]); }      /* the other history, from now on the current one */
    void release() { hipFree(state); *this = PolyphaseState(); }               /* behind a synchronisation of the context's stream */
};

/* api_channel.cpp.  The polyphase channeliser (qpsk_channel_*): behind the prototype the state holds the transform's table and the
 * selection; the histories are (P - 1) M samples, none at P = 1 */
struct QPSK_UNIT_LOCAL Channeliser : PolyphaseState {
    int M = 0, P = 0, nsel = 0;
    float *tw = nullptr;          /* into state */
    int32_t *chan = nullptr;
    void release() { PolyphaseState::release(); *this = Channeliser(); }      /* leaves the group value-initialised: no channeliser */
};

/* api_channel.cpp.  The polyphase synthesis bank (qpsk_synth_*): the channeliser's state under the transmit bank's meaning -- the histories
 * are the last P - 1 TRANSFORMED vectors, (P - 1) M values, and the selection holds distinct channels -- and the scratch of V rows between
 * the bank's two launches, sized by the largest push so far.  Separate from qpsk_ctx::channel: both banks are live in one context */
struct QPSK_UNIT_LOCAL Synthesiser {
    Channeliser bank;
    DevBuf scratch;               /* V [T][M][2] floats of the running push */
    void release() { bank.release(); scratch.release(); }      /* no bank, no scratch.  Behind a synchronisation of the context's stream */
};

/* api_resample.cpp.  The batched rational resampler (qpsk_resample_*): the L P taps and histories of the last P consumed samples per
 * stream.  The position r = n0 D - c0 L (0 after a reset, then in [D - L, D)) is the same for every stream and is the host's */
struct QPSK_UNIT_LOCAL Resampler : PolyphaseState {
    int nstreams = 0, L = 0, D = 0, P = 0;
    int r = 0;
    void release() { PolyphaseState::release(); *this = Resampler(); }      /* leaves the group value-initialised: no resampler */
};

} // namespace qpsk

struct qpsk_ctx {
    int device = 0;
    qpsk::Tuning tune;
    int ncu = 256;                /* compute units of the device (256 on MI355X) */
    const char *last_kernel = ""; /* the kernel the last rx batch (or qpsk_rrc_fir_batch, ...) launched (qpsk_ctx_last_kernel) */
    int viterbi_launches = 0;     /* decode launches of the last qpsk_viterbi_batch / _punct_batch / _ilv_batch / qpsk_deframer_push_coded (qpsk_test_viterbi_launches) */
    bool taps_symmetric = false;  /* taps[k] == taps[126 - k] bit for bit: rx_lean_kernel keeps the 64 distinct ones in SGPRs */
    hipStream_t stream = nullptr; /* caller's stream; nullptr = default stream */
    qpsk_params prm{};
    int cycles = 0, nsym = 0;
    float taps[QPSK_NTAPS];
    float damping = 0.f, alpha = 0.f, beta = 0.f;
    float min_freq = 0.f, max_freq = 0.f;
    float *d_taps = nullptr;     /* 128 floats */
    float *d_gains = nullptr;    /* MAX_BW x (alpha, beta) */
    std::vector<float> h_gains;
    /* scratch that several units use: what a buffer holds means nothing once the call that filled it has returned
     * (qpsk_ctx_destroy releases every one of them: a new one goes into its list) */
    qpsk::DevBuf index, filtered, mixed, keystream, sympad, mislist;
    qpsk::DevBuf datacostas;      /* qpsk_rx_batch_data off rx_lean_kernel: the costas_frame[] the data rule is taken from */
    qpsk::DevBuf vitdec;          /* qpsk_viterbi_batch off the LDS route: the decision words between the forward pass and the trace-back */
    qpsk::DevBuf softgain;        /* qpsk_soft_batch on rows beyond the one-pass bound: the gain per row, between the two passes */
    qpsk::DevBuf dfstage;         /* the soft rows of the packets a coded push completes, between the hunt and the decode */
    int keystream_len = 0;
    std::map<int, double *> twiddles;
    float *d_fast = nullptr;      /* qpsk_rrc_fir_batch_fast: H[512][2] then tw[512][2]; rebuilt when the taps change */
    bool fast_valid = false;
    /* ---- state with one owner */
    qpsk::StatusWord status;
    qpsk::HistGuess hist;
    qpsk::Streams streams;
    qpsk::Transmitters tx;
    qpsk::Deframer df;
    qpsk::Framer framer;
    qpsk::ViterbiStream vs;
    qpsk::OuterLink outer;
    qpsk::NodeSync nodesync;
    qpsk::Dispersal dispersal;
    qpsk::Channeliser channel;
    qpsk::Synthesiser synth;
    qpsk::Resampler resample;
};

namespace qpsk {

static const int MAX_BW = 64;

/* ---- api_ctx.cpp */
QPSK_UNIT_LOCAL int ensure(qpsk_ctx *c, DevBuf &b, size_t bytes);
/* after a synchronisation of the context's stream: did a kernel of the calls just completed flag its results? */
QPSK_UNIT_LOCAL int check_status(qpsk_ctx *c);
QPSK_UNIT_LOCAL int bind(const qpsk_ctx *c);
/* make d_gains[0] the context's own (alpha, beta) again after a bandwidth sweep replaced it */
QPSK_UNIT_LOCAL int use_context_gains(qpsk_ctx *c);
/* for a reset that replaces per-stream device state (who: the entry point, noun: what `count` counts, "streams" or "links"): *state = count
 * x stride new bytes, allocated FIRST, so that a failure leaves the context and the state it has as they were, and handed over behind a
 * synchronisation of the context's stream, because pushes of the old state may still run.  The caller then release()s the old group,
 * assigns the new one and launches its init kernel */
QPSK_UNIT_LOCAL int replace_state(qpsk_ctx *c, const char *who, const char *noun, int count, size_t stride, uint8_t **state);
/* for a reset of a polyphase stage (who: the entry point): are the n taps finite ... */
QPSK_UNIT_LOCAL int taps_finite(const char *who, const float *h_proto, size_t n);
/* ... and, behind the stage's own checks of its arguments, the new state in *fresh, a group of the caller's own that holds nothing yet:
 * nhead floats of h_head (the taps first), rounded up to a whole complex value, two zeroed histories of nhist floats each, ntail bytes of
 * h_tail; sizes: the stage's own, for the allocation's refusal.  Refuses a NULL context; allocates FIRST, so that a failure leaves the
 * stage the context has as it was; uploads behind a synchronisation of the context's stream, because pushes on the old state may still
 * run.  The caller then sets its own members in *fresh, release()s the context's group and assigns the new one */
QPSK_UNIT_LOCAL int polyphase_reset(qpsk_ctx *c, PolyphaseState *fresh, const char *who, const char *sizes, const float *h_head, size_t nhead,
                                    size_t nhist, const void *h_tail, size_t ntail);
/* behind a push's launches on st.begin_push() (`kernel`: the name qpsk_ctx_last_kernel reports): unless K = 0 or the stage has no history
 * (n = 0), polyphase_history_kernel leaves the last n of every row's (history, in [K]) in the other history, which becomes the current
 * one; the stage is ready again */
QPSK_UNIT_LOCAL int polyphase_end_push(qpsk_ctx *c, PolyphaseState &st, const char *kernel, const float2 *in, size_t in_pitch, size_t K, int rows,
                                       size_t n);

/* ---- api_rx.cpp, for the streams' kernels apart */
QPSK_UNIT_LOCAL int fir_full_rate(qpsk_ctx *c, const float *x, const float *memory, float *y, int nframes, int length, size_t in_pitch = 0);
QPSK_UNIT_LOCAL int fft_timing_indices(qpsk_ctx *c, const float *d_in, int nframes, int32_t *d_index, float *d_y = nullptr,
                                       double *d_X = nullptr, size_t pitch = 0, double *d_bin = nullptr);
QPSK_UNIT_LOCAL int costas_over_symbols(qpsk_ctx *c, float *d_symbols, int nframes, int nsym, int dstride, float *d_state,
                                        uint8_t *d_sym, float *d_costas, const float *refill = nullptr,
                                        const int32_t *refill_index = nullptr, bool refill_planar = false);

/* ---- api_coded.cpp, for the coded deframer and the framer */
/* a pattern as the entry points take it */
struct Pattern {
    int period;
    uint32_t keep0, keep1;
};
QPSK_UNIT_LOCAL int layout_add_pattern(const char *who, const Pattern *pattern, CodedLayout *l);
QPSK_UNIT_LOCAL int layout_add_stride(const char *who, int nsteps, const int *stride, CodedLayout *l);
/* the rule for `rows` rows of nsteps steps, whatever their layout: per_row = the decision words' bytes; chunk_rows = rows per launch, what
 * VITERBI_SCRATCH_MAX allows (one row at least), on the scratch route fewer where QPSK_VITERBI_CHUNK_ROWS says so -- the key can only lower
 * the cap, so the scratch buffer never grows by it */
struct ViterbiRoute {
    size_t per_row;
    bool lds;
    size_t chunk_rows;
};
QPSK_UNIT_LOCAL ViterbiRoute viterbi_route(const qpsk_ctx *c, size_t rows, int nsteps);

} // namespace qpsk

#endif
