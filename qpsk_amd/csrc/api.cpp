/*
 * api.cpp -- the C ABI of include/qpsk_hip.h: contexts, argument checking,
 * scratch management and kernel sequencing.  No arithmetic of the receive
 * path happens here: per-configuration numbers come from host_math.c (as in
 * the reference, on the host), everything per sample runs in kernels.hip.
 * There is deliberately no CPU fallback: without a usable GPU every entry
 * point fails with QPSK_ERR_NO_DEVICE / QPSK_ERR_HIP.
 */
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

using namespace qpsk;

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

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

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
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

static const struct { const char *name; int Tuning::*field; } TUNING_KEYS[] = {
    {"QPSK_FUSED_G", &Tuning::fused_g},       {"QPSK_FUSED_S", &Tuning::fused_s},     {"QPSK_FUSED_LDS", &Tuning::fused_lds},
    {"QPSK_FUSED_GENERIC", &Tuning::generic}, {"QPSK_PIPE_NF", &Tuning::pipe_nf},
    {"QPSK_PIPE_DBG", &Tuning::pipe_variant}, {"QPSK_HIST_GENERIC", &Tuning::hist_generic},
    {"QPSK_PIPE_V", &Tuning::pipe_v},         {"QPSK_PIPE_G", &Tuning::pipe_g},
    {"QPSK_PIPE_LAYOUT_LO", &Tuning::layout_lo}, {"QPSK_PIPE_LAYOUT_HI", &Tuning::layout_hi},
    {"QPSK_FIR_GENERIC", &Tuning::fir_generic}, {"QPSK_FFT_FUSED", &Tuning::fft_fused},
    {"QPSK_STREAM_BLOCK", &Tuning::stream_block}, {"QPSK_STREAM_POLL", &Tuning::stream_poll},
    {"QPSK_STREAM_SCAN", &Tuning::stream_scan}, {"QPSK_STREAM_CARRIER", &Tuning::stream_carrier},
    {"QPSK_LEAN_DMA", &Tuning::lean_dma},     {"QPSK_LEAN_PAIR", &Tuning::lean_pair},
    {"QPSK_EST_WAVES", &Tuning::est_waves},   {"QPSK_HIST_ONEPASS", &Tuning::hist_onepass},
    {"QPSK_VITERBI_LDS", &Tuning::viterbi_lds},   {"QPSK_VITERBI_CHUNK_ROWS", &Tuning::viterbi_chunk_rows},
};

/* layout bits a product build honours: 4 no spare waves, 8 C++ Costas step, 64/128 lane-mapping variants.  The
 * result-changing ablation bits (1 skip the filter arithmetic, 2 skip the recurrence) and the cycle accounting (32)
 * exist only in the measurement build (make profile, -DQPSK_PIPE_PROFILE) */
#ifdef QPSK_PIPE_PROFILE
static const int PIPE_VARIANT_MASK = ~0;
#else
static const int PIPE_VARIANT_MASK = 4 | 8 | 16 | 64 | 128 | 256 | 512 | 1024 | 8192;
#endif

struct qpsk_ctx {
    int device = 0;
    Tuning tune;
    int ncu = 256;                /* compute units of the device (256 on MI355X) */
    const char *last_kernel = ""; /* the receive kernel the last rx batch launched (qpsk_ctx_last_kernel) */
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
    /* Status word, in pinned host memory that the device can write: a kernel stores a nonzero STATUS_* there when
     * its results are invalid (its in-LDS pipeline exhausted the bounded spins; a loop phase beyond the bounded
     * 2 pi wrap).  The host looks at it after EVERY synchronisation the library performs (check_status), so no
     * entry point that hands results to the caller can return QPSK_OK over invalid ones. */
    unsigned *h_done = nullptr, *d_done = nullptr;   /* stream_block_kernel's wave counter (mapped pinned memory), host / device view */
    unsigned done_expect = 0;
    int *h_status = nullptr;     /* host view */
    int *d_status = nullptr;     /* device view of the same word */
    std::vector<float> h_gains;
    DevBuf index, filtered, mixed, keystream, sympad, mislist;
    DevBuf datacostas;            /* qpsk_rx_batch_data off rx_lean_kernel: the costas_frame[] the data rule is taken from */
    DevBuf vitdec;                /* qpsk_viterbi_batch off the LDS route: the decision words between the forward pass and the trace-back */
    DevBuf softgain;              /* qpsk_soft_batch on rows beyond the one-pass bound: the gain per row, between the two passes */
    /* the one-pass histogram route (rx_hist_kernel): d_hint[0] = the guessed decimation offset = the majority index of the context's last
     * histogram-mode batch (left there by index_majority_kernel, in stream order: no synchronisation), d_hint[1] = the frames the guess
     * missed in the running call; h_hist_stats (pinned, written by that kernel) = {majority, frames, missed} of the last batch whose
     * kernels have completed: the host reads it to stay away from the route while the guess misses many frames */
    int32_t *d_hint = nullptr;
    int32_t *h_hist_stats = nullptr, *d_hist_stats = nullptr;
    bool hint_valid = false;
    int keystream_len = 0;
    std::map<int, double *> twiddles;
    float *d_fast = nullptr;      /* qpsk_rrc_fir_batch_fast: H[512][2] then tw[512][2]; rebuilt when the taps change */
    bool fast_valid = false;
    /* streams */
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
    /* transmitters (N2) */
    int ntx = 0;
    uint8_t *t_hist = nullptr;    /* [ntx][tx_history_symbols()]: the symbols still inside tx_filter */
    float *t_mixer = nullptr;     /* [ntx][4]: carrier phase and step */
    DevBuf tx_b;                  /* shaped baseband when the caller does not want it */
    /* deframer (qpsk_deframer_*): per-stream state (kernels.h, DeframeHeader) and the tables (packed keystream, then the lanes' CRC
     * advance factors at DF_ADV_OFFSET) */
    uint8_t *df_state = nullptr, *df_tables = nullptr;
    size_t df_stride = 0;
    int df_nstreams = 0, df_nsync = 0, df_min_score = 0, df_nbytes = 0, df_max_packets = 0;
    unsigned long long df_sync_lo[2] = {0, 0}, df_sync_hi[2] = {0, 0};
    bool df_ready = false;        /* a reset has completed and no push has failed since */
    /* the coded mode (qpsk_deframer_reset_coded): the same state with int8 soft pairs as the pending body; the tables are the keystream
     * dibits [nsteps], then the CRC advance factors x^(8 m), m < nbytes, at DFC_ADV_OFFSET.  One deframer per context, in one mode */
    bool df_coded = false;
    int df_mode = 0, df_nsteps = 0;      /* df_nsteps: the trellis steps of a packet, 8 (nbytes + 2) + 6 */
    int df_nbody = 0;             /* Nc: a body's dibits on air, coded_ndibits(df_layout, df_nsteps) */
    CodedLayout df_layout;        /* the body's layout; its kind is the reset's (qpsk_deframer_reset_coded / _punct / _ilv), whatever the pattern and the stride */
    float df_scale = 0.f;
    unsigned df_crc_init = 0;
    DevBuf dfstage;               /* the soft rows of the packets a coded push completes, between the hunt and the decode */
    /* the framer (qpsk_frame_batch): its own keystream table, frame_ks_len dibits from SEED -- a prefix serves every shorter row and body, so
     * it only ever grows; qpsk_scramble_batch's table (keystream, above) is another buffer and is left alone */
    uint8_t *frame_ks = nullptr;
    int frame_ks_len = 0;
};

static const int MAX_BW = 64;

static int ensure(qpsk_ctx *c, DevBuf &b, size_t bytes)
{
    if (b.cap >= bytes) return QPSK_OK;
    if (b.p) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(QPSK_ERR_ALLOC, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    }
    b.cap = bytes;
    return QPSK_OK;
}

/* after a synchronisation of the context's stream: did a kernel of the calls just completed flag its results? */
static int check_status(qpsk_ctx *c)
{
    const int st = __atomic_exchange_n(c->h_status, 0, __ATOMIC_ACQ_REL);
    if (st != STATUS_PIPE_TIMEOUT) c->stream_work_unchecked = false;
    if (st == STATUS_PIPE_TIMEOUT) {
        /* a kernel gave up a bounded wait.  Running streams are affected only if a STREAM call has enqueued work since the status word was
         * last looked at (device-pointer stream calls do not synchronise: their kernels' verdict arrives here, through whichever call
         * synchronises next); a batch call's timeout with no stream work in flight leaves the streams' carried state alone (ADVICE r5:
         * this function used to poison them for any call) */
        if (c->nstreams > 0 && c->stream_work_unchecked) {
            c->streams_poisoned = true;
            c->carrier_shared = false;
            c->carrier_pending = nullptr;
        }
        c->stream_work_unchecked = false;
        return fail(QPSK_ERR_HIP, "pipeline kernel: producer/consumer wait timed out; results of the calls since the last synchronisation are invalid");
    }
    if (st == STATUS_PHASE_RANGE)
        return fail(QPSK_ERR_RANGE, "Costas loop phase beyond the bounded 2 pi wrap (input amplitude far outside the modem's range; "
                                    "the reference's phase_wrap() would spin or hang, costas_loop.c:61-67); results of the calls since the last synchronisation are invalid");
    if (st == STATUS_BAD_INDEX)
        return fail(QPSK_ERR_ARG, "an external timing offset (qpsk_rx_batch_ext d_index_in) lies outside 0..%d: the kernel demodulated that frame "
                                  "at offset 0; results of the calls since the last synchronisation are invalid", MAX_INDEX);
    if (st == STATUS_EST_NONFINITE)
        return fail(QPSK_ERR_RANGE, "qpsk_carrier_est_batch: a NaN / Inf sample inside the window the estimate reads; results of the calls since "
                                    "the last synchronisation are invalid");
    if (st == STATUS_SOFT_NONFINITE)
        return fail(QPSK_ERR_RANGE, "qpsk_soft_batch / qpsk_deframer_push_coded: a NaN / Inf sample among those a row's sums or soft output use, or a NaN / Inf gain; "
                                    "results of the calls since the last synchronisation are invalid");
    if (st == STATUS_SOFT_BAD_LAG)
        return fail(QPSK_ERR_ARG, "qpsk_soft_batch: a lag in d_lag is negative or puts the payload beyond the row (that row's soft output is zeros); "
                                  "results of the calls since the last synchronisation are invalid");
    if (st == STATUS_NONFINITE)
        return fail(QPSK_ERR_RANGE, "a Costas loop ended on a NaN / Inf state: the input held a non-finite sample (the reference hangs in phase_wrap() "
                                    "on an infinite phase, costas_loop.c:61-67); results of the calls since the last synchronisation are invalid");
    if (st != 0) return fail(QPSK_ERR_HIP, "kernel status %d", st);
    return QPSK_OK;
}

/* test hook (tests/test_gpu_parity.py, the stream error paths): stores a kernel status code in the context's status word as a kernel
 * that gave up would; the next synchronising call of the context reports it */
int qpsk_test_inject_status(qpsk_ctx *c, int code)
{
    if (!c || !c->h_status) return fail(QPSK_ERR_ARG, "null context");
    __atomic_store_n(c->h_status, code, __ATOMIC_RELEASE);
    return QPSK_OK;
}

/* test hook: the one-pass histogram route's books after a synchronisation -- out[0] = the guess the next call will take (-1: none), out[1] = frames
 * the last one-pass call's guess missed, out[2..4] = the statistics the host reads (majority, frames, missed) */
int qpsk_test_hist_state(qpsk_ctx *c, int32_t *out)
{
    if (!c || !out) return fail(QPSK_ERR_ARG, "null argument");
    out[0] = out[1] = out[2] = out[3] = out[4] = -1;
    if (!c->d_hint) return QPSK_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int32_t h[2];
    HIP_TRY(hipMemcpy(h, c->d_hint, sizeof h, hipMemcpyDeviceToHost));
    out[0] = c->hint_valid ? h[0] : -1;
    out[1] = h[1];
    out[2] = c->h_hist_stats[0]; out[3] = c->h_hist_stats[1]; out[4] = c->h_hist_stats[2];
    return QPSK_OK;
}

static int bind(const qpsk_ctx *c)
{
    HIP_TRY(hipSetDevice(c->device));
    return QPSK_OK;
}

/* make d_gains[0] the context's own (alpha, beta) again after a bandwidth sweep replaced it */
static int use_context_gains(qpsk_ctx *c)
{
    const float g[2] = {c->alpha, c->beta};
    if (c->h_gains.size() != 2 || c->h_gains[0] != g[0] || c->h_gains[1] != g[1]) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->h_gains.assign(g, g + 2);
        HIP_TRY(hipMemcpyAsync(c->d_gains, c->h_gains.data(), sizeof g, hipMemcpyHostToDevice, c->stream));
    }
    return QPSK_OK;
}

extern "C" {

const char *qpsk_last_error(void) { return g_err; }
const char *qpsk_version(void) { return "qpsk_hip 0.3 (gfx950)"; }

int qpsk_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void qpsk_params_default(qpsk_params *p)
{
    if (!p) return;
    p->fs = 9600.0;
    p->rs = 2400.0;
    p->frame_size = 512;
    p->rrc_alpha = .35f;
    p->loop_bw = (float)(2.0 * 3.14159265358979323846 / 100.0f); /* (TAU / 100.0f), qpsk.c:302 */
    p->min_freq = -1.0f;
    p->max_freq = 1.0f;
    p->timing_mode = QPSK_TIMING_HIST;
    p->fixed_index = 0;
}

static int upload_config(qpsk_ctx *c)
{
    float t128[128];
    memset(t128, 0, sizeof t128);
    memcpy(t128, c->taps, sizeof c->taps);
    c->taps_symmetric = true;
    for (int k = 0; k < QPSK_NTAPS / 2; k++)
        if (memcmp(&c->taps[k], &c->taps[QPSK_NTAPS - 1 - k], sizeof(float)) != 0) c->taps_symmetric = false;
    HIP_TRY(hipMemcpyAsync(c->d_taps, t128, sizeof t128, hipMemcpyHostToDevice, c->stream));
    const float g[2] = {c->alpha, c->beta};
    c->h_gains.assign(g, g + 2);
    HIP_TRY(hipMemcpyAsync(c->d_gains, c->h_gains.data(), sizeof g, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QPSK_OK;
}

int qpsk_ctx_create(qpsk_ctx **out, int device, const qpsk_params *p, void *stream)
{
    if (!out || !p) return fail(QPSK_ERR_ARG, "qpsk_ctx_create: null argument");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(QPSK_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail(QPSK_ERR_NO_DEVICE, "device %d out of range (%d devices)", device, ndev);
    if (!(p->fs > 0.0) || !(p->rs > 0.0) || p->frame_size <= 0)
        return fail(QPSK_ERR_ARG, "fs, rs and frame_size must be positive");
    const int cycles = (int)(p->fs / p->rs); /* qpsk.h:21 */
    if (cycles < 1 || cycles > 64) return fail(QPSK_ERR_ARG, "CYCLES = (int)(fs/rs) = %d out of range 1..64", cycles);
    if (p->frame_size % cycles != 0)
        return fail(QPSK_ERR_ARG, "frame_size %d is not a multiple of CYCLES %d", p->frame_size, cycles);
    if (p->timing_mode < QPSK_TIMING_HIST || p->timing_mode > QPSK_TIMING_FFT)
        return fail(QPSK_ERR_ARG, "unknown timing_mode %d", p->timing_mode);
    if (p->fixed_index < 0 || p->fixed_index > MAX_INDEX)
        return fail(QPSK_ERR_ARG, "fixed_index %d outside 0..%d", p->fixed_index, MAX_INDEX);

    HIP_TRY(hipSetDevice(device));
    KERNEL_TRY(prepare_kernels());
    KERNEL_TRY(prepare_pipe_kernel());
    KERNEL_TRY(prepare_timing_scan());
    KERNEL_TRY(prepare_stream_block());
    KERNEL_TRY(prepare_stream_scan());
    KERNEL_TRY(prepare_carrier_est());
    qpsk_ctx *c = new qpsk_ctx();
    c->device = device;
    for (const auto &k : TUNING_KEYS) {   /* the only place the environment is read */
        const char *v = getenv(k.name);
        if (!v || !*v) continue;
        if (k.field == &Tuning::viterbi_chunk_rows) {      /* a number or nothing: text that is no integer leaves the key unset, 0 is refused below */
            char *end = nullptr;
            const long n = strtol(v, &end, 10);
            if (end == v || *end) continue;
            c->tune.*(k.field) = n < 0 ? -1 : n > INT_MAX ? INT_MAX : (int)n;
            continue;
        }
        c->tune.*(k.field) = atoi(v);
    }
    if (c->tune.viterbi_chunk_rows == 0) {      /* as qpsk_ctx_set_tuning: no chunk of no rows */
        delete c;
        return fail(QPSK_ERR_ARG, "qpsk_ctx_create: QPSK_VITERBI_CHUNK_ROWS = 0 in the environment (>= 1, or negative for the library's own choice)");
    }
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
            c->ncu = ncu;
    }
    c->prm = *p;
    c->cycles = cycles;
    c->nsym = p->frame_size / cycles;
    c->stream = (hipStream_t)stream; /* NULL = the HIP default stream, like every HIP library */
    qpsk_host_rrc_taps((float)p->fs, (float)p->rs, p->rrc_alpha, c->taps); /* rrc_make(FS, RS, alpha), qpsk.c:308 */
    c->damping = sqrtf(2.0f) / 2.0f;                                        /* costas_loop.c:38 */
    qpsk_host_loop_gains(c->damping, p->loop_bw, &c->alpha, &c->beta);
    c->min_freq = p->min_freq;
    c->max_freq = p->max_freq;
    if (hipMalloc((void **)&c->d_taps, 128 * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&c->d_gains, MAX_BW * 2 * sizeof(float)) != hipSuccess ||
        hipHostMalloc((void **)&c->h_status, sizeof(int), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->d_status, c->h_status, 0) != hipSuccess) {
        qpsk_ctx_destroy(c);
        return fail(QPSK_ERR_ALLOC, "hipMalloc of configuration buffers failed");
    }
    *c->h_status = 0;
    if (hipHostMalloc((void **)&c->h_done, sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->d_done, c->h_done, 0) != hipSuccess) {
        qpsk_ctx_destroy(c);
        return fail(QPSK_ERR_ALLOC, "pinned counter");
    }
    *c->h_done = 0;
    int rc = upload_config(c);
    if (rc != QPSK_OK) { qpsk_ctx_destroy(c); return rc; }
    *out = c;
    return QPSK_OK;
}

static void free_streams(qpsk_ctx *c)
{
    if (c->h_stage) hipHostFree(c->h_stage);
    hipFree(c->d_stage);
    c->h_stage = c->d_stage = nullptr;
    c->stage_cap = 0;
    hipFree(c->s_memory); hipFree(c->s_dec); hipFree(c->s_loop); hipFree(c->s_mixer); hipFree(c->s_ctab); hipFree(c->s_cstate);
    c->s_memory = c->s_dec = c->s_loop = c->s_mixer = c->s_ctab = c->s_cstate = nullptr;
    c->carrier_shared = false;
    c->carrier_pending = nullptr;       /* points into s_ctab */
    c->nstreams = 0;
}

static void free_deframer(qpsk_ctx *c)
{
    hipFree(c->df_state); hipFree(c->df_tables);
    c->df_state = c->df_tables = nullptr;
    c->df_ready = false;
    c->df_coded = false;
    c->df_layout = CodedLayout{};
    c->df_nstreams = 0;
}

static void free_transmitters(qpsk_ctx *c)
{
    hipFree(c->t_hist); hipFree(c->t_mixer); hipFree(c->tx_b.p);
    c->t_hist = nullptr;
    c->t_mixer = nullptr;
    c->tx_b = DevBuf();
    c->ntx = 0;
}

void qpsk_ctx_destroy(qpsk_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipFree(c->d_taps);
    hipFree(c->d_gains);
    if (c->h_status) hipHostFree(c->h_status);
    if (c->h_done) hipHostFree(c->h_done);
    hipFree(c->index.p);
    hipFree(c->filtered.p);
    hipFree(c->mixed.p);
    hipFree(c->keystream.p);
    hipFree(c->sympad.p);
    hipFree(c->mislist.p);
    hipFree(c->softgain.p);
    hipFree(c->vitdec.p);
    hipFree(c->dfstage.p);
    hipFree(c->frame_ks);
    if (c->d_hint) hipFree(c->d_hint);
    if (c->h_hist_stats) hipHostFree(c->h_hist_stats);
    for (auto &kv : c->twiddles) hipFree(kv.second);
    hipFree(c->d_fast);
    free_streams(c);
    free_transmitters(c);
    free_deframer(c);
    delete c;
}

int qpsk_ctx_sync(qpsk_ctx *c)
{
    if (!c) return fail(QPSK_ERR_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return check_status(c);
}

/* four 2-bit symbols per byte (bitstages.hip): what a host that gathers every step copies back instead of a byte per symbol */
int qpsk_pack_symbols(qpsk_ctx *c, const uint8_t *d_sym, long long nrows, int nsym, uint8_t *d_packed)
{
    if (!c || !d_sym || !d_packed || nrows < 0 || nsym <= 0) return fail(QPSK_ERR_ARG, "qpsk_pack_symbols: bad argument");
    if (bind(c)) return QPSK_ERR_HIP;
    if ((nsym & 15) == 0 && (((uintptr_t)d_sym & 15) || ((uintptr_t)d_packed & 3)))
        return fail(QPSK_ERR_ARG, "qpsk_pack_symbols: d_sym must be 16-byte and d_packed 4-byte aligned");
    KERNEL_TRY(launch_pack_dibits(d_sym, d_packed, (size_t)nrows, nsym, c->stream));
    return QPSK_OK;
}

/* the host side of it: plain C, a format conversion for callers that want a byte per symbol again */
int qpsk_unpack_symbols_host(const uint8_t *h_packed, long long nrows, int nsym, uint8_t *h_sym)
{
    if (!h_packed || !h_sym || nrows < 0 || nsym <= 0) return fail(QPSK_ERR_ARG, "qpsk_unpack_symbols_host: bad argument");
    const size_t pb = (size_t)(nsym + 3) / 4;
    for (long long r = 0; r < nrows; r++) {
        const uint8_t *p = h_packed + (size_t)r * pb;
        uint8_t *o = h_sym + (size_t)r * (size_t)nsym;
        for (int i = 0; i < nsym; i++) o[i] = (uint8_t)((p[i >> 2] >> (2 * (i & 3))) & 3u);
    }
    return QPSK_OK;
}

/* the status word WITHOUT a synchronisation: what the kernels completed so far have flagged (multi.cpp looks at it behind a result
 * slot's copy event, while the next step may already be running on the compute stream) */
int qpsk_ctx_check(qpsk_ctx *c)
{
    if (!c) return fail(QPSK_ERR_ARG, "null context");
    return check_status(c);
}

/* multi.cpp's shard threads report through the CALLING thread's error text */
int qpsk_set_error(int code, const char *msg)
{
    return fail(code, "%s", msg ? msg : "");
}

int qpsk_ctx_set_stream(qpsk_ctx *c, void *stream)
{
    if (!c) return fail(QPSK_ERR_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)stream;
    return QPSK_OK;
}

int qpsk_ctx_set_tuning(qpsk_ctx *c, const char *name, int value)
{
    if (!c || !name) return fail(QPSK_ERR_ARG, "null argument");
    for (const auto &k : TUNING_KEYS)
        if (!strcmp(k.name, name)) {
            if (value == 0 && k.field == &Tuning::viterbi_chunk_rows)
                return fail(QPSK_ERR_ARG, "qpsk_ctx_set_tuning: QPSK_VITERBI_CHUNK_ROWS = 0 (>= 1, or negative for the library's own choice)");
            c->tune.*(k.field) = value < 0 ? -1 : value;
            return QPSK_OK;
        }
    return fail(QPSK_ERR_ARG, "qpsk_ctx_set_tuning: unknown name '%s'", name);
}

int qpsk_ctx_cycles(const qpsk_ctx *c) { return c ? c->cycles : 0; }
int qpsk_ctx_nsym(const qpsk_ctx *c) { return c ? c->nsym : 0; }
const char *qpsk_ctx_last_kernel(const qpsk_ctx *c) { return c ? c->last_kernel : ""; }

int qpsk_ctx_get_taps(const qpsk_ctx *c, float *h)
{
    if (!c || !h) return fail(QPSK_ERR_ARG, "null argument");
    memcpy(h, c->taps, sizeof c->taps);
    return QPSK_OK;
}

int qpsk_ctx_get_gains(const qpsk_ctx *c, float *a, float *b)
{
    if (!c || !a || !b) return fail(QPSK_ERR_ARG, "null argument");
    *a = c->alpha;
    *b = c->beta;
    return QPSK_OK;
}

int qpsk_ctx_set_taps(qpsk_ctx *c, const float *h)
{
    if (!c || !h) return fail(QPSK_ERR_ARG, "null argument");
    if (bind(c)) return QPSK_ERR_HIP;
    memcpy(c->taps, h, sizeof c->taps);
    c->fast_valid = false;
    return upload_config(c);
}

int qpsk_ctx_set_loop(qpsk_ctx *c, float alpha, float beta, float min_freq, float max_freq)
{
    if (!c) return fail(QPSK_ERR_ARG, "null argument");
    if (bind(c)) return QPSK_ERR_HIP;
    /* the limits are kernel arguments; the gains live in device memory and go up only when they change (the
     * drop-in rx_frame() calls this before every block) */
    c->min_freq = min_freq; c->max_freq = max_freq;
    if (alpha == c->alpha && beta == c->beta && !(alpha == 0.0f && beta == 0.0f)) return QPSK_OK;
    c->alpha = alpha; c->beta = beta;
    return upload_config(c);
}

/* ---------------------------------------------------------------- tiling */
static int tuned(int v, int dflt) { return v >= 0 ? v : dflt; }

/* full-rate rrc_fir() of a batch of delay lines (rrc_fir.c:17-30): the generated stream with the taps in SGPRs when the
 * filter is symmetric (firstream.hip), the compiler-scheduled kernel for any other tap set (kernels.hip) */
static int fir_full_rate(qpsk_ctx *c, const float *x, const float *memory, float *y, int nframes, int length, size_t in_pitch = 0)
{
    if (c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0)
        return launch_rrc_fir_stream(x, memory, y, c->d_taps, nframes, length, c->stream, in_pitch, c->ncu);
    return launch_rrc_fir(x, memory, y, c->d_taps, nframes, length, c->stream, in_pitch);
}

/* frames per workgroup G and symbols per chunk S of rx_fused_kernel */
static void pick_tiling(const qpsk_ctx *c, int nframes, int nbw, int *G, int *S)
{
    int g = nframes / 256;                 /* one workgroup per CU when the batch allows it */
    if (g < 1) g = 1;
    if (g > 64 / nbw) g = 64 / nbw;
    if (g < 1) g = 1;
    g = tuned(c->tune.fused_g, g);
    if (g < 1) g = 1;
    if (g * nbw > 64) g = 64 / nbw;
    int s = tuned(c->tune.fused_s, 64);
    s &= ~7;
    if (s < 8) s = 8;
    const size_t budget = (size_t)tuned(c->tune.fused_lds, 64 * 1024);
    while (s > 8 && fused_lds_bytes(g, s, c->cycles, nbw) > budget) s -= 8;
    while (g > 1 && fused_lds_bytes(g, s, c->cycles, nbw) > (size_t)MAX_LDS_BYTES) g--;
    *G = g;
    *S = s;
}

/* device copy of the size-n twiddle table (cos, sin)(TAU j/n), built once per n with the host's libm (fft.c:55-56) */
static int get_twiddles(qpsk_ctx *c, int n, double **out)
{
    auto it = c->twiddles.find(n);
    if (it != c->twiddles.end()) { *out = it->second; return QPSK_OK; }
    const size_t cnt = n >= 2 ? (size_t)n / 2 : 1;
    std::vector<double> h(2 * cnt, 0.0);
    qpsk_host_twiddles(n, h.data());
    double *tw = nullptr;
    HIP_TRY(hipMalloc((void **)&tw, sizeof(double) * 2 * cnt));
    HIP_TRY(hipMemcpy(tw, h.data(), sizeof(double) * 2 * cnt, hipMemcpyHostToDevice));
    c->twiddles[n] = tw;
    *out = tw;
    return QPSK_OK;
}

/* the FFT timing estimate's host-built tables: size-512 twiddles and the CYCLES candidate phases (libm, like fft.c:55-56) */
static int fft_timing_tables(qpsk_ctx *c, double **tw_out, double **cs_out)
{
    const int C = c->cycles, nfft = timing_fft_nfft();
    if (C < 2 || C > 8 || (C & (C - 1)))
        return fail(QPSK_ERR_ARG, "QPSK_TIMING_FFT needs CYCLES in {2,4,8} (the symbol-rate bin NFFT/CYCLES must be exact and the offset < 8); CYCLES = %d", C);
    if (c->prm.frame_size < timing_fft_first() + nfft)
        return fail(QPSK_ERR_ARG, "QPSK_TIMING_FFT needs frame_size >= %d", timing_fft_first() + nfft);
    double *tw = nullptr;
    int rc = get_twiddles(c, nfft, &tw);
    if (rc) return rc;
    /* candidate phases (cos, sin)(TAU i/CYCLES): entry -C of the twiddle cache (key < 0 cannot collide with an FFT size) */
    double *cs = nullptr;
    auto it = c->twiddles.find(-C);
    if (it == c->twiddles.end()) {
        std::vector<double> full(2 * (size_t)C);
        qpsk_host_phases(C, full.data());
        HIP_TRY(hipMalloc((void **)&cs, sizeof(double) * 2 * C));
        HIP_TRY(hipMemcpy(cs, full.data(), sizeof(double) * 2 * C, hipMemcpyHostToDevice));
        c->twiddles[-C] = cs;
    } else {
        cs = it->second;
    }
    *tw_out = tw;
    *cs_out = cs;
    return QPSK_OK;
}

static int fft_timing_indices(qpsk_ctx *c, const float *d_in, int nframes, int32_t *d_index, float *d_y = nullptr,
                              double *d_X = nullptr, size_t pitch = 0, double *d_bin = nullptr)
{
    double *tw = nullptr, *cs = nullptr;
    int rc = fft_timing_tables(c, &tw, &cs);
    if (rc) return rc;
    KERNEL_TRY(launch_timing_fft(d_in, nframes, c->prm.frame_size, c->cycles, c->d_taps, tw, cs, d_index, d_y, d_X, d_bin, c->stream, pitch,
                                 c->ncu, c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0));
    return QPSK_OK;
}

/* QPSK_HIST_GENERIC = 1 or 2 keeps the three-kernel path (rrc_fir -> scan -> pipeline), 2 with the any-CYCLES scan too */
static bool scan_fused_ok(const qpsk_ctx *c, const float *d_in)
{
    return c->cycles == 8 && c->prm.frame_size % timing_scan_tile() == 0 && ((uintptr_t)d_in % 16) == 0 &&
           tuned(c->tune.hist_generic, 0) == 0;
}

/* fused_fft: the caller will run the FFT estimate inside the receive launch (rx_fused_pipe_kernel, full workgroups): no
 * launch here, *d_index_out stays NULL; c->index is sized for the indices the kernel leaves */
static int timing_indices(qpsk_ctx *c, const float *d_in, size_t pitch, int nframes, const int32_t **d_index_out, bool fused_fft = false)
{
    *d_index_out = nullptr;
    if (c->prm.timing_mode == QPSK_TIMING_FIXED) return QPSK_OK;
    int rc = ensure(c, c->index, sizeof(int32_t) * (size_t)nframes);
    if (rc) return rc;
    if (fused_fft && c->prm.timing_mode == QPSK_TIMING_FFT) return QPSK_OK;
    if (c->prm.timing_mode == QPSK_TIMING_HIST) {
        /* the fused full-rate FIR + scan kernel keeps the filtered block in LDS (timing_scan.hip): the input is read
         * once here and once by the pipeline kernel that follows, nothing is written but the index */
        if (scan_fused_ok(c, d_in) && (pitch & 1) == 0) {
            KERNEL_TRY(launch_timing_scan(d_in, nframes, c->prm.frame_size, c->d_taps, (int32_t *)c->index.p, nullptr,
                                          c->d_status, c->stream, pitch, c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0));
            *d_index_out = (const int32_t *)c->index.p;
            return QPSK_OK;
        }
        const size_t bytes = sizeof(float) * 2 * (size_t)nframes * c->prm.frame_size;
        rc = ensure(c, c->filtered, bytes);
        if (rc) return rc;
        KERNEL_TRY(fir_full_rate(c, d_in, nullptr, (float *)c->filtered.p, nframes, c->prm.frame_size, pitch));
        KERNEL_TRY(launch_timing_hist((const float *)c->filtered.p, nframes, c->prm.frame_size, c->cycles,
                                      (int32_t *)c->index.p, nullptr, tuned(c->tune.hist_generic, 0) == 2, c->stream));
        *d_index_out = (const int32_t *)c->index.p;
        return QPSK_OK;
    }
    /* QPSK_TIMING_FFT: symbol-rate line of |y|^2 through the reference's radix-2 FFT (timing_fft.hip) */
    rc = fft_timing_indices(c, d_in, nframes, (int32_t *)c->index.p, nullptr, nullptr, pitch);
    if (rc) return rc;
    *d_index_out = (const int32_t *)c->index.p;
    return QPSK_OK;
}

/* acquisition supplied from outside (qpsk_rx_batch_ext): per-frame decimation offsets in place of the context's timing estimate,
 * per-loop (phase, freq) seeds in place of (0, 0); either may be NULL */
struct ExtAcq {
    const int32_t *index;
    const float *seed;
};

/* ---- which kernel takes a receive batch: decided ONCE, as a route.  rx_route() only reads -- the context and the filled arguments are
 * const, so it cannot allocate, launch or touch last_kernel -- and everything behind it reads the route: the buffers, the timing
 * estimate's placement, the launch.  Nothing restates the choice (round 4 restated it for the in-launch FFT estimate and missed a tuning
 * key: QPSK_PIPE_G above 16 sent the batch to rx_lean_kernel with no index computed).
 * The pipeline kernels [measured, DESIGN.md 4.1]: rx_lean_kernel wherever its stream serves the shape; rx_fused_pipe_kernel (16-frame
 * workgroups, four-symbol FIR lanes) for batches below four frames per workgroup, several loops per frame, a costas_frame[] dump and
 * config 3; rx_pipe2_kernel for those above 16 frames per CU; the generic chunked kernel (kernels.hip) for any other shape. */
enum RxKind { K_GENERIC, K_FUSED_PIPE, K_PIPE2, K_LEAN };

struct RxRoute {
    RxKind kind = K_GENERIC;
    int G = 0;                        /* K_PIPE2, K_LEAN: frames per workgroup */
    int nf = 0;                       /* K_FUSED_PIPE: FIR waves per workgroup */
    unsigned long long layout = 0;    /* K_PIPE2, K_LEAN: units per hardware wave */
    bool pipe_ok = false;             /* the shape the pipeline kernels (rx_pipe.h) are built for */
    bool fused_fft = false;           /* the FFT timing estimate runs inside the receive launch, not in a launch in front */
    bool need_pad = false;            /* the caller provides -- K_LEAN on a batch that is not whole workgroups: FusedArgs::sym_pad, G rows */
    bool data_rule = false;           /* qpsk_rx_batch_data: the kernel writes the data rule's decisions itself (FusedArgs::data_rule) */
    bool need_dump = false;           /* qpsk_rx_batch_data on any other route: a costas_frame[] dump of the library's own to take them from */
};

/* the caller's wave layout (measurements): 4 bits per hardware wave = units it owns, waves 1-5 in QPSK_PIPE_LAYOUT_LO, 6-11 in
 * QPSK_PIPE_LAYOUT_HI; false = neither is set, the library's own layout */
static bool tuned_layout(const qpsk_ctx *c, unsigned long long *layout)
{
    if (c->tune.layout_lo < 0 && c->tune.layout_hi < 0) return false;
    *layout = ((unsigned long long)(unsigned)tuned(c->tune.layout_lo, 0) << 4) | ((unsigned long long)(unsigned)tuned(c->tune.layout_hi, 0) << 24);
    return true;
}

/* a: as rx_batch_common fills it (a.index = the caller's own offsets, a.data_rule = data decisions wanted WITHOUT the slicer's); want_data: a qpsk_rx_batch_data call */
static int rx_route(const qpsk_ctx *c, const FusedArgs &a, bool want_data, RxRoute *rt)
{
    const int nframes = a.nframes, nbw = a.nbw;
    *rt = RxRoute{};
    /* the pipeline kernels are built for CYCLES = 8, 16-byte aligned frames and an index below CYCLES */
    const bool pipe_ok = rt->pipe_ok = c->cycles == pipe_cycles() && (a.frame_size % 2) == 0 && (a.frame_pitch % 2) == 0 &&
                                       ((uintptr_t)a.x % 16) == 0 && nbw * pipe_frames(1) <= 64 && tuned(c->tune.generic, 0) == 0;
    /* QPSK_PIPE_V = 3 asks for rx_lean_kernel at any batch size, 1 / 2 for the older kernels */
    const int by_size = nframes > 16 * c->ncu ? 2 : 1;
    int pipe_v = tuned(c->tune.pipe_v, by_size);
    unsigned long long own_layout = 0;
    const bool has_layout = tuned_layout(c, &own_layout);

    /* rx_lean_kernel (the FIR waves' chunk loop as one hand-written stream) serves even workgroups of frames made of whole chunks, one
     * loop per frame, symmetric filter, no costas_frame[] dump -- so not a caller who wants data decisions AND the slicer's.  Above 16
     * frames per CU always (the filter is the limit there); below, both kernels sit on the serial wave and this one is 1-3 % ahead
     * from four frames per workgroup on (profiles/r05_config2_lean.txt).  A batch that is not whole workgroups rides in the same launch:
     * the last workgroup's pad frames read the batch's last frame and leave their symbols in the pad rows (round 5's second launch for
     * them cost one more serial chain, 0.25 + 0.15 ms for 8193 frames against 0.25 for 8192). */
    if (pipe_ok && c->taps_symmetric && (pipe_v == 3 || c->tune.pipe_v < 0) && !(want_data && !a.data_rule)) {
        int G = tuned(c->tune.pipe_g, (nframes + c->ncu - 1) / c->ncu);
        if (G > pipe2_max_frames()) G = pipe2_max_frames();
        G += G & 1;
        const bool wanted = pipe_v == 3 || G >= 4;
        const unsigned long long layout = has_layout ? own_layout : G >= 2 ? lean_default_layout(G / 2) : 0;
        if (wanted && layout && lean_shape_ok(a, G)) {
            const LayoutCount n = layout_count(layout);
            if (n.units == G / 2 && lean_lds_bytes(G, n.nwin) <= (size_t)MAX_LDS_BYTES) {
                rt->kind = K_LEAN;
                rt->G = G;
                rt->layout = layout;
                rt->need_pad = nframes % G != 0;
                rt->data_rule = a.data_rule != 0;
            }
        }
    }
    /* every other shape: the pipeline kernels of rounds 1-2, or the generic chunked kernel */
    const bool older = rt->kind != K_LEAN && pipe_ok;
    if (pipe_v == 3) pipe_v = by_size;
    if (older && pipe_v == 2) {
        /* rx_pipe2_kernel: up to 32 frames per workgroup, one workgroup per CU when the batch allows it */
        int G = tuned(c->tune.pipe_g, (nframes + c->ncu - 1) / c->ncu);
        if (G > pipe2_max_frames()) G = pipe2_max_frames();
        if (G * nbw > 64) G = 64 / nbw;
        if (G < 1) G = 1;
        unsigned long long layout = own_layout;
        if (has_layout) {      /* its units fix G */
            const LayoutCount n = layout_count(layout);
            if (n.units < 1 || (G + 1) / 2 != n.units || pipe2_lds_bytes(G, n.nwin, nbw) > (size_t)MAX_LDS_BYTES)
                return fail(QPSK_ERR_ARG, "QPSK_PIPE_LAYOUT_*: %d units on %d waves do not match %d frames per workgroup", n.units, n.nwin, G);
        } else {
            for (;;) {   /* many loops per frame: the record rings grow, fewer frames fit */
                layout = pipe2_default_layout((G + 1) / 2);
                if (layout && pipe2_lds_bytes(G, layout_count(layout).nwin, nbw) <= (size_t)MAX_LDS_BYTES) break;
                if (G == 1) return fail(QPSK_ERR_ARG, "pipeline geometry does not fit: %d loops per frame", nbw);
                G--;
            }
        }
        rt->kind = K_PIPE2;
        rt->G = G;
        rt->layout = layout;
    } else if (older) {
        /* rx_fused_pipe_kernel: 16-frame workgroups (four FIR waves of four frames, fewer when the batch gives a CU fewer frames); a
         * batch above 16 frames per CU would run them in rounds.  One lane of the serial wave per (frame, loop); rings grow with the loops */
        const int full = pipe_max_nf();
        int nf = 1;
        while (nf < full && (long long)c->ncu * pipe_frames(nf) < nframes) nf++;
        nf = tuned(c->tune.pipe_nf, nf);
        if (nf < 1) nf = 1;
        if (nf > full) nf = full;
        while (pipe_frames(nf) * nbw > 64 || pipe_lds_bytes(nf, nbw) > (size_t)MAX_LDS_BYTES) {
            if (nf == 1) return fail(QPSK_ERR_ARG, "pipeline geometry does not fit: nf %d, %d loops per frame", nf, nbw);
            nf--;
        }
        rt->kind = K_FUSED_PIPE;
        rt->nf = nf;
    }
    rt->need_dump = want_data && !rt->data_rule && !a.costas;
    /* BASELINE config 3's shape -- FFT estimate, rx_fused_pipe_kernel in full 16-frame workgroups -- and rx_lean_kernel where the
     * estimate fits beside its geometry run the estimate inside the receive launch; every other route gets its indices from a launch in
     * front (timing_fft_kernel / timing_scan_kernel / ...) */
    rt->fused_fft = c->prm.timing_mode == QPSK_TIMING_FFT && !a.index && nbw == 1 && tuned(c->tune.fft_fused, 1) != 0 &&
                    a.frame_size >= timing_fft_first() + timing_fft_nfft() &&
                    ((rt->kind == K_FUSED_PIPE && rt->nf == pipe_max_nf() && !(a.dbg & (128 | 4))) ||
                     (rt->kind == K_LEAN && lean_est_ok(a, rt->G, rt->layout)));
    return QPSK_OK;
}

/* ---- histogram timing in ONE pass (round 6; rx_hist.hip, rx_hist_kernel): where the context has a guess -- the majority index of its
 * previous histogram-mode batch -- the scan kernel's workgroup runs the receive path on that guess while it scans, the frames whose true
 * index differs are redone by a fall-back pass over their list (usually empty), and the batch's own majority becomes the next guess.
 * *taken = false and nothing launched: no guess yet, a shape the kernel does not serve, or a last batch that missed frames (the caller
 * goes on with the two-launch route).  Not for an ext call: with its own offsets it needs no estimate, without them it takes the
 * two-launch route and neither reads nor updates the guess. */
static int rx_hist_onepass(qpsk_ctx *c, const FusedArgs &a, const RxRoute &rt, int32_t *d_index, bool *taken)
{
    *taken = false;
    /* (QPSK_PIPE_V asks for one of the receive kernels by name) */
    if (!rt.pipe_ok || !c->taps_symmetric || !scan_fused_ok(c, (const float *)a.x) || c->tune.pipe_v >= 0) return QPSK_OK;
    if (!c->d_hint) {
        /* all three or none: a failure half way leaves the context without the route's books, and the next call starts over */
        int32_t *hint = nullptr, *h_stats = nullptr, *d_stats = nullptr;
        hipError_t e = hipMalloc((void **)&hint, 2 * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemset(hint, 0, 2 * sizeof(int32_t));
        if (e == hipSuccess) e = hipHostMalloc((void **)&h_stats, 4 * sizeof(int32_t), hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&d_stats, h_stats, 0);
        if (e != hipSuccess) {
            if (h_stats) hipHostFree(h_stats);
            if (hint) hipFree(hint);
            return fail(QPSK_ERR_ALLOC, "one-pass histogram route: %s", hipGetErrorString(e));
        }
        h_stats[0] = h_stats[1] = h_stats[2] = -1;
        c->d_hint = hint;
        c->h_hist_stats = h_stats;
        c->d_hist_stats = d_stats;
        c->hint_valid = false;
    }
    const int op = tuned(c->tune.hist_onepass, -1);
    /* the route pays only while the guess holds for EVERY frame: a frame it misses goes through the fall-back pass, whose one
     * workgroup takes 0.4 ms whatever the count (a serial chain again) against the 0.07 ms the route saves.  Every histogram-mode call
     * leaves behind how many frames of its batch were off the batch's majority index (or missed by its guess): zero = try the route */
    const int seen = __atomic_load_n(&c->h_hist_stats[1], __ATOMIC_ACQUIRE), off_majority = __atomic_load_n(&c->h_hist_stats[2], __ATOMIC_ACQUIRE);
    const bool guess_is_good = seen > 0 && off_majority == 0;
    if (op == 0 || !c->hint_valid || !(op == 1 || guess_is_good) || !rx_hist_shape_ok(a)) return QPSK_OK;
    if (int rc = ensure(c, c->index, sizeof(int32_t) * (size_t)a.nframes)) return rc;
    if (int rc = ensure(c, c->mislist, sizeof(int32_t) * (size_t)a.nframes)) return rc;
    /* the miss counter starts from zero whatever the last call left: index_majority_kernel resets it, but a call that failed between its
     * launches never got that far, and rx_hist_kernel appends from the count it finds */
    int32_t *mis_count = c->d_hint + 1;
    HIP_TRY(hipMemsetAsync(mis_count, 0, sizeof(int32_t), c->stream));
    KERNEL_TRY(launch_rx_hist(a, (int32_t *)c->index.p, c->d_hint, (int32_t *)c->mislist.p, mis_count, c->d_status, c->stream));
    /* the fall-back pass: the generic chunked kernel over the listed frames with their true indices (its grid is sized for the
     * whole batch: the list's length is known on the device only; workgroups beyond it retire at once) */
    FusedArgs af = a;
    af.index = (const int32_t *)c->index.p;
    af.frame_list = (const int32_t *)c->mislist.p;
    af.frame_list_count = mis_count;
    af.G = 4;
    af.S = 64;
    KERNEL_TRY(launch_rx_fused(af, c->stream));
    KERNEL_TRY(launch_index_majority((const int32_t *)c->index.p, a.nframes, c->d_hint, mis_count, c->d_hist_stats, c->stream));
    c->last_kernel = "rx_hist_kernel (one pass on the guessed index) + rx_fused_kernel (fall-back list)";
    if (d_index)
        HIP_TRY(hipMemcpyAsync(d_index, c->index.p, sizeof(int32_t) * (size_t)a.nframes, hipMemcpyDeviceToDevice, c->stream));
    *taken = true;
    return QPSK_OK;
}

/* the receive launch the route names */
static int rx_launch(qpsk_ctx *c, const FusedArgs &a, const RxRoute &rt)
{
    /* only rx_fused_pipe_kernel's full workgroups and rx_lean_kernel look at est_tw; any other kernel would demodulate with fixed_index */
    if (a.est_tw && !(rt.kind == K_FUSED_PIPE && rt.nf == pipe_max_nf()) && rt.kind != K_LEAN)
        return fail(QPSK_ERR_STATE, "internal: in-launch FFT timing estimate planned for a kernel that has none");
    if (a.data_rule && rt.kind != K_LEAN)
        return fail(QPSK_ERR_STATE, "internal: data rule planned for a kernel that has none");
    switch (rt.kind) {
    case K_LEAN:
        KERNEL_TRY(launch_rx_lean(a, rt.G, rt.layout, c->d_status, c->stream));
        c->last_kernel = a.est_tw ? "rx_lean_kernel (FFT timing estimate inside the launch)" : "rx_lean_kernel";
        break;
    case K_PIPE2:
        KERNEL_TRY(launch_rx_pipe2(a, rt.G, rt.layout, c->d_status, c->stream));
        c->last_kernel = "rx_pipe2_kernel";
        break;
    case K_FUSED_PIPE:
        KERNEL_TRY(launch_rx_fused_pipe(a, rt.nf, c->d_status, c->stream));
        c->last_kernel = a.est_tw ? "rx_fused_pipe_kernel (FFT timing estimate inside the launch)" : "rx_fused_pipe_kernel";
        break;
    default:
        KERNEL_TRY(launch_rx_fused(a, c->stream));
        c->last_kernel = "rx_fused_kernel";
    }
    return QPSK_OK;
}

/* every qpsk_rx_batch* entry point: check, fill the arguments, route, buffers, one-pass attempt, timing estimate, launch, epilogue */
static int rx_batch_common(qpsk_ctx *c, const float *d_in, long long frame_pitch, int nframes, int nbw, uint8_t *d_sym,
                           float *d_freq, float *d_phase, float *d_costas, int32_t *d_index, float *d_hz,
                           const ExtAcq *ext = nullptr, uint8_t *d_data = nullptr)
{
    if (!c || !d_in || !(d_sym || d_data)) return fail(QPSK_ERR_ARG, "qpsk_rx_batch: null context, input or symbol buffer");
    if (nframes <= 0) return fail(QPSK_ERR_ARG, "qpsk_rx_batch: nframes = %d", nframes);
    if (frame_pitch == 0) frame_pitch = c->prm.frame_size;
    if (frame_pitch < c->prm.frame_size)
        return fail(QPSK_ERR_ARG, "qpsk_rx_batch_pitched: frame_pitch %lld below frame_size %d", frame_pitch, c->prm.frame_size);
    if (bind(c)) return QPSK_ERR_HIP;
    FusedArgs a{};
    a.x = reinterpret_cast<const float2 *>(d_in);
    a.frame_pitch = (size_t)frame_pitch;
    a.nframes = nframes;
    a.frame_size = c->prm.frame_size;
    a.cycles = c->cycles;
    a.nsym = c->nsym;
    pick_tiling(c, nframes, nbw, &a.G, &a.S);
    a.fixed_index = c->prm.fixed_index;
    a.dbg = tuned(c->tune.pipe_variant, 0) & PIPE_VARIANT_MASK;
    a.lean_dma = tuned(c->tune.lean_dma, 1) != 0;
    a.lean_twowin = tuned(c->tune.lean_dma, 1) != 2 ? 1 : 0;      /* QPSK_LEAN_DMA = 2: LDS-DMA, but one window per FIR wave whatever the LDS allows */
    a.est_waves = tuned(c->tune.est_waves, 0);
    a.lean_pair = tuned(c->tune.lean_pair, 3);      /* 3: the library's own rule (launch_rx_lean) */
    a.taps = c->d_taps;
    a.gains = c->d_gains;
    a.nbw = nbw;
    a.min_freq = c->min_freq;
    a.max_freq = c->max_freq;
    a.rs = c->prm.rs;
    /* qpsk_rx_batch_data: with d_sym NULL, rx_lean_kernel writes the data rule's decisions where the slicer's go (FusedArgs::data_rule);
     * every other route dumps costas_frame[] and takes the data rule from it behind the launch (the epilogue) */
    a.sym = d_sym ? d_sym : d_data;
    a.data_rule = d_data && !d_sym;
    a.freq = d_freq;
    a.phase = d_phase;
    a.costas = reinterpret_cast<float2 *>(d_costas);
    a.hz = d_hz;
    a.status = c->d_status;
    /* an ext call's offsets: every timing estimate skipped, the kernels check each value where they read it (STATUS_BAD_INDEX); its
     * seeds: the serial waves apply set_phase() / set_frequency() at the load (kernels.h, seed_setters) */
    if (ext) a.index = ext->index;
    if (ext && ext->seed) {
        a.state_in = ext->seed;
        a.seed_setters = 1;
    }

    RxRoute rt;
    if (int rc = rx_route(c, a, d_data != nullptr, &rt)) return rc;

    /* ---- what the route asks the caller for */
    a.data_rule = rt.data_rule;
    if (rt.need_pad) {
        if (int rc = ensure(c, c->sympad, (size_t)rt.G * (size_t)c->nsym)) return rc;
        a.sym_pad = (uint8_t *)c->sympad.p;
    }
    if (rt.need_dump) {
        if (int rc = ensure(c, c->datacostas, sizeof(float2) * (size_t)nframes * (size_t)c->nsym)) return rc;
        a.costas = (float2 *)c->datacostas.p;
    }

    const bool hist_guess = c->prm.timing_mode == QPSK_TIMING_HIST && !ext;      /* the call reads and updates the one-pass route's guess */
    if (hist_guess) {
        bool taken = false;
        const int rc = rx_hist_onepass(c, a, rt, d_index, &taken);
        if (rc || taken) return rc;
    }

    /* ---- the timing estimate: inside the receive launch where the route says so (the kernel leaves the indices in c->index when the
     * caller wants them), else from a launch in front */
    const int32_t *idx = a.index;
    if (!idx) {
        if (int rc = timing_indices(c, d_in, (size_t)frame_pitch, nframes, &idx, rt.fused_fft)) return rc;
        a.index = idx;
    }
    if (rt.fused_fft) {
        double *est_tw = nullptr, *est_cs = nullptr;
        if (int rc = fft_timing_tables(c, &est_tw, &est_cs)) return rc;
        a.est_tw = reinterpret_cast<const double2 *>(est_tw);
        a.est_cs = reinterpret_cast<const double2 *>(est_cs);
        a.index_out = d_index ? (int32_t *)c->index.p : nullptr;
        if (d_index) idx = (const int32_t *)c->index.p;      /* copied to the caller's array behind the launch, below */
    }

    if (int rc = rx_launch(c, a, rt)) return rc;

    /* ---- the epilogue */
    if (hist_guess && c->d_hint && idx && tuned(c->tune.hist_onepass, -1) != 0) {
        /* the batch's majority index as the next histogram-mode call's guess (one workgroup, in stream order) */
        KERNEL_TRY(launch_index_majority(idx, nframes, c->d_hint, c->d_hint + 1, c->d_hist_stats, c->stream));
        c->hint_valid = true;
    }
    if (rt.kind == K_LEAN && (nframes & 1)) {
        /* the last frame of an odd batch shares its two-frame unit with a pad frame: the unit's rows are pad rows (rx_lean.hip,
         * lean_unit_rows); its own row goes to its place behind the launch */
        const size_t last0 = (size_t)((nframes - 1) / rt.G) * (size_t)rt.G;      /* the last workgroup's first frame */
        HIP_TRY(hipMemcpyAsync(a.sym + (size_t)(nframes - 1) * (size_t)c->nsym, a.sym_pad + ((size_t)(nframes - 1) - last0) * (size_t)c->nsym,
                               (size_t)c->nsym, hipMemcpyDeviceToDevice, c->stream));
    }
    if (d_data && !a.data_rule)      /* qpsk_rx_batch_data off rx_lean_kernel: the data rule over the costas_frame[] just written */
        KERNEL_TRY(launch_data_from_costas(a.costas, d_data, (size_t)nframes * (size_t)c->nsym, c->stream));
    if (d_index) {
        if (idx == d_index) {
            /* the caller's own offsets, in place */
        } else if (idx)
            HIP_TRY(hipMemcpyAsync(d_index, idx, sizeof(int32_t) * (size_t)nframes, hipMemcpyDeviceToDevice, c->stream));
        else
            KERNEL_TRY(launch_fill_i32(d_index, nframes, c->prm.fixed_index, c->stream));
    }
    return QPSK_OK;
}

/* what every single-loop entry point does first, ahead of its own argument checks: the context's device, and its own (alpha, beta) back
 * in d_gains[0].  A null context passes: rx_batch_common reports it, behind those checks */
static int rx_prologue(qpsk_ctx *c)
{
    if (!c) return QPSK_OK;
    if (bind(c)) return QPSK_ERR_HIP;
    return use_context_gains(c);
}

int qpsk_rx_batch(qpsk_ctx *c, const float *d_in, int nframes, uint8_t *d_sym, float *d_freq, float *d_phase,
                  float *d_costas, int32_t *d_index, float *d_hz)
{
    if (int rp = rx_prologue(c)) return rp;
    return rx_batch_common(c, d_in, 0, nframes, 1, d_sym, d_freq, d_phase, d_costas, d_index, d_hz);
}

int qpsk_rx_batch_pitched(qpsk_ctx *c, const float *d_in, long long frame_pitch, int nframes, uint8_t *d_sym, float *d_freq,
                          float *d_phase, float *d_costas, int32_t *d_index, float *d_hz)
{
    if (int rp = rx_prologue(c)) return rp;
    if (frame_pitch <= 0) return fail(QPSK_ERR_ARG, "qpsk_rx_batch_pitched: frame_pitch = %lld", frame_pitch);
    return rx_batch_common(c, d_in, frame_pitch, nframes, 1, d_sym, d_freq, d_phase, d_costas, d_index, d_hz);
}

static int rx_batch_bw_impl(qpsk_ctx *c, const float *d_in, int nframes, const float *h_loop_bw, int nbw, uint8_t *d_sym,
                            float *d_freq, float *d_phase, int32_t *d_index, const ExtAcq *ext)
{
    if (!c || !h_loop_bw) return fail(QPSK_ERR_ARG, "qpsk_rx_batch_bw: null argument");
    if (nbw < 1 || nbw > MAX_BW) return fail(QPSK_ERR_ARG, "nbw = %d outside 1..%d", nbw, MAX_BW);
    if (bind(c)) return QPSK_ERR_HIP;
    std::vector<float> g(2 * (size_t)nbw);
    for (int b = 0; b < nbw; b++)
        qpsk_host_loop_gains(c->damping, h_loop_bw[b], &g[2 * b], &g[2 * b + 1]); /* set_loop_bandwidth(), costas_loop.c:79-87 */
    if (g != c->h_gains) {
        HIP_TRY(hipStreamSynchronize(c->stream)); /* the previous upload may still read h_gains */
        c->h_gains = g;
        HIP_TRY(hipMemcpyAsync(c->d_gains, c->h_gains.data(), sizeof(float) * g.size(), hipMemcpyHostToDevice, c->stream));
    }
    return rx_batch_common(c, d_in, 0, nframes, nbw, d_sym, d_freq, d_phase, nullptr, d_index, nullptr, ext);
}

int qpsk_rx_batch_bw(qpsk_ctx *c, const float *d_in, int nframes, const float *h_loop_bw, int nbw, uint8_t *d_sym,
                     float *d_freq, float *d_phase, int32_t *d_index)
{
    return rx_batch_bw_impl(c, d_in, nframes, h_loop_bw, nbw, d_sym, d_freq, d_phase, d_index, nullptr);
}

int qpsk_rx_batch_ext(qpsk_ctx *c, const float *d_in, long long frame_pitch, int nframes, const int32_t *d_index_in, const float *d_seed,
                      uint8_t *d_sym, float *d_freq, float *d_phase, float *d_costas, int32_t *d_index, float *d_hz)
{
    if (int rp = rx_prologue(c)) return rp;
    if (frame_pitch < 0) return fail(QPSK_ERR_ARG, "qpsk_rx_batch_ext: frame_pitch = %lld", frame_pitch);
    const ExtAcq ext = {d_index_in, d_seed};
    return rx_batch_common(c, d_in, frame_pitch, nframes, 1, d_sym, d_freq, d_phase, d_costas, d_index, d_hz, &ext);
}

int qpsk_rx_batch_data(qpsk_ctx *c, const float *d_in, long long frame_pitch, int nframes, const int32_t *d_index_in, const float *d_seed,
                       uint8_t *d_data, uint8_t *d_sym, float *d_freq, float *d_phase, int32_t *d_index, float *d_hz)
{
    if (int rp = rx_prologue(c)) return rp;
    if (frame_pitch < 0) return fail(QPSK_ERR_ARG, "qpsk_rx_batch_data: frame_pitch = %lld", frame_pitch);
    if (!d_data) return fail(QPSK_ERR_ARG, "qpsk_rx_batch_data: d_data is NULL");
    const ExtAcq ext = {d_index_in, d_seed};
    return rx_batch_common(c, d_in, frame_pitch, nframes, 1, d_sym, d_freq, d_phase, nullptr, d_index, d_hz, &ext, d_data);
}

int qpsk_sync_batch(qpsk_ctx *c, const uint8_t *d_data, int nframes, int nsym, const uint8_t *h_sync, int nsync, int lag_min, int lag_max,
                    int nout, uint8_t *d_out, int32_t *d_lag, int32_t *d_rot, int32_t *d_score)
{
    if (!c || !d_data || !h_sync) return fail(QPSK_ERR_ARG, "qpsk_sync_batch: null context, data or sync word");
    if (nframes <= 0 || nsym <= 0) return fail(QPSK_ERR_ARG, "qpsk_sync_batch: nframes = %d, nsym = %d", nframes, nsym);
    if (nsync < 1 || nsync > SYNC_MAX_WORD) return fail(QPSK_ERR_ARG, "qpsk_sync_batch: nsync = %d outside 1..%d", nsync, SYNC_MAX_WORD);
    if (nout < 0 || lag_min < 0 || lag_max < lag_min || (long long)lag_max + nsync + nout > nsym)
        return fail(QPSK_ERR_ARG, "qpsk_sync_batch: lags %d..%d, nsync %d, nout %d do not fit a row of %d", lag_min, lag_max, nsync, nout, nsym);
    if (!d_out && !d_lag && !d_rot && !d_score) return fail(QPSK_ERR_ARG, "qpsk_sync_batch: every output is NULL");
    for (int i = 0; i < nsync; i++)
        if (h_sync[i] > 3) return fail(QPSK_ERR_ARG, "qpsk_sync_batch: sync[%d] = %d is not a dibit", i, (int)h_sync[i]);
    if (d_out && nout > 0) {
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)nframes * (size_t)nout;
        const uintptr_t d0 = (uintptr_t)d_data, d1 = d0 + (size_t)nframes * (size_t)nsym;
        if (o0 < d1 && d0 < o1) return fail(QPSK_ERR_ARG, "qpsk_sync_batch: d_out overlaps d_data");
    }
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_sync_search(d_data, nframes, nsym, h_sync, nsync, lag_min, lag_max, nout, nout > 0 ? d_out : nullptr, d_lag, d_rot,
                                  d_score, c->stream));
    c->last_kernel = "sync_search_kernel";
    return QPSK_OK;
}

int qpsk_rx_batch_bw_ext(qpsk_ctx *c, const float *d_in, int nframes, const float *h_loop_bw, int nbw, const int32_t *d_index_in,
                         const float *d_seed, uint8_t *d_sym, float *d_freq, float *d_phase, int32_t *d_index)
{
    const ExtAcq ext = {d_index_in, d_seed};
    return rx_batch_bw_impl(c, d_in, nframes, h_loop_bw, nbw, d_sym, d_freq, d_phase, d_index, &ext);
}

/* Costas + slicer over decimated symbols already in device memory (qpsk.c:196-212): the pipeline kernel with
 * loader waves in place of the FIR waves; the one-lane-per-frame kernel only when QPSK_FUSED_GENERIC is set. */
/* Costas + slicer over rows of decimated symbols.  Streaming mode: refill != NULL names the block just filtered
 * ([nframes][nsym*CYCLES]) and refill_index its timing indices; each row of d_symbols is then replaced by that
 * block's picks once the loop has taken the old ones (qpsk.c:186-191). */
static int costas_over_symbols(qpsk_ctx *c, float *d_symbols, int nframes, int nsym, int dstride, float *d_state,
                               uint8_t *d_sym, float *d_costas, const float *refill = nullptr,
                               const int32_t *refill_index = nullptr, bool refill_planar = false)
{
    float *carrier_tab = c->carrier_pending;
    c->carrier_pending = nullptr;
    if (tuned(c->tune.generic, 0)) {
        if (carrier_tab) KERNEL_TRY(launch_carrier_table(c->s_cstate, carrier_tab, c->prm.frame_size, true, c->stream));
        KERNEL_TRY(launch_costas(d_symbols, nframes, nsym, dstride, 1, c->d_gains, c->min_freq, c->max_freq, d_state, d_state,
                                 d_sym, d_costas, c->d_status, c->stream));
        if (refill) {
            if (dstride != nsym) return fail(QPSK_ERR_ARG, "internal: refill needs packed rows");
            KERNEL_TRY(launch_decimate(refill, refill_index, d_symbols, nframes, nsym * c->cycles, c->cycles, nsym, c->stream));
        }
        return QPSK_OK;
    }
    FusedArgs a{};
    a.nframes = nframes;
    a.nsym = nsym;
    a.frame_size = nsym * c->cycles;
    a.cycles = c->cycles;
    a.refill = reinterpret_cast<const float2 *>(refill);
    a.refill_dst = reinterpret_cast<float2 *>(d_symbols);
    a.refill_planar = refill_planar ? 1 : 0;
    a.index = refill_index;
    a.gains = c->d_gains;
    a.nbw = 1;
    a.min_freq = c->min_freq;
    a.max_freq = c->max_freq;
    a.rs = c->prm.rs;
    a.state_in = d_state;
    a.state_out = d_state;
    a.sym = d_sym;
    a.costas = reinterpret_cast<float2 *>(d_costas);
    a.dsrc = reinterpret_cast<const float2 *>(d_symbols);
    a.dstride = dstride;
    a.status = c->d_status;
    if (carrier_tab) {
        a.carrier_state = c->s_cstate;
        a.carrier_tab = reinterpret_cast<float2 *>(carrier_tab);
        a.carrier_frame = c->prm.frame_size;
    }
    a.dbg = tuned(c->tune.pipe_variant, 0) & PIPE_VARIANT_MASK;
    int nf = (nframes + c->ncu * pipe_frames(1) - 1) / (c->ncu * pipe_frames(1));
    if (nf < 1) nf = 1;
    if (nf > pipe_max_nf()) nf = pipe_max_nf();
    KERNEL_TRY(launch_costas_pipe(a, nf, c->d_status, c->stream));
    return QPSK_OK;
}

/* ---------------------------------------------------------------- stages */
int qpsk_rrc_fir_batch(qpsk_ctx *c, float *d_memory, const float *d_in, float *d_out, int nframes, int length)
{
    if (!c || !d_in || !d_out) return fail(QPSK_ERR_ARG, "qpsk_rrc_fir_batch: null argument");
    if (nframes <= 0 || length <= 0) return fail(QPSK_ERR_ARG, "qpsk_rrc_fir_batch: nframes %d length %d", nframes, length);
    if (bind(c)) return QPSK_ERR_HIP;
    const float *src = d_in;
    if (d_in == d_out) {
        /* rrc_fir() works in place (rrc_fir.c:28); a tiled kernel cannot, so filter from a copy */
        const size_t bytes = sizeof(float) * 2 * (size_t)nframes * length;
        int rc = ensure(c, c->mixed, bytes);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->mixed.p, d_in, bytes, hipMemcpyDeviceToDevice, c->stream));
        src = (const float *)c->mixed.p;
    }
    KERNEL_TRY(fir_full_rate(c, src, d_memory, d_out, nframes, length));
    if (d_memory) KERNEL_TRY(launch_delay_line(src, d_memory, nframes, length, c->stream));
    return QPSK_OK;
}

int qpsk_rrc_fir_batch_fast(qpsk_ctx *c, float *d_memory, const float *d_in, float *d_out, int nframes, int length)
{
    if (!c || !d_in || !d_out) return fail(QPSK_ERR_ARG, "qpsk_rrc_fir_batch_fast: null argument");
    if (nframes <= 0 || length <= 0) return fail(QPSK_ERR_ARG, "qpsk_rrc_fir_batch_fast: nframes %d length %d", nframes, length);
    if (d_in == d_out) return fail(QPSK_ERR_ARG, "qpsk_rrc_fir_batch_fast: every block reads 126 samples in front of it: separate buffers");
    if (bind(c)) return QPSK_ERR_HIP;
    if (!c->fast_valid) {      /* the filter's spectrum and the twiddles, in double on the host (host_math.c) */
        const int n = rrc_fir_fast_nfft();
        std::vector<float> t(4 * (size_t)n);
        qpsk_host_fir_fast_tables(c->taps, t.data(), t.data() + 2 * n);
        if (!c->d_fast) HIP_TRY(hipMalloc((void **)&c->d_fast, sizeof(float) * t.size()));
        HIP_TRY(hipStreamSynchronize(c->stream));      /* an earlier call may still read the old tables */
        HIP_TRY(hipMemcpy(c->d_fast, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice));
        c->fast_valid = true;
    }
    KERNEL_TRY(launch_rrc_fir_fast(d_in, d_memory, d_out, c->d_fast, c->d_fast + 2 * rrc_fir_fast_nfft(), nframes, length, c->stream));
    if (d_memory) KERNEL_TRY(launch_delay_line(d_in, d_memory, nframes, length, c->stream));
    return QPSK_OK;
}

int qpsk_timing_hist_batch(qpsk_ctx *c, const float *d_filtered, int nframes, int32_t *d_index, int32_t *d_hist)
{
    if (!c || !d_filtered || !d_index) return fail(QPSK_ERR_ARG, "qpsk_timing_hist_batch: null argument");
    if (nframes <= 0) return fail(QPSK_ERR_ARG, "nframes = %d", nframes);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_timing_hist(d_filtered, nframes, c->prm.frame_size, c->cycles, d_index, d_hist,
                                  tuned(c->tune.hist_generic, 0) == 2, c->stream));
    return QPSK_OK;
}

int qpsk_timing_scan_batch(qpsk_ctx *c, const float *d_in, int nframes, int32_t *d_index, int32_t *d_hist)
{
    if (!c || !d_in || !d_index) return fail(QPSK_ERR_ARG, "qpsk_timing_scan_batch: null argument");
    if (nframes <= 0) return fail(QPSK_ERR_ARG, "nframes = %d", nframes);
    if (bind(c)) return QPSK_ERR_HIP;
    if (!(c->cycles == 8 && c->prm.frame_size % timing_scan_tile() == 0 && ((uintptr_t)d_in % 16) == 0))
        return fail(QPSK_ERR_ARG, "qpsk_timing_scan_batch needs CYCLES = 8, frame_size %% %d == 0 and 16-byte aligned input "
                                  "(use qpsk_rrc_fir_batch + qpsk_timing_hist_batch otherwise)", timing_scan_tile());
    KERNEL_TRY(launch_timing_scan(d_in, nframes, c->prm.frame_size, c->d_taps, d_index, d_hist, c->d_status, c->stream, 0,
                                  c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0));
    return QPSK_OK;
}

int qpsk_timing_fft_batch(qpsk_ctx *c, const float *d_in, int nframes, int32_t *d_index, float *d_filtered, double *d_spectrum)
{
    if (!c || !d_in || !d_index) return fail(QPSK_ERR_ARG, "qpsk_timing_fft_batch: null argument");
    if (nframes <= 0) return fail(QPSK_ERR_ARG, "nframes = %d", nframes);
    if (bind(c)) return QPSK_ERR_HIP;
    return fft_timing_indices(c, d_in, nframes, d_index, d_filtered, d_spectrum);
}

int qpsk_timing_fft_bin_batch(qpsk_ctx *c, const float *d_in, int nframes, int32_t *d_index, float *d_filtered, double *d_bin)
{
    if (!c || !d_in || !d_index) return fail(QPSK_ERR_ARG, "qpsk_timing_fft_bin_batch: null argument");
    if (nframes <= 0) return fail(QPSK_ERR_ARG, "nframes = %d", nframes);
    if (bind(c)) return QPSK_ERR_HIP;
    return fft_timing_indices(c, d_in, nframes, d_index, d_filtered, nullptr, 0, d_bin);
}

/* the fourth-power carrier estimate (carrier_est.hip; definition in include/qpsk_hip.h).  S = { k : |k| < n / (2 CYCLES), min_freq <=
 * w(k) <= max_freq } is a contiguous range of k (w(k) is monotone in k): found here, once per call, with the kernel's own formula */
static float carrier_est_omega(int k, int C, int n)
{
    const double tau = 2.0 * 3.14159265358979323846;      /* qpsk.h:29, as the kernel's TAU */
    return (float)(tau * (double)(k * C) / (double)(4 * n));
}

int qpsk_carrier_est_batch(qpsk_ctx *c, const float *d_in, long long frame_pitch, int nframes, int start, int n, float *d_seed,
                           float *d_freq, int32_t *d_bin, double *d_line)
{
    if (!c || !d_in) return fail(QPSK_ERR_ARG, "qpsk_carrier_est_batch: null context or input");
    if (!d_seed && !d_freq && !d_bin && !d_line) return fail(QPSK_ERR_ARG, "qpsk_carrier_est_batch: every output is NULL");
    if (nframes <= 0) return fail(QPSK_ERR_ARG, "qpsk_carrier_est_batch: nframes = %d", nframes);
    if (n < 64 || n > 8192 || (n & (n - 1)))
        return fail(QPSK_ERR_ARG, "qpsk_carrier_est_batch: n = %d must be a power of two in 64..8192", n);
    const int fs = c->prm.frame_size;
    if (start < 0 || (long long)start + n > fs)
        return fail(QPSK_ERR_ARG, "qpsk_carrier_est_batch: start %d + n %d outside the frame (%d samples)", start, n, fs);
    if (frame_pitch == 0) frame_pitch = fs;
    if (frame_pitch < fs || (frame_pitch % 2) != 0)
        return fail(QPSK_ERR_ARG, "qpsk_carrier_est_batch: frame_pitch = %lld (0, or even and >= frame_size %d)", frame_pitch, fs);
    const int C = c->cycles;
    int klo = 1, khi = 0;
    for (int k = -(n / (2 * C)); k <= n / (2 * C); k++) {
        if ((long long)(k < 0 ? -k : k) * 2 * C >= n) continue;
        const float w = carrier_est_omega(k, C, n);
        if (!(w >= c->min_freq && w <= c->max_freq)) continue;
        if (klo > khi) klo = k;
        khi = k;
    }
    if (klo > khi)
        return fail(QPSK_ERR_ARG, "qpsk_carrier_est_batch: no bin |k| < n / (2 CYCLES) = %d / %d lies in the loop clamp [%g, %g]", n, 2 * C,
                    (double)c->min_freq, (double)c->max_freq);
    const int kdef = klo <= 0 && khi >= 0 ? 0 : (khi < 0 ? khi : klo);
    if (bind(c)) return QPSK_ERR_HIP;
    double *tw = nullptr;
    if (int rt = get_twiddles(c, n, &tw)) return rt;
    KERNEL_TRY(launch_carrier_est(d_in, (size_t)frame_pitch, nframes, start, n, C, klo, khi, kdef, c->d_taps, tw, d_seed, d_freq, d_bin,
                                  d_line, c->d_status, c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0, c->stream));
    c->last_kernel = "carrier_est_kernel";
    return QPSK_OK;
}

/* soft decisions and signal quality per row of costas_frame[] (soft.hip; definition in include/qpsk_hip.h).  Rows up to SOFT_ONE_PASS_MAX
 * symbols that need both the sums and the soft output are read once (soft_onepass_kernel); longer rows take sums, then soft */
int qpsk_soft_batch(qpsk_ctx *c, const float *d_costas, long long row_pitch, int nrows, int nsym, int skip, int mode, float scale,
                    const float *d_gain_in, const int32_t *d_lag, const int32_t *d_rot, int first, int nout, int8_t *d_soft,
                    float *d_quality, double *d_sums)
{
    if (!c || !d_costas) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: null context or input");
    if (!d_soft && !d_quality && !d_sums) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: every output is NULL");
    if (nrows <= 0 || nsym <= 0 || nsym > SOFT_MAX_NSYM)
        return fail(QPSK_ERR_ARG, "qpsk_soft_batch: nrows = %d, nsym = %d (1..%d)", nrows, nsym, SOFT_MAX_NSYM);
    if (skip < 0 || skip >= nsym) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: skip = %d outside 0..%d", skip, nsym - 1);
    if (mode != QPSK_SOFT_UNIT && mode != QPSK_SOFT_LLR) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: unknown mode %d", mode);
    if (!(scale > 0.0f && scale <= 3.402823466e+38f)) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: scale = %g is not finite and > 0", (double)scale);
    if (row_pitch == 0) row_pitch = nsym;
    if (row_pitch < nsym) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: row_pitch = %lld (0, or >= nsym %d)", row_pitch, nsym);
    if ((uintptr_t)d_costas % 8) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: d_costas is not 8-byte aligned");
    if (d_soft) {
        if (nout < 0 || first < 0 || (long long)first + nout > nsym)
            return fail(QPSK_ERR_ARG, "qpsk_soft_batch: first %d, nout %d do not fit a row of %d", first, nout, nsym);
        if ((uintptr_t)d_soft % 2) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: d_soft is not 2-byte aligned");
        const uintptr_t o0 = (uintptr_t)d_soft, o1 = o0 + 2 * (size_t)nrows * (size_t)nout;
        const uintptr_t i0 = (uintptr_t)d_costas, i1 = i0 + 8 * ((size_t)(nrows - 1) * (size_t)row_pitch + (size_t)nsym);
        if (o0 < i1 && i0 < o1) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: d_soft overlaps d_costas");
    }
    static_assert(QPSK_SOFT_UNIT == SOFT_MODE_UNIT && QPSK_SOFT_LLR == SOFT_MODE_LLR, "the kernels take the header's mode values");
    if (bind(c)) return QPSK_ERR_HIP;
    const size_t pitch = (size_t)row_pitch;
    const bool need_sums = d_quality || d_sums || !d_gain_in;
    if (!d_soft) {
        KERNEL_TRY(launch_soft_sums(d_costas, pitch, nrows, nsym, skip, mode, scale, nullptr, d_quality, d_sums, c->d_status, c->stream));
        c->last_kernel = "soft_sums_kernel";
    } else if (!need_sums) {
        KERNEL_TRY(launch_soft_apply(d_costas, pitch, nrows, nsym, d_gain_in, true, d_lag, d_rot, first, nout, d_soft, c->d_status, c->stream));
        c->last_kernel = "soft_apply_kernel";
    } else if (nsym <= SOFT_ONE_PASS_MAX) {
        KERNEL_TRY(launch_soft_onepass(d_costas, pitch, nrows, nsym, skip, mode, scale, d_gain_in, d_lag, d_rot, first, nout, d_soft, d_quality,
                                       d_sums, c->d_status, c->stream));
        c->last_kernel = "soft_onepass_kernel";
    } else {
        float *gain = nullptr;
        if (!d_gain_in) {
            if (int rg = ensure(c, c->softgain, sizeof(float) * (size_t)nrows)) return rg;
            gain = (float *)c->softgain.p;
        }
        KERNEL_TRY(launch_soft_sums(d_costas, pitch, nrows, nsym, skip, mode, scale, gain, d_quality, d_sums, c->d_status, c->stream));
        KERNEL_TRY(launch_soft_apply(d_costas, pitch, nrows, nsym, d_gain_in ? d_gain_in : gain, d_gain_in != nullptr, d_lag, d_rot, first, nout,
                                     d_soft, c->d_status, c->stream));
        c->last_kernel = "soft_sums_kernel + soft_apply_kernel";
    }
    return QPSK_OK;
}

/* PUNCTURING (include/qpsk_hip.h): the pattern of a call, checked; who = the entry point's name */
static int punct_make(const char *who, int period, uint32_t keep0, uint32_t keep1, Puncture *p)
{
    if (period < 1 || period > 32) return fail(QPSK_ERR_ARG, "%s: period = %d outside 1..32", who, period);
    const uint32_t above = period == 32 ? 0u : ~((1u << period) - 1u);
    if ((keep0 | keep1) & above) return fail(QPSK_ERR_ARG, "%s: keep0 = 0x%x / keep1 = 0x%x has a bit at or above period %d", who, keep0, keep1, period);
    if (!(keep0 | keep1)) return fail(QPSK_ERR_ARG, "%s: keep0 and keep1 are both 0: nothing would be sent", who);
    *p = Puncture{period, keep0, keep1, __builtin_popcount(keep0) + __builtin_popcount(keep1)};
    return QPSK_OK;
}

/* INTERLEAVING (include/qpsk_hip.h): the stride of a call over the ntx transmitted dibits of its rows, checked; who = the entry point's name */
static int ilv_make(const char *who, long long ntx, int stride, Interleave *v)
{
    if (ntx < 1) return fail(QPSK_ERR_ARG, "%s: nothing is sent (ntx = 0), so there is nothing to interleave", who);
    const unsigned n = 2u * (unsigned)ntx;
    if (stride < 1 || (unsigned)stride >= std::max(n, 2u)) return fail(QPSK_ERR_ARG, "%s: stride = %d outside 1..%u", who, stride, std::max(n, 2u) - 1);
    if (qpsk_host_gcd((unsigned)stride, n) != 1) return fail(QPSK_ERR_ARG, "%s: stride = %d is not coprime to the row's %u bits", who, stride, n);
    *v = Interleave{n, (unsigned)stride, qpsk_host_mod_inverse((unsigned)stride, n)};
    return QPSK_OK;
}

/* a pattern as the entry points take it */
struct Pattern {
    int period;
    uint32_t keep0, keep1;
};

/* The layout of a call's rows (kernels.h, CodedLayout) is made layer by layer, each layer checked as it is added, and the kind follows the
 * arguments the entry point has, never their values.  An entry point takes the two steps where its own checks have always had them: the
 * pattern first, the stride once nsteps is known to be in range.  NULL adds nothing.
 * layout_add_pattern: a plain *l becomes punctured */
static int layout_add_pattern(const char *who, const Pattern *pattern, CodedLayout *l)
{
    if (!pattern) return QPSK_OK;
    if (int rc = punct_make(who, pattern->period, pattern->keep0, pattern->keep1, &l->punct)) return rc;
    l->kind = CODED_PUNCT;
    return QPSK_OK;
}
/* layout_add_stride: *l becomes interleaved over the ntx dibits its nsteps steps have on air */
static int layout_add_stride(const char *who, int nsteps, const int *stride, CodedLayout *l)
{
    if (!stride) return QPSK_OK;
    if (int rc = ilv_make(who, coded_ndibits(*l, nsteps), *stride, &l->ilv)) return rc;
    l->kind = CODED_ILV;
    return QPSK_OK;
}
/* both at once, where nothing lies between them */
static int coded_layout_make(const char *who, int nsteps, const Pattern *pattern, const int *stride, CodedLayout *l)
{
    if (int rc = layout_add_pattern(who, pattern, l)) return rc;
    return layout_add_stride(who, nsteps, stride, l);
}

int qpsk_punct_ntx(int nsteps, int period, uint32_t keep0, uint32_t keep1)
{
    const Pattern pattern = {period, keep0, keep1};
    CodedLayout l;
    if (int rc = layout_add_pattern("qpsk_punct_ntx", &pattern, &l)) return rc;
    if (nsteps < 1 || nsteps > VITERBI_MAX_STEPS) return fail(QPSK_ERR_ARG, "qpsk_punct_ntx: nsteps = %d (1..%d)", nsteps, VITERBI_MAX_STEPS);
    return (int)coded_ndibits(l, nsteps);
}

int qpsk_ilv_stride(int nbits, int want)
{
    if (nbits < 2 || want < 1) return fail(QPSK_ERR_ARG, "qpsk_ilv_stride: nbits = %d (>= 2), want = %d (>= 1)", nbits, want);
    int s = std::min(want, nbits - 1);
    while (qpsk_host_gcd((unsigned)s, (unsigned)nbits) != 1) s++;      /* gcd(nbits - 1, nbits) = 1 ends it */
    return s;
}

/* the K = 7, rate-1/2 convolutional code (viterbi.hip; definition in include/qpsk_hip.h).  The three encoders: who = the entry point's name, the
 * layout from what it takes.  A punctured row of which nothing is sent is no launch; behind a stride coded_layout_make has refused it */
static int conv_encode_impl(qpsk_ctx *c, const char *who, const uint8_t *d_bits, int nrows, int nbits, int flags, const Pattern *pattern,
                            const int *stride, uint8_t *d_dibits)
{
    static const char *const label[] = {"conv_encode_kernel", "conv_encode_punct_kernel", "conv_encode_ilv_kernel"};
    if (!c || !d_bits || !d_dibits) return fail(QPSK_ERR_ARG, "%s: null argument", who);
    if (flags & ~QPSK_CONV_TAIL) return fail(QPSK_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    const int tail = (flags & QPSK_CONV_TAIL) ? 6 : 0;
    if (nrows <= 0 || nbits <= 0 || nbits > VITERBI_MAX_STEPS - tail)
        return fail(QPSK_ERR_ARG, "%s: nrows = %d, nbits = %d (1..%d)", who, nrows, nbits, VITERBI_MAX_STEPS - tail);
    CodedLayout l;
    if (int rc = coded_layout_make(who, nbits + tail, pattern, stride, &l)) return rc;
    if (bind(c)) return QPSK_ERR_HIP;
    if (coded_nsent(l, nbits + tail) == 0) return QPSK_OK;      /* every step of so short a row is deleted: nothing is sent */
    KERNEL_TRY(launch_conv_encode(d_bits, nrows, nbits, nbits + tail, l, d_dibits, c->stream));
    c->last_kernel = label[l.kind];
    return QPSK_OK;
}

int qpsk_conv_encode_batch(qpsk_ctx *c, const uint8_t *d_bits, int nrows, int nbits, int flags, uint8_t *d_dibits)
{
    return conv_encode_impl(c, "qpsk_conv_encode_batch", d_bits, nrows, nbits, flags, nullptr, nullptr, d_dibits);
}

int qpsk_conv_encode_punct_batch(qpsk_ctx *c, const uint8_t *d_bits, int nrows, int nbits, int flags, int period, uint32_t keep0, uint32_t keep1,
                                 uint8_t *d_dibits)
{
    const Pattern pattern = {period, keep0, keep1};
    return conv_encode_impl(c, "qpsk_conv_encode_punct_batch", d_bits, nrows, nbits, flags, &pattern, nullptr, d_dibits);
}

int qpsk_conv_encode_ilv_batch(qpsk_ctx *c, const uint8_t *d_bits, int nrows, int nbits, int flags, int period, uint32_t keep0, uint32_t keep1,
                               int stride, uint8_t *d_dibits)
{
    const Pattern pattern = {period, keep0, keep1};
    return conv_encode_impl(c, "qpsk_conv_encode_ilv_batch", d_bits, nrows, nbits, flags, &pattern, &stride, d_dibits);
}

/* Where the decision words (8 bytes per step) wait for the trace-back: in LDS when a row's fit the launch limit and -- the library's own
 * choice -- every row of the call is resident at once (160 KB of LDS per compute unit), so that the LDS never costs a second round of
 * workgroups; otherwise in the context's scratch buffer, rows in chunks of at most VITERBI_SCRATCH_MAX bytes of it */
static const size_t VITERBI_SCRATCH_MAX = (size_t)1 << 30;

/* the rule for `rows` rows of nsteps steps, whatever their layout: per_row = the decision words' bytes; chunk_rows = rows per launch, what
 * VITERBI_SCRATCH_MAX allows (one row at least), on the scratch route fewer where QPSK_VITERBI_CHUNK_ROWS says so -- the key can only lower
 * the cap, so the scratch buffer never grows by it */
struct ViterbiRoute {
    size_t per_row;
    bool lds;
    size_t chunk_rows;
};
static ViterbiRoute viterbi_route(const qpsk_ctx *c, size_t rows, int nsteps)
{
    const size_t per_row = viterbi_scratch_bytes_per_row(nsteps);
    const bool fits = per_row <= (size_t)VITERBI_LDS_MAX_BYTES;
    const bool resident = fits && rows <= (size_t)c->ncu * (((size_t)160 << 10) / per_row);
    const bool lds = fits && tuned(c->tune.viterbi_lds, resident ? 1 : 0) != 0;
    size_t cap = std::max<size_t>(1, VITERBI_SCRATCH_MAX / per_row);
    if (!lds && c->tune.viterbi_chunk_rows >= 1) cap = std::min<size_t>(cap, (size_t)c->tune.viterbi_chunk_rows);
    return ViterbiRoute{per_row, lds, std::min<size_t>(rows, cap)};
}

/* the three decoders: who = the entry point's name, the layout from what it takes.  Behind a pattern the rows hold the ntx transmitted dibits
 * of nsteps steps, and row_pitch and d_flip go by ntx.  The pattern is checked first, as the entry points always have; the stride once nsteps
 * is known to be in range */
static int viterbi_impl(qpsk_ctx *c, const char *who, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, const Pattern *pattern,
                        const int *stride, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info)
{
    static const char *const label[][2] = {{"viterbi_kernel", "viterbi_lds_kernel"},
                                           {"viterbi_punct_kernel", "viterbi_punct_lds_kernel"},
                                           {"viterbi_ilv_kernel", "viterbi_ilv_lds_kernel"}};
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context or input", who);
    c->viterbi_launches = 0;      /* a refused call made none */
    CodedLayout l;
    if (int rc = layout_add_pattern(who, pattern, &l)) return rc;
    if (!d_soft) return fail(QPSK_ERR_ARG, "%s: null context or input", who);
    if (!d_bits && !d_info) return fail(QPSK_ERR_ARG, "%s: every output is NULL", who);
    if (nrows <= 0 || nsteps <= 0 || nsteps > VITERBI_MAX_STEPS)
        return fail(QPSK_ERR_ARG, "%s: nrows = %d, nsteps = %d (1..%d)", who, nrows, nsteps, VITERBI_MAX_STEPS);
#ifdef QPSK_VITERBI_PROFILE
    const int known = QPSK_VITERBI_OPEN_START | QPSK_VITERBI_OPEN_END | VITERBI_PROFILE_FORWARD_ONLY | VITERBI_PROFILE_CYCLES;
#else
    const int known = QPSK_VITERBI_OPEN_START | QPSK_VITERBI_OPEN_END;
#endif
    if (flags & ~known) return fail(QPSK_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    const long long nrow = coded_ndibits(l, nsteps);      /* the dibits of a row */
    if (row_pitch == 0) row_pitch = nrow;
    if (row_pitch < nrow) return fail(QPSK_ERR_ARG, "%s: row_pitch = %lld (0, or >= %s %lld)", who, row_pitch, pattern ? "ntx" : "nsteps", nrow);
    if ((uintptr_t)d_soft % 2) return fail(QPSK_ERR_ARG, "%s: d_soft is not 2-byte aligned", who);
    if ((uintptr_t)d_info % 4) return fail(QPSK_ERR_ARG, "%s: d_info is not 4-byte aligned", who);
    if (int rc = layout_add_stride(who, nsteps, stride, &l)) return rc;
    static_assert(QPSK_VITERBI_OPEN_START == VITERBI_OPEN_START && QPSK_VITERBI_OPEN_END == VITERBI_OPEN_END, "the kernel takes the header's flag values");
    if (bind(c)) return QPSK_ERR_HIP;
    const ViterbiRoute route = viterbi_route(c, (size_t)nrows, nsteps);
    /* one launch of rows [r0, r0 + n) */
    const auto launch = [&](size_t r0, int n, unsigned long long *scratch) {
        return launch_viterbi(d_soft + 2 * r0 * (size_t)row_pitch, (size_t)row_pitch, n, nsteps, l, d_flip, flags, scratch, route.lds,
                              d_bits ? d_bits + r0 * (((size_t)nsteps + 7) / 8) : nullptr, d_info ? d_info + 4 * r0 : nullptr, c->stream);
    };
    if (route.lds) {      /* nothing to chunk for: one launch */
        KERNEL_TRY(launch(0, nrows, nullptr));
        c->viterbi_launches = 1;
    } else {
        if (int rg = ensure(c, c->vitdec, route.chunk_rows * route.per_row)) return rg;
        for (size_t r0 = 0; r0 < (size_t)nrows; r0 += route.chunk_rows) {      /* stream order: a chunk's trace-back is over before the next one's forward pass */
            KERNEL_TRY(launch(r0, (int)std::min<size_t>(route.chunk_rows, (size_t)nrows - r0), (unsigned long long *)c->vitdec.p));
            c->viterbi_launches++;
        }
    }
    c->last_kernel = label[l.kind][route.lds];
    return QPSK_OK;
}

int qpsk_viterbi_batch(qpsk_ctx *c, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, const uint8_t *d_flip, int flags,
                       uint8_t *d_bits, int32_t *d_info)
{
    return viterbi_impl(c, "qpsk_viterbi_batch", d_soft, row_pitch, nrows, nsteps, nullptr, nullptr, d_flip, flags, d_bits, d_info);
}

int qpsk_viterbi_punct_batch(qpsk_ctx *c, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, int period, uint32_t keep0,
                             uint32_t keep1, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info)
{
    const Pattern pattern = {period, keep0, keep1};
    return viterbi_impl(c, "qpsk_viterbi_punct_batch", d_soft, row_pitch, nrows, nsteps, &pattern, nullptr, d_flip, flags, d_bits, d_info);
}

int qpsk_viterbi_ilv_batch(qpsk_ctx *c, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, int period, uint32_t keep0,
                           uint32_t keep1, int stride, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info)
{
    const Pattern pattern = {period, keep0, keep1};
    return viterbi_impl(c, "qpsk_viterbi_ilv_batch", d_soft, row_pitch, nrows, nsteps, &pattern, &stride, d_flip, flags, d_bits, d_info);
}

int qpsk_costas_batch(qpsk_ctx *c, const float *d_symbols_in, int nframes, int nsym, float *d_state, uint8_t *d_sym,
                      float *d_costas)
{
    if (!c || !d_symbols_in) return fail(QPSK_ERR_ARG, "qpsk_costas_batch: null argument");
    if (nframes <= 0 || nsym <= 0) return fail(QPSK_ERR_ARG, "nframes %d nsym %d", nframes, nsym);
    if (bind(c)) return QPSK_ERR_HIP;
    if (int rg = use_context_gains(c)) return rg;
    /* no refill: the rows are only read */
    return costas_over_symbols(c, const_cast<float *>(d_symbols_in), nframes, nsym, nsym, d_state, d_sym, d_costas);
}

int qpsk_fft_batch(qpsk_ctx *c, const double *d_in, double *d_out, int nbatch, int n, int inverse)
{
    if (!c || !d_in || !d_out) return fail(QPSK_ERR_ARG, "qpsk_fft_batch: null argument");
    if (nbatch <= 0 || n < 1 || (n & (n - 1))) return fail(QPSK_ERR_ARG, "n = %d must be a power of two, nbatch %d > 0", n, nbatch);
    if (n > (1 << 21)) return fail(QPSK_ERR_ARG, "n = %d: transforms above 2^21 points are not supported (the late stages' tile must fit the LDS)", n);
    if (bind(c)) return QPSK_ERR_HIP;
    int log2n = 0;
    while ((1 << log2n) < n) log2n++;
    if (n <= fft_lds_max_n()) {   /* one workgroup per transform, LDS-resident */
        double *tw = nullptr;
        if (int rt = get_twiddles(c, n, &tw)) return rt;
        KERNEL_TRY(launch_fft(d_in, d_out, tw, nbatch, n, log2n, inverse ? 1 : 0, c->stream));
        return QPSK_OK;
    }
    /* two passes over global memory (kernels.hip, fft_big_*); the first gathers bit-reversed, so it cannot run in place */
    double *twb = nullptr, *twn = nullptr;
    if (int rt = get_twiddles(c, fft_big_block(), &twb)) return rt;
    if (int rt = get_twiddles(c, n, &twn)) return rt;
    const double *src = d_in;
    if (d_in == d_out) {
        const size_t bytes = sizeof(double) * 2 * (size_t)nbatch * n;
        int rc = ensure(c, c->mixed, bytes);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->mixed.p, d_in, bytes, hipMemcpyDeviceToDevice, c->stream));
        src = (const double *)c->mixed.p;
    }
    KERNEL_TRY(launch_fft_big(src, d_out, twb, twn, nbatch, n, log2n, inverse ? 1 : 0, c->stream));
    return QPSK_OK;
}

/* --------------------------------------------------------------- streams */
/* A stream call enqueues several launches and keeps host-side books about them (which carrier table is current, the relay's turn, a
 * table half built).  If it fails between its launches -- or a kernel reports that it gave up (QPSK_ERR_HIP from the status word) -- the
 * carried state of the streams is undefined: the shared carrier is dropped and every later stream call is refused until
 * qpsk_streams_reset().  Argument errors and flagged NUMBERS (QPSK_ERR_RANGE: NaN samples, a phase beyond the bounded wrap) do not
 * poison: the kernels completed and the state is what the reference's would be or fenced as documented. */
static int stream_call_done(qpsk_ctx *c, int rc)
{
    if (rc == QPSK_ERR_HIP || rc == QPSK_ERR_ALLOC) {
        c->streams_poisoned = true;
        c->carrier_shared = false;
        c->carrier_pending = nullptr;
    }
    return rc;
}

static int streams_usable(qpsk_ctx *c, const char *who)
{
    if (c->nstreams <= 0) return fail(QPSK_ERR_STATE, "call qpsk_streams_reset() first");
    if (c->streams_poisoned)
        return fail(QPSK_ERR_STATE, "%s: an earlier stream call failed between its launches; the streams' carried state is undefined until qpsk_streams_reset()", who);
    c->stream_work_unchecked = true;      /* every caller goes on to enqueue stream work (or to read what such work left) */
    return QPSK_OK;
}

/* ---- which kernels take a block of the running streams: decided ONCE per call, as a route (rx_route()'s twin).  stream_route() only
 * reads -- the context is const, so it cannot launch, allocate or touch the carrier's books, last_kernel or streams_poisoned -- and
 * stream_run() and the host entry execute what it says.  tests/test_stream_route_gpu.py pins the route on either side of every threshold. */
enum StreamKind { SK_BLOCK, SK_SCAN, SK_APART };      /* stream_block_kernel; stream_scan_kernel + costas_pipe_kernel; the kernels apart */
struct StreamRoute {
    StreamKind kind = SK_APART;
    bool mixer = false;        /* PCM that neither kernel takes: mixer_kernel first, and kind is the route of the MIXED block, as complex input */
    bool carrier = false;      /* the launch that reads the PCM takes its phases from the streams' one carrier table (carrier.h) */
};

/* One launch per block (streamblock.hip) instead of the five-kernel composition: few, short streams -- the reference's call
 * pattern, where the launches are the cost.  Histogram or fixed timing (the FFT estimate keeps its own kernel). */
static bool stream_block_ok(const qpsk_ctx *c, bool pcm)
{
    const int t = tuned(c->tune.stream_block, -1);
    if (t == 0 || c->prm.timing_mode == QPSK_TIMING_FFT || c->prm.frame_size > stream_block_max_frame() ||
        c->nsym * c->cycles > c->prm.frame_size || tuned(c->tune.generic, 0) != 0 ||
        stream_block_lds_bytes(c->prm.frame_size, c->nsym) > (size_t)MAX_LDS_BYTES)
        return false;
    /* [measured, profiles/r04_streams_short_blocks.txt: PCM streams back to back] the kernels apart cost 70 us (512-sample blocks) to
     * 220 us (2048) whatever the count -- launches and serial chains -- and this kernel ~17 us + 13.5 ns per 512 samples of a stream:
     * it wins up to ~4 M samples per block of all streams (7800 x 512, 4400 x 1024, 2400 x 2048).  Complex input: round 4's first rule */
    const long long nl = (long long)c->nstreams * c->prm.frame_size;
    /* complex input has no carrier chain in front of it: at CYCLES = 8 the kernels apart (hand-scheduled filter, 8-lane scan) take 29 us
     * at 1024 x 512 and 55 us at 256 x 2048, where this kernel takes 27 and 73 -- it keeps the small batches (<= 0.4 M samples); at other
     * rates the kernels apart run the generic scan (72 us at 2048 x 512 against 40 here) and the PCM rule holds */
    return t == 1 || (pcm || c->cycles != 8 ? nl <= 3500000LL : nl <= 400000LL);
}

/* Many streams, histogram timing: mixer, filter and scan as ONE kernel (streamscan.hip) -- the carrier recurrences run a tile ahead
 * of the filter waves of the same workgroup, PCM comes in at 2 bytes per sample, no mixed block goes through HBM and the scan
 * reads the filtered samples from LDS.  A workgroup takes 16 streams through the whole block (its time does not shrink with the
 * batch), so it pays from about 2500 streams on; below that the kernels apart are quicker. */
static bool stream_scan_ok(const qpsk_ctx *c, bool pcm, bool shared_carrier)
{
    /* [measured, profiles/r04_streams_blocks.txt] 2560 streams: PCM input 0.94 against 1.03 ms per block with the kernels apart, complex
     * input 0.79 against 0.70; 4096 streams: 1.00 against 1.27 and 0.92 against 1.01.  With the streams' one carrier from the table
     * (MODE 2: no mixer wave, no mixer kernel) PCM input pays from 1024 streams on: 0.73 against 0.79 ms there, 0.75 against 0.93 at
     * 2048, 0.76 against 1.00 at 2560 (profiles/r04_streams_carrier.txt) */
    const int from = pcm ? (shared_carrier ? 1024 : 2560) : 3584;
    bool wanted = c->nstreams >= from;
    /* short blocks (the one-launch kernel's range), shared carrier: a workgroup's time shrinks with the block, so the kernel pays from
     * ~1.4 M samples per block of all streams on -- 106.7 us against 151.9 (one launch per block) and 117.1 (kernels apart) at
     * 1024 x 2048, 61.8 against 95.9 and 80.6 at 2048 x 1024, 41.7 against 71.7 and 61.8 at 4096 x 512; below that the one-launch
     * kernel is ahead (profiles/r04_streams_short_blocks.txt) */
    if (pcm && shared_carrier && c->prm.frame_size <= stream_block_max_frame())
        wanted = (long long)c->nstreams * c->prm.frame_size >= 1400000LL && c->nstreams >= 256;
    return c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0 && tuned(c->tune.generic, 0) == 0 && (c->cycles == 8 || c->cycles == 4) &&
           (c->prm.timing_mode == QPSK_TIMING_HIST || c->prm.timing_mode == QPSK_TIMING_FIXED) && c->prm.frame_size % stream_scan_tile() == 0 &&
           tuned(c->tune.stream_scan, wanted ? 1 : 0) != 0;
}

/* pcm: in is int16 PCM, otherwise complex float samples; want_sym: the caller takes the symbols (the one-launch kernel always writes them) */
static void stream_route(const qpsk_ctx *c, bool pcm, const void *in, bool want_sym, StreamRoute *rt)
{
    *rt = StreamRoute{};
    rt->carrier = pcm && c->carrier_shared && tuned(c->tune.stream_carrier, 1) != 0;      /* the one carrier is in use */
    bool aligned = (uintptr_t)in % (pcm ? 4 : 16) == 0;      /* what stream_scan_kernel loads: 4 bytes of PCM, 16 of complex samples */
    for (;;) {
        const bool scan = aligned && stream_scan_ok(c, pcm, rt->carrier);
        /* streams that both stream_scan_kernel and the one-launch kernel would take: which of the two */
        const bool block = want_sym && stream_block_ok(c, pcm) && !(scan && tuned(c->tune.stream_block, -1) != 1);
        rt->kind = block ? SK_BLOCK : scan ? SK_SCAN : SK_APART;
        if (!pcm || rt->kind != SK_APART) return;
        /* PCM that neither kernel takes: mixer_kernel in front, and a second decision for the mixed block -- complex input like a caller's,
         * so many streams of it still go to stream_scan_kernel.  Its alignment needs no pointer: the block lies at the start of the
         * context's `mixed` buffer, which hipMalloc (ensure()) aligns to 256 bytes whenever it comes to be allocated */
        rt->mixer = aligned = true;
        rt->carrier = pcm = false;
    }
}

int qpsk_streams_reset(qpsk_ctx *c, int nstreams, double mixer_hz)
{
    if (!c || nstreams <= 0) return fail(QPSK_ERR_ARG, "qpsk_streams_reset: bad argument");
    if (bind(c)) return QPSK_ERR_HIP;
    /* poisoned until this call has COMPLETED: a reset that fails half way (a launch, the last synchronisation) must not leave
     * streams that look usable over half-initialised state */
    c->streams_poisoned = true;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nstreams != c->nstreams) {
        free_streams(c);
        const size_t n = (size_t)nstreams;
        if (hipMalloc((void **)&c->s_memory, sizeof(float) * 2 * QPSK_NTAPS * n) != hipSuccess ||
            hipMalloc((void **)&c->s_dec, sizeof(float) * 2 * c->nsym * n) != hipSuccess ||
            hipMalloc((void **)&c->s_loop, sizeof(float) * 2 * n) != hipSuccess ||
            hipMalloc((void **)&c->s_ctab, sizeof(float) * 2 * 2 * (size_t)c->prm.frame_size) != hipSuccess ||
            hipMalloc((void **)&c->s_cstate, sizeof(float) * 8) != hipSuccess ||
            hipMalloc((void **)&c->s_mixer, sizeof(float) * 4 * n) != hipSuccess) {
            free_streams(c);
            return fail(QPSK_ERR_ALLOC, "hipMalloc of stream state failed");
        }
        c->nstreams = nstreams;
    }
    const size_t n = (size_t)nstreams;
    HIP_TRY(hipMemsetAsync(c->s_memory, 0, sizeof(float) * 2 * QPSK_NTAPS * n, c->stream));
    HIP_TRY(hipMemsetAsync(c->s_dec, 0, sizeof(float) * 2 * c->nsym * n, c->stream));
    HIP_TRY(hipMemsetAsync(c->s_loop, 0, sizeof(float) * 2 * n, c->stream));
    /* fbb_rx_phase = cmplx(0.0f); fbb_rx_rect = cmplxconj(TAU * hz / FS)  (qpsk.c:341-342) */
    float rect[2];
    qpsk_host_rect(mixer_hz, c->prm.fs, rect);
    std::vector<float> m(4 * n);
    for (size_t i = 0; i < n; i++) { m[4 * i] = 1.0f; m[4 * i + 1] = 0.0f; m[4 * i + 2] = rect[0]; m[4 * i + 3] = rect[1]; }
    HIP_TRY(hipMemcpyAsync(c->s_mixer, m.data(), sizeof(float) * m.size(), hipMemcpyHostToDevice, c->stream));
    /* one carrier for all of them: the first block's phases now, every later block's by the block before it (streamscan.hip MODE 2) */
    const float cst[8] = {1.0f, 0.0f, rect[0], rect[1], 1.0f, 0.0f, 0.0f, 0.0f};
    HIP_TRY(hipMemcpyAsync(c->s_cstate, cst, sizeof cst, hipMemcpyHostToDevice, c->stream));
    c->carrier_shared = false;
    c->carrier_blocks = 0;
    c->carrier_scans = 0;
    c->carrier_pending = nullptr;
    if (c->prm.frame_size % 2 == 0 && (stream_scan_ok(c, true, true) || stream_block_ok(c, true))) {      /* (a kernel that uses it would take these streams) */
        KERNEL_TRY(launch_carrier_table(c->s_cstate, c->s_ctab, c->prm.frame_size, false, c->stream));
        c->carrier_shared = true;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* the one-launch kernel's wave counter: whatever an earlier, failed call left between the host's expectation and the device's count
     * (a polled call whose synchronisation failed had already advanced done_expect), the stream is idle now: back in step */
    if (c->h_done) c->done_expect = *(volatile unsigned *)c->h_done;
    (void)__atomic_exchange_n(c->h_status, 0, __ATOMIC_ACQ_REL);      /* a status word left by the call that poisoned the streams belongs to it */
    c->streams_poisoned = false;
    return QPSK_OK;
}

/* the shared carrier ends: every stream's mixer state = the phase the next block starts from (before any other reader of s_mixer) */
static int carrier_to_streams(qpsk_ctx *c)
{
    if (!c->carrier_shared) return QPSK_OK;
    KERNEL_TRY(launch_carrier_broadcast(c->s_cstate, c->s_mixer, c->nstreams, c->stream));
    c->carrier_shared = false;
    return QPSK_OK;
}

/* In front of a launch that reads PCM.  use (StreamRoute::carrier): *cur = the table of this block's phases, *next = the one the launch fills for
 * the block after it (s_ctab's halves take turns; the caller commits the books once its launch is in the stream).  Otherwise both stay NULL:
 * the launch runs every stream's own mixer state, and the carrier, if there was one, ends here */
static int stream_carrier(qpsk_ctx *c, bool use, const float **cur, float **next)
{
    *cur = *next = nullptr;
    if (!use) return carrier_to_streams(c);
    const size_t L2 = 2 * (size_t)c->prm.frame_size;
    *cur = c->s_ctab + L2 * (c->carrier_blocks & 1u);
    *next = c->s_ctab + L2 * ((c->carrier_blocks + 1u) & 1u);
    return QPSK_OK;
}

int qpsk_streams_set_loop_state(qpsk_ctx *c, const float *h_state)
{
    if (!c || !h_state) return fail(QPSK_ERR_ARG, "null argument");
    if (int ru = streams_usable(c, "qpsk_streams_set_loop_state")) return ru;
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(c->s_loop, h_state, sizeof(float) * 2 * (size_t)c->nstreams, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QPSK_OK;
}

int qpsk_streams_get_loop_state(qpsk_ctx *c, float *h_state)
{
    if (!c || !h_state) return fail(QPSK_ERR_ARG, "null argument");
    if (int ru = streams_usable(c, "qpsk_streams_get_loop_state")) return ru;
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(h_state, c->s_loop, sizeof(float) * 2 * (size_t)c->nstreams, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return check_status(c);
}

/* pcm / cplx: exactly one of them; every pointer device-visible (device memory or mapped pinned host memory) */
static int streams_block_launch(qpsk_ctx *c, const StreamRoute &rt, const int16_t *pcm, const float *cplx, const float *loop_in, float *loop_out,
                                uint8_t *sym, float *costas, int32_t *index, const StreamBlockInline *inl = nullptr, bool count = false)
{
    if (int rg = use_context_gains(c)) return rg;
    StreamBlockArgs a{};
    /* the streams' one carrier (carrier.h): this block's phases from the table, the next block's by workgroup 0's third wave */
    const float *ctab = nullptr;
    float *ctab_next = nullptr;
    if (pcm)
        if (int rb = stream_carrier(c, rt.carrier, &ctab, &ctab_next)) return rb;
    a.ctab = reinterpret_cast<const float2 *>(ctab);
    a.ctab_next = reinterpret_cast<float2 *>(ctab_next);
    a.cstate = ctab ? c->s_cstate : nullptr;
    a.pcm = pcm;
    a.cplx = reinterpret_cast<const float2 *>(cplx);
    a.mixer = c->s_mixer;
    a.memory = reinterpret_cast<float2 *>(c->s_memory);
    a.dec = reinterpret_cast<float2 *>(c->s_dec);
    a.loop = c->s_loop;
    a.loop_in = loop_in;
    a.loop_out = loop_out;
    a.taps = c->d_taps;
    a.gains = c->d_gains;
    a.min_freq = c->min_freq;
    a.max_freq = c->max_freq;
    a.frame_size = c->prm.frame_size;
    a.cycles = c->cycles;
    a.nsym = c->nsym;
    a.hist_timing = c->prm.timing_mode == QPSK_TIMING_HIST;
    a.fixed_index = c->prm.fixed_index;
    a.sym = sym;
    a.costas = reinterpret_cast<float2 *>(costas);
    a.index = index;
    a.status = c->d_status;
    a.done = count ? c->d_done : nullptr;
    KERNEL_TRY(launch_stream_block(a, c->nstreams, c->stream, inl));
    if (ctab) c->carrier_blocks++;      /* the tables flip only once the launch that fills the next one is in the stream */
    c->last_kernel = "stream_block_kernel";
    return QPSK_OK;
}

static int streams_copy_loop(qpsk_ctx *c, float *d_freq, float *d_phase)
{
    const int n = c->nstreams;
    if (d_phase) HIP_TRY(hipMemcpy2DAsync(d_phase, sizeof(float), c->s_loop, 2 * sizeof(float), sizeof(float), n, hipMemcpyDeviceToDevice, c->stream));
    if (d_freq) HIP_TRY(hipMemcpy2DAsync(d_freq, sizeof(float), c->s_loop + 1, 2 * sizeof(float), sizeof(float), n, hipMemcpyDeviceToDevice, c->stream));
    return QPSK_OK;
}

/* A block of the running streams from the rrc_fir() call on (qpsk.c:125-212), in the context's `filtered` and `index` buffers (stream_run()
 * has sized them).  scanned: stream_scan_kernel has left the filtered block there, planar by decimation phase, and the index, and has
 * updated the delay lines; otherwise d_in is the complex block to filter. */
static int streams_from_filter(qpsk_ctx *c, const float *d_in, bool scanned, uint8_t *d_sym, float *d_freq, float *d_phase,
                               float *d_costas, int32_t *d_index)
{
    const int n = c->nstreams, L = c->prm.frame_size, N = c->nsym;
    float *filt = (float *)c->filtered.p;
    int32_t *idx = (int32_t *)c->index.p;
    if (!scanned) {
        /* qpsk.c:125 */
        KERNEL_TRY(fir_full_rate(c, d_in, c->s_memory, filt, n, L));
        KERNEL_TRY(launch_delay_line(d_in, c->s_memory, n, L, c->stream));
    }
    /* qpsk.c:127-180 (scanned: fixed timing rides on the same kernel -- its scan waves have slack; their index is simply replaced) */
    if (c->prm.timing_mode == QPSK_TIMING_FIXED) {
        KERNEL_TRY(launch_fill_i32(idx, n, c->prm.fixed_index, c->stream));
    } else if (!scanned && c->prm.timing_mode == QPSK_TIMING_HIST) {
        KERNEL_TRY(launch_timing_hist(filt, n, L, c->cycles, idx, nullptr, tuned(c->tune.hist_generic, 0) == 2, c->stream));
    } else if (!scanned) {
        if (int rf = fft_timing_indices(c, d_in, n, idx)) return rf;   /* stateless: it looks at the raw block from sample 2 on */
    }
    /* qpsk.c:196-212 over decimated_frame[0..N) = the PREVIOUS block's picks, which s_dec holds; qpsk.c:186-191:
     * this block's picks replace them for the next call */
    if (int rg = use_context_gains(c)) return rg;
    if (int rc = costas_over_symbols(c, c->s_dec, n, N, N, c->s_loop, d_sym, d_costas, filt, idx, scanned)) return rc;
    if (d_index) HIP_TRY(hipMemcpyAsync(d_index, idx, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    c->last_kernel = scanned ? "stream_scan_kernel + costas_pipe_kernel"
                             : tuned(c->tune.generic, 0) ? "filter, timing, costas_kernel, decimate_kernel" : "filter, timing, costas_pipe_kernel";
    return streams_copy_loop(c, d_freq, d_phase);
}

/* Executes a route.  d_pcm / d_cplx: the block the route was made for, in device memory, exactly one of them */
static int stream_run(qpsk_ctx *c, const StreamRoute &rt, const int16_t *d_pcm, const float *d_cplx, uint8_t *d_sym, float *d_freq,
                      float *d_phase, float *d_costas, int32_t *d_index)
{
    const int n = c->nstreams, L = c->prm.frame_size;
    if (rt.mixer) {
        if (int rc = ensure(c, c->mixed, sizeof(float) * 2 * (size_t)n * L)) return rc;
        /* qpsk.c:114-120 */
        if (int rb = carrier_to_streams(c)) return rb;
        KERNEL_TRY(launch_mixer(d_pcm, (float *)c->mixed.p, c->s_mixer, n, L, c->stream));
        d_pcm = nullptr;
        d_cplx = (const float *)c->mixed.p;
    }
    if (rt.kind == SK_BLOCK) {
        if (int rb = streams_block_launch(c, rt, d_pcm, d_cplx, nullptr, nullptr, d_sym, d_costas, d_index)) return rb;
        return streams_copy_loop(c, d_freq, d_phase);
    }
    if (int rc = ensure(c, c->filtered, sizeof(float) * 2 * (size_t)n * L)) return rc;
    if (int rc = ensure(c, c->index, sizeof(int32_t) * (size_t)n)) return rc;
    if (rt.kind == SK_SCAN) {
        const float *ctab = nullptr;
        float *ctab_next = nullptr;
        if (d_pcm)
            if (int rb = stream_carrier(c, rt.carrier, &ctab, &ctab_next)) return rb;
        KERNEL_TRY(launch_stream_scan(d_pcm, d_cplx, c->s_mixer, c->s_memory, (float *)c->filtered.p, c->d_taps, (int32_t *)c->index.p, n, L,
                                      c->d_status, c->stream, ctab, ctab_next, c->s_cstate, ctab ? c->carrier_scans : 0u, c->cycles));
        if (ctab) {      /* the bookkeeping describes launches that ARE in the stream: the tables flip, the relay's turn advances, the rest of the
                          * next table is owed (a failure between here and the launch that pays it poisons the streams: stream_call_done) */
            c->carrier_blocks++;
            c->carrier_scans++;
            c->carrier_pending = ctab_next;
        }
    }
    const int rc = streams_from_filter(c, d_cplx, rt.kind == SK_SCAN, d_sym, d_freq, d_phase, d_costas, d_index);
    if (c->carrier_pending) {      /* the loop kernel was never reached: the table is finished all the same */
        float *tab = c->carrier_pending;
        c->carrier_pending = nullptr;
        KERNEL_TRY(launch_carrier_table(c->s_cstate, tab, L, true, c->stream));
    }
    return rc;
}

int qpsk_streams_rx_cplx(qpsk_ctx *c, const float *d_in, uint8_t *d_sym, float *d_freq, float *d_phase,
                         float *d_costas, int32_t *d_index)
{
    if (!c || !d_in) return fail(QPSK_ERR_ARG, "qpsk_streams_rx_cplx: null argument");
    if (int ru = streams_usable(c, "qpsk_streams_rx_cplx")) return ru;
    if (bind(c)) return QPSK_ERR_HIP;
    StreamRoute rt;
    stream_route(c, false, d_in, d_sym != nullptr, &rt);
    return stream_call_done(c, stream_run(c, rt, nullptr, d_in, d_sym, d_freq, d_phase, d_costas, d_index));
}

int qpsk_streams_rx_pcm(qpsk_ctx *c, const int16_t *d_pcm, uint8_t *d_sym, float *d_freq, float *d_phase,
                        float *d_costas, int32_t *d_index)
{
    if (!c || !d_pcm) return fail(QPSK_ERR_ARG, "qpsk_streams_rx_pcm: null argument");
    if (int ru = streams_usable(c, "qpsk_streams_rx_pcm")) return ru;
    if (bind(c)) return QPSK_ERR_HIP;
    StreamRoute rt;
    stream_route(c, true, d_pcm, d_sym != nullptr, &rt);
    return stream_call_done(c, stream_run(c, rt, d_pcm, nullptr, d_sym, d_freq, d_phase, d_costas, d_index));
}

static inline void cpu_relax(void)
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#endif
}

/*
 * One block per stream with HOST buffers on both sides -- the call pattern of the reference's main loop
 * (qpsk.c:344-354: fread 512 int16, rx_frame()).  Everything a block needs goes up in ONE pinned copy (PCM, the
 * streams' loop state, the loop gains when they changed), everything it produces comes down in ONE (symbols,
 * costas_frame[], loop state, timing index), and the stream is synchronised ONCE, at the end; the per-call pieces
 * qpsk_dev_upload / qpsk_streams_rx_pcm / qpsk_streams_get_loop_state / qpsk_dev_download synchronise eight times
 * for the same work.
 *   h_pcm [nstreams][frame_size] int16          h_loop_io [nstreams][2] (phase, freq) in and out, may be NULL (carried state)
 *   h_sym [nstreams][nsym] uint8                h_costas [nstreams][nsym][2] float, may be NULL
 *   h_index [nstreams] int32, may be NULL
 */
static int streams_rx_pcm_host_impl(qpsk_ctx *c, const int16_t *h_pcm, float *h_loop_io, uint8_t *h_sym, float *h_costas, int32_t *h_index)
{
    const size_t n = (size_t)c->nstreams, L = (size_t)c->prm.frame_size, N = (size_t)c->nsym;
    /* arena layout, every part 16-byte aligned: in = [loop 8n | pcm 2nL], out = [sym nN | costas 8nN | loop 8n | index 4n] */
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_loop = 0, o_pcm = al(8 * n), in_bytes = o_pcm + al(2 * n * L);
    const size_t o_sym = in_bytes, o_cos = o_sym + al(n * N), o_lout = o_cos + al(8 * n * N), o_idx = o_lout + al(8 * n),
                 total = o_idx + al(4 * n);
    if (c->stage_cap < total) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->h_stage) hipHostFree(c->h_stage);
        hipFree(c->d_stage);
        c->h_stage = c->d_stage = nullptr;
        c->stage_cap = 0;
        if (hipHostMalloc((void **)&c->h_stage, total, hipHostMallocDefault) != hipSuccess ||
            hipMalloc((void **)&c->d_stage, total) != hipSuccess)
            return fail(QPSK_ERR_ALLOC, "staging buffers of %zu bytes", total);
        c->stage_cap = total;
    }
    if (h_loop_io) memcpy(c->h_stage + o_loop, h_loop_io, 8 * n);
    memcpy(c->h_stage + o_pcm, h_pcm, 2 * n * L);
    /* the route of the block where the kernels apart would read it, in the device arena (16-byte aligned, symbols always wanted) */
    StreamRoute rt;
    stream_route(c, true, c->d_stage + o_pcm, true, &rt);
    bool polled = false;
    if (rt.kind == SK_BLOCK && !rt.mixer) {
        /* one launch, no copy engine: the kernel reads the PCM (and the loop state) from the pinned staging buffer and leaves its
         * results there -- a kilobyte in, a few hundred bytes out per stream */
        unsigned char *m = nullptr;
        HIP_TRY(hipHostGetDevicePointer((void **)&m, c->h_stage, 0));
        /* a block of up to 2 KB rides in the kernel arguments (device memory the host writes into): the kernel then reads no host
         * memory at all -- a read of pinned host memory from the GPU costs 8-14 us on this pool, a posted write a fraction of that */
        /* few streams: the waves count themselves off in pinned memory (a system-scope atomic each: ~1 us apiece over PCIe, so only
         * for a handful -- 64 streams took 156 us that way against 47 with the stream's own completion signal) */
        polled = tuned(c->tune.stream_poll, n <= (size_t)StreamBlockInline::MAX_STREAMS ? 1 : 0) != 0;
        StreamBlockInline inl;
        const bool use_inl = n <= (size_t)StreamBlockInline::MAX_STREAMS && n * L <= (size_t)StreamBlockInline::MAX_SAMPLES;
        if (use_inl) {
            if (h_loop_io) memcpy(inl.loop, h_loop_io, 8 * n);
            memcpy(inl.pcm, h_pcm, 2 * n * L);
        }
        if (int rb = streams_block_launch(c, rt, (const int16_t *)(m + o_pcm), nullptr, h_loop_io ? (const float *)(m + o_loop) : nullptr,
                                          (float *)(m + o_lout), m + o_sym, h_costas ? (float *)(m + o_cos) : nullptr, (int32_t *)(m + o_idx),
                                          use_inl ? &inl : nullptr, polled))
            return rb;
        if (polled) {
            /* the kernel's two waves per stream count themselves off in pinned memory behind their last store: watching that word
             * is quicker than the stream's completion signal.  Bounded by the WALL CLOCK (2 s, looked at every 4096 spins): then the
             * ordinary synchronisation takes over, and a counter that is still short after THAT is an error -- the kernel did not run to
             * its end, its results are not in the staging buffer -- with the expectation put back in step with the counter. */
            c->done_expect += 2u * (unsigned)n;
            const volatile unsigned *dn = c->h_done;
            struct timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            for (unsigned spins = 0; (int)(*dn - c->done_expect) < 0; ) {
                cpu_relax();
                if ((++spins & 4095u) == 0) {
                    clock_gettime(CLOCK_MONOTONIC, &t1);
                    if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > 2.0) break;
                }
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            if ((int)(*dn - c->done_expect) < 0) {
                HIP_TRY(hipStreamSynchronize(c->stream));
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                if ((int)(*dn - c->done_expect) < 0) {
                    const unsigned have = *dn, want = c->done_expect;
                    c->done_expect = have;
                    (void)check_status(c);      /* take the kernel's own word, if it left one, out of the status word */
                    return fail(QPSK_ERR_HIP, "stream_block_kernel: %u of %u waves reported completion; the block's results are invalid",
                                2u * (unsigned)n - (want - have), 2u * (unsigned)n);
                }
            }
        }
    } else {
        const size_t up0 = h_loop_io ? o_loop : o_pcm;
        HIP_TRY(hipMemcpyAsync(c->d_stage + up0, c->h_stage + up0, in_bytes - up0, hipMemcpyHostToDevice, c->stream));
        if (h_loop_io) HIP_TRY(hipMemcpyAsync(c->s_loop, c->d_stage + o_loop, 8 * n, hipMemcpyDeviceToDevice, c->stream));
        if (int rc = stream_run(c, rt, (const int16_t *)(c->d_stage + o_pcm), nullptr, c->d_stage + o_sym, nullptr, nullptr,
                                h_costas ? (float *)(c->d_stage + o_cos) : nullptr, (int32_t *)(c->d_stage + o_idx)))
            return rc;
        HIP_TRY(hipMemcpyAsync(c->d_stage + o_lout, c->s_loop, 8 * n, hipMemcpyDeviceToDevice, c->stream));
        /* one copy down: from the symbols to the index (costas_frame[] in between travels even when it is not wanted
         * only if it was computed: without it the two parts around it go separately) */
        if (h_costas) {
            HIP_TRY(hipMemcpyAsync(c->h_stage + o_sym, c->d_stage + o_sym, total - o_sym, hipMemcpyDeviceToHost, c->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(c->h_stage + o_sym, c->d_stage + o_sym, al(n * N), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(c->h_stage + o_lout, c->d_stage + o_lout, total - o_lout, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (!polled) HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c)) return st;
    memcpy(h_sym, c->h_stage + o_sym, n * N);
    if (h_costas) memcpy(h_costas, c->h_stage + o_cos, 8 * n * N);
    if (h_loop_io) memcpy(h_loop_io, c->h_stage + o_lout, 8 * n);
    if (h_index) memcpy(h_index, c->h_stage + o_idx, 4 * n);
    return QPSK_OK;
}

int qpsk_streams_rx_pcm_host(qpsk_ctx *c, const int16_t *h_pcm, float *h_loop_io, uint8_t *h_sym, float *h_costas, int32_t *h_index)
{
    if (!c || !h_pcm || !h_sym) return fail(QPSK_ERR_ARG, "qpsk_streams_rx_pcm_host: null argument");
    if (int ru = streams_usable(c, "qpsk_streams_rx_pcm_host")) return ru;
    if (bind(c)) return QPSK_ERR_HIP;
    return stream_call_done(c, streams_rx_pcm_host_impl(c, h_pcm, h_loop_io, h_sym, h_costas, h_index));
}

/* ------------------------------------------------------------ transmit side (N2) */
int qpsk_tx_reset(qpsk_ctx *c, int nstreams, double tx_hz)
{
    if (!c || nstreams <= 0) return fail(QPSK_ERR_ARG, "qpsk_tx_reset: bad argument");
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)nstreams;
    const size_t hist_bytes = (size_t)tx_history_symbols() * n;
    if (nstreams != c->ntx) {
        hipFree(c->t_hist); hipFree(c->t_mixer);
        c->t_hist = nullptr;
        c->t_mixer = nullptr;
        c->ntx = 0;
        if (hipMalloc((void **)&c->t_hist, hist_bytes) != hipSuccess ||
            hipMalloc((void **)&c->t_mixer, sizeof(float) * 4 * n) != hipSuccess)
            return fail(QPSK_ERR_ALLOC, "hipMalloc of transmitter state failed");
        c->ntx = nstreams;
    }
    /* memset(tx_filter, 0, ...): no symbol sent yet (code 4), i.e. a delay line of zeros */
    HIP_TRY(hipMemsetAsync(c->t_hist, 4, hist_bytes, c->stream));
    /* fbb_tx_phase = cmplx(0.0f); fbb_tx_rect = cmplx(TAU * hz / FS)  (qpsk.c:316,320) */
    float rect[2];
    qpsk_host_rect_tx(tx_hz, c->prm.fs, rect);
    std::vector<float> m(4 * n);
    for (size_t i = 0; i < n; i++) { m[4 * i] = 1.0f; m[4 * i + 1] = 0.0f; m[4 * i + 2] = rect[0]; m[4 * i + 3] = rect[1]; }
    HIP_TRY(hipMemcpyAsync(c->t_mixer, m.data(), sizeof(float) * m.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QPSK_OK;
}

int qpsk_tx_symbols(qpsk_ctx *c, const uint8_t *d_symbols, int nsym, int16_t *d_pcm, float *d_baseband)
{
    if (!c || !d_symbols || (!d_pcm && !d_baseband)) return fail(QPSK_ERR_ARG, "qpsk_tx_symbols: null argument");
    if (c->ntx <= 0) return fail(QPSK_ERR_STATE, "call qpsk_tx_reset() first");
    if (nsym <= 0) return fail(QPSK_ERR_ARG, "nsym = %d", nsym);
    if (bind(c)) return QPSK_ERR_HIP;
    const int n = c->ntx, len = nsym * c->cycles;
    const size_t bytes = sizeof(float) * 2 * (size_t)n * len;
    float *shaped = d_baseband;
    if (!shaped) {
        int rc = ensure(c, c->tx_b, bytes);
        if (rc) return rc;
        shaped = (float *)c->tx_b.p;
    }
    /* qpsk.c:273-282 + 232-238 + 243: Gray map, zero-stuffing and rrc_fir(tx_filter, ...) in one kernel;
     * :248-261 up-mix */
    KERNEL_TRY(launch_tx_shape(d_symbols, c->t_hist, c->d_taps, shaped, n, nsym, c->cycles, c->stream));
    if (d_pcm) KERNEL_TRY(launch_tx_upmix(shaped, d_pcm, c->t_mixer, n, len, c->stream));
    return QPSK_OK;
}

/* ------------------------------------------------------------ bit stages */
int qpsk_crc16_batch(qpsk_ctx *c, const uint8_t *d_data, int npackets, int nbytes, uint16_t *d_crc)
{
    if (!c || !d_data || !d_crc) return fail(QPSK_ERR_ARG, "qpsk_crc16_batch: null argument");
    if (npackets <= 0 || nbytes < 0) return fail(QPSK_ERR_ARG, "npackets %d nbytes %d", npackets, nbytes);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_crc16(d_data, npackets, nbytes, d_crc, c->stream));
    return QPSK_OK;
}

int qpsk_interleave_batch(qpsk_ctx *c, uint8_t *d_data, int npackets, int nbytes, int dir)
{
    if (!c || !d_data) return fail(QPSK_ERR_ARG, "qpsk_interleave_batch: null argument");
    if (npackets <= 0 || nbytes <= 0 || nbytes * 8 >= 65536 || (dir != 0 && dir != 1))
        return fail(QPSK_ERR_ARG, "npackets %d, nbytes %d (1..8191), dir %d (0|1)", npackets, nbytes, dir);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_interleave(d_data, npackets, nbytes, qpsk_host_interleave_prime((unsigned)nbytes * 8u), dir, c->stream));
    return QPSK_OK;
}

int qpsk_scramble_batch(qpsk_ctx *c, uint8_t *d_sym, int npackets, int nsym)
{
    if (!c || !d_sym) return fail(QPSK_ERR_ARG, "qpsk_scramble_batch: null argument");
    if (npackets <= 0 || nsym <= 0) return fail(QPSK_ERR_ARG, "npackets %d nsym %d", npackets, nsym);
    if (bind(c)) return QPSK_ERR_HIP;
    int rc = ensure(c, c->keystream, (size_t)nsym);
    if (rc) return rc;
    if (c->keystream_len != nsym) {
        std::vector<unsigned char> ks((size_t)nsym);
        qpsk_host_scramble_keystream(ks.data(), nsym);
        HIP_TRY(hipMemcpy(c->keystream.p, ks.data(), (size_t)nsym, hipMemcpyHostToDevice));
        c->keystream_len = nsym;
    }
    KERNEL_TRY(launch_scramble(d_sym, (const uint8_t *)c->keystream.p, npackets, nsym, c->stream));
    return QPSK_OK;
}

/* ---------------------------------------------------------------- deframer */
static const int DF_ADV_OFFSET = 1040;      /* the tables: keystream bytes [0, nbytes + 2), then 64 uint16 */

/* r x^(8 k) mod the CRC-16 polynomial: k zero bytes through crc16()'s register, starting from r */
static uint16_t crc_shift(unsigned r, int k)
{
    for (int i = 0; i < 8 * k; i++) r = ((r << 1) ^ ((r & 0x8000u) ? 0x1021u : 0u)) & 0xFFFFu;
    return (uint16_t)r;
}
/* x^(8 k) */
static uint16_t crc_advance(int k) { return crc_shift(1u, k); }

static const int DFC_ADV_OFFSET = (DEFRAME_CODED_MAX_STEPS + 15) & ~15;      /* the coded mode's tables: keystream dibits [nsteps], then nbytes uint16 */

/* all four resets: who = the entry point's name; coded: the body is the coded dibits of 8 (nbytes + 2) + 6 trellis steps, held as int8 pairs, in the
 * layout of what the entry point takes.  The pattern is checked first, as the entry points always have; the stride behind everything else */
static int deframer_reset_impl(qpsk_ctx *c, const char *who, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes,
                               int max_packets, bool coded, int mode, float scale, const Pattern *pattern = nullptr, const int *stride = nullptr)
{
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context or sync word", who);
    CodedLayout l;
    if (int rc = layout_add_pattern(who, pattern, &l)) return rc;
    if (!h_sync) return fail(QPSK_ERR_ARG, "%s: null context or sync word", who);
    if (nstreams <= 0) return fail(QPSK_ERR_ARG, "%s: nstreams = %d", who, nstreams);
    if (nsync < 1 || nsync > SYNC_MAX_WORD) return fail(QPSK_ERR_ARG, "%s: nsync = %d outside 1..%d", who, nsync, SYNC_MAX_WORD);
    if (min_score < 1 || min_score > nsync) return fail(QPSK_ERR_ARG, "%s: min_score = %d outside 1..%d", who, min_score, nsync);
    if (nbytes < 1 || nbytes > DEFRAME_MAX_BYTES) return fail(QPSK_ERR_ARG, "%s: nbytes = %d outside 1..%d", who, nbytes, DEFRAME_MAX_BYTES);
    if (max_packets < 1 || max_packets > DEFRAME_MAX_PACKETS)
        return fail(QPSK_ERR_ARG, "%s: max_packets = %d outside 1..%d", who, max_packets, DEFRAME_MAX_PACKETS);
    for (int i = 0; i < nsync; i++)
        if (h_sync[i] > 3) return fail(QPSK_ERR_ARG, "%s: sync[%d] = %d is not a dibit", who, i, (int)h_sync[i]);
    if (coded && mode != QPSK_SOFT_UNIT && mode != QPSK_SOFT_LLR) return fail(QPSK_ERR_ARG, "%s: unknown mode %d", who, mode);
    if (coded && !(scale > 0.0f && scale <= 3.402823466e+38f)) return fail(QPSK_ERR_ARG, "%s: scale = %g is not finite and > 0", who, (double)scale);
    const int nb = nbytes + 2, nsteps = 8 * nb + 6;
    /* dibits of a body: a punctured one is shorter than 8 nb + 6, so the pending buffer and the keystream table's bound hold as they are.
     * K >= 1 sent bit per period and nsteps > 32 >= period: at least one dibit */
    const int N = coded ? (int)coded_ndibits(l, nsteps) : 4 * nb;
    if (int rc = layout_add_stride(who, nsteps, stride, &l)) return rc;      /* a bad stride resets nothing */
    if (bind(c)) return QPSK_ERR_HIP;
    /* refused until this call has completed */
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_deframer(c);
    const size_t state_stride = (size_t)DEFRAME_PEND_OFFSET + (((size_t)N * (coded ? 2 : 1) + 15) & ~(size_t)15);
    const size_t tab_bytes = coded ? (size_t)DFC_ADV_OFFSET + 2 * (size_t)DEFRAME_MAX_BYTES : (size_t)DF_ADV_OFFSET + 128;
    if (hipMalloc(&c->df_state, state_stride * (size_t)nstreams) != hipSuccess || hipMalloc(&c->df_tables, tab_bytes) != hipSuccess) {
        free_deframer(c);
        (void)hipGetLastError();
        return fail(QPSK_ERR_ALLOC, "%s: %d streams of %zu bytes of state", who, nstreams, state_stride);
    }
    std::vector<unsigned char> ks((size_t)N);
    qpsk_host_scramble_keystream(ks.data(), N);
    std::vector<uint8_t> tab(tab_bytes, 0);
    if (coded) {
        memcpy(tab.data(), ks.data(), (size_t)N);
        uint16_t adv = 1;                                               /* x^(8 m), m = 0 .. nbytes - 1, a byte at a time */
        for (int m = 0; m < nbytes; m++, adv = crc_shift(adv, 1)) memcpy(&tab[DFC_ADV_OFFSET + 2 * m], &adv, 2);
        c->df_crc_init = crc_shift(0xFFFFu, nbytes);
    } else {
        for (int k = 0; k < nb; k++) tab[k] = (uint8_t)(ks[4 * k] | ks[4 * k + 1] << 2 | ks[4 * k + 2] << 4 | ks[4 * k + 3] << 6);
        const int per = (nb + 63) / 64;
        for (int l = 0; l < 64; l++) {
            const int end = (l + 1) * per < nbytes ? (l + 1) * per : nbytes;
            const uint16_t v = crc_advance(nbytes - end);
            memcpy(&tab[DF_ADV_OFFSET + 2 * l], &v, 2);
        }
    }
    c->df_sync_lo[0] = c->df_sync_lo[1] = c->df_sync_hi[0] = c->df_sync_hi[1] = 0;
    for (int i = 0; i < nsync; i++) {
        const unsigned r = h_sync[i] ^ (h_sync[i] >> 1);
        if (r & 1u) c->df_sync_lo[i >> 6] |= 1ull << (i & 63);
        if (r & 2u) c->df_sync_hi[i >> 6] |= 1ull << (i & 63);
    }
    HIP_TRY(hipMemsetAsync(c->df_state, 0, state_stride * (size_t)nstreams, c->stream));
    HIP_TRY(hipMemcpyAsync(c->df_tables, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->df_stride = state_stride;
    c->df_nstreams = nstreams;
    c->df_nsync = nsync;
    c->df_min_score = min_score;
    c->df_nbytes = nbytes;
    c->df_max_packets = max_packets;
    c->df_coded = coded;
    c->df_mode = mode;
    c->df_scale = scale;
    c->df_nsteps = coded ? nsteps : 0;
    c->df_nbody = coded ? N : 0;
    c->df_layout = l;
    c->df_ready = true;
    return QPSK_OK;
}

int qpsk_deframer_reset(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets)
{
    return deframer_reset_impl(c, "qpsk_deframer_reset", nstreams, h_sync, nsync, min_score, nbytes, max_packets, false, 0, 1.0f);
}

int qpsk_deframer_reset_coded(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets,
                              int mode, float scale)
{
    return deframer_reset_impl(c, "qpsk_deframer_reset_coded", nstreams, h_sync, nsync, min_score, nbytes, max_packets, true, mode, scale);
}

/* the coded mode behind a puncturing pattern: the body is the ntx(8 (nbytes + 2) + 6) transmitted dibits; the pattern lives in the
 * deframer's state, and qpsk_deframer_push_coded decodes with the punctured kernels */
int qpsk_deframer_reset_coded_punct(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets,
                                    int mode, float scale, int period, uint32_t keep0, uint32_t keep1)
{
    const Pattern pattern = {period, keep0, keep1};
    return deframer_reset_impl(c, "qpsk_deframer_reset_coded_punct", nstreams, h_sync, nsync, min_score, nbytes, max_packets, true, mode, scale, &pattern);
}

/* the same behind a stride of INTERLEAVING as well: the body is as long, its bits lie at pi(k) on air, and qpsk_deframer_push_coded decodes
 * with the interleaved kernels */
int qpsk_deframer_reset_coded_ilv(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets,
                                  int mode, float scale, int period, uint32_t keep0, uint32_t keep1, int stride)
{
    const Pattern pattern = {period, keep0, keep1};
    return deframer_reset_impl(c, "qpsk_deframer_reset_coded_ilv", nstreams, h_sync, nsync, min_score, nbytes, max_packets, true, mode, scale,
                               &pattern, &stride);
}

/* what both pushes do behind their own argument checks (who = the entry point's name): the state checks, no output (the caller's
 * list; NULL entries are skipped) may overlap the input of sym_bytes a symbol, the device, and the hunt's arguments from the context */
struct DeframeOutput { const void *p; size_t bytes; const char *name; };
static int deframer_push_begin(qpsk_ctx *c, const char *who, bool coded, const void *in, size_t sym_bytes, int nsym,
                               std::initializer_list<DeframeOutput> outs, DeframeHuntArgs &a)
{
    if (!c->df_state) return fail(QPSK_ERR_STATE, "%s: no %s yet", who, coded ? "qpsk_deframer_reset_coded" : "qpsk_deframer_reset");
    if (c->df_coded != coded)
        return fail(QPSK_ERR_STATE, "%s: the deframer was reset in %s mode (%s)", who, coded ? "uncoded" : "coded",
                    coded ? "qpsk_deframer_push" : "qpsk_deframer_push_coded");
    if (!c->df_ready) return fail(QPSK_ERR_STATE, "%s: the deframer's state is undefined after a failed push; reset it", who);
    const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (size_t)c->df_nstreams * (size_t)nsym * sym_bytes;
    for (const auto &o : outs) {
        if (!o.p) continue;
        const uintptr_t o0 = (uintptr_t)o.p, o1 = o0 + o.bytes;
        if (o0 < i1 && i0 < o1) return fail(QPSK_ERR_ARG, "%s: %s overlaps the input", who, o.name);
    }
    if (bind(c)) return QPSK_ERR_HIP;
    a.nstreams = c->df_nstreams;
    a.nsym = nsym;
    a.nsync = c->df_nsync;
    a.min_score = c->df_min_score;
    a.state = c->df_state;
    a.state_stride = c->df_stride;
    for (int i = 0; i < 2; i++) { a.sync_lo[i] = c->df_sync_lo[i]; a.sync_hi[i] = c->df_sync_hi[i]; }
    return QPSK_OK;
}

int qpsk_deframer_push(qpsk_ctx *c, const float *d_costas, const uint8_t *d_data, int nsym, int32_t *d_count, uint8_t *d_bytes,
                       long long *d_pos, int32_t *d_rot, int32_t *d_score, uint8_t *d_crc_ok)
{
    if (!c) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: null context");
    if ((d_costas != nullptr) == (d_data != nullptr)) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: give exactly one of d_costas, d_data");
    if (!d_count) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: d_count is required");
    if (nsym < 1 || nsym > DEFRAME_MAX_NSYM) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: nsym = %d outside 1..%d", nsym, DEFRAME_MAX_NSYM);
    const size_t S = (size_t)c->df_nstreams, M = (size_t)c->df_max_packets;
    DeframeArgs a{};
    if (int rc = deframer_push_begin(c, "qpsk_deframer_push", false, d_costas ? (const void *)d_costas : (const void *)d_data,
                                     d_costas ? 2 * sizeof(float) : 1, nsym,
                                     {{d_count, S * 4, "d_count"}, {d_bytes, S * M * (size_t)(c->df_nbytes + 2), "d_bytes"}, {d_pos, S * M * 8, "d_pos"},
                                      {d_rot, S * M * 4, "d_rot"}, {d_score, S * M * 4, "d_score"}, {d_crc_ok, S * M, "d_crc_ok"}}, a))
        return rc;
    a.data = d_data;
    a.costas = reinterpret_cast<const float2 *>(d_costas);
    a.nbytes = c->df_nbytes;
    a.max_packets = c->df_max_packets;
    a.bytes_per_lane = (c->df_nbytes + 2 + 63) / 64;
    a.keystream = c->df_tables;
    a.crc_adv = reinterpret_cast<const uint16_t *>(c->df_tables + DF_ADV_OFFSET);
    a.count = d_count;
    a.bytes = d_bytes;
    a.pos = d_pos;
    a.rot = d_rot;
    a.score = d_score;
    a.crc_ok = d_crc_ok;
    (void)hipGetLastError();
    const int e = launch_deframe(a, c->stream);
    if (e != 0) {
        c->df_ready = false;
        return fail(QPSK_ERR_HIP, "deframe_kernel launch: %s", hipGetErrorString((hipError_t)e));
    }
    c->last_kernel = "deframe_kernel";
    return QPSK_OK;
}

/* the coded mode's push (deframe_coded.hip): [the row's gain, unless the caller gives one] -> hunt + soft rows -> decode.  Everything that can
 * fail without a launch -- arguments, the three buffers -- comes before the first launch */
int qpsk_deframer_push_coded(qpsk_ctx *c, const float *d_costas, int nsym, const float *d_gain, int32_t *d_count, uint8_t *d_bytes,
                             long long *d_pos, int32_t *d_rot, int32_t *d_score, uint8_t *d_crc_ok, int32_t *d_info)
{
    if (!c) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: null context");
    c->viterbi_launches = 0;      /* a refused call made none */
    if (!d_costas) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: d_costas is required");
    if (!d_count) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: d_count is required");
    if (nsym < 1 || nsym > DEFRAME_MAX_NSYM) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: nsym = %d outside 1..%d", nsym, DEFRAME_MAX_NSYM);
    if ((uintptr_t)d_costas % 8) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: d_costas is not 8-byte aligned");
    if ((uintptr_t)d_gain % 4 || (uintptr_t)d_count % 4 || (uintptr_t)d_rot % 4 || (uintptr_t)d_score % 4 || (uintptr_t)d_info % 4 || (uintptr_t)d_pos % 8)
        return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: a misaligned array");
    const size_t S = (size_t)c->df_nstreams, M = (size_t)c->df_max_packets;
    DeframeCodedArgs a{};
    if (int rc = deframer_push_begin(c, "qpsk_deframer_push_coded", true, d_costas, 2 * sizeof(float), nsym,
                                     {{d_count, S * 4, "d_count"}, {d_bytes, S * M * (size_t)(c->df_nbytes + 2), "d_bytes"}, {d_pos, S * M * 8, "d_pos"},
                                      {d_rot, S * M * 4, "d_rot"}, {d_score, S * M * 4, "d_score"}, {d_crc_ok, S * M, "d_crc_ok"},
                                      {d_info, S * M * 16, "d_info"}}, a))
        return rc;
    const int Nc = c->df_nbody, pitch = (Nc + 1) & ~1;      /* the staging rows go by what is on air, the decision words by the steps */
    const int per = std::min<long long>(c->df_max_packets, (long long)nsym / (c->df_nsync + Nc) + 1);
    const size_t rows = S * (size_t)per;
    const bool decode = d_bytes || d_crc_ok || d_info;
    const ViterbiRoute route = viterbi_route(c, rows, c->df_nsteps);
    if (int rg = ensure(c, c->dfstage, rows * 2 * (size_t)pitch)) return rg;
    if (!d_gain)
        if (int rg = ensure(c, c->softgain, sizeof(float) * S)) return rg;
    if (decode && !route.lds)
        if (int rg = ensure(c, c->vitdec, route.chunk_rows * route.per_row)) return rg;

    a.costas = reinterpret_cast<const float2 *>(d_costas);
    a.gain = d_gain ? d_gain : (const float *)c->softgain.p;
    a.check_gain = d_gain != nullptr;
    a.nbytes = c->df_nbytes;
    a.max_packets = c->df_max_packets;
    a.nsteps = c->df_nsteps;
    a.per_stream = per;
    a.stage = (int8_t *)c->dfstage.p;
    a.flip = c->df_tables;
    a.crc_adv = reinterpret_cast<const uint16_t *>(c->df_tables + DFC_ADV_OFFSET);
    a.crc_init = c->df_crc_init;
    a.count = d_count;
    a.bytes = d_bytes;
    a.pos = d_pos;
    a.rot = d_rot;
    a.score = d_score;
    a.crc_ok = d_crc_ok;
    a.info = d_info;
    a.status = c->d_status;
    (void)hipGetLastError();
    if (!d_gain)      /* nothing of the deframer's has run yet: a failure here leaves its state as it was */
        KERNEL_TRY(launch_soft_sums(d_costas, (size_t)nsym, c->df_nstreams, nsym, 0, c->df_mode, c->df_scale, (float *)c->softgain.p, nullptr, nullptr,
                                    c->d_status, c->stream));
    const DeframeCodedBody body = {Nc, pitch};      /* the decode's launch adds the layout */
    int e = launch_deframe_coded_hunt(a, body, c->stream);
    for (size_t r0 = 0; e == 0 && decode && r0 < rows; r0 += route.chunk_rows) {      /* stream order: a chunk's trace-back is over before the next one's forward pass */
        const int n = (int)std::min<size_t>(route.chunk_rows, rows - r0);
        e = launch_deframe_coded_decode(a, body, c->df_layout, (int)r0, n, route.lds ? nullptr : (unsigned long long *)c->vitdec.p, route.lds, c->stream);
        if (e == 0) c->viterbi_launches++;
    }
    if (e != 0) {
        c->df_ready = false;
        return fail(QPSK_ERR_HIP, "qpsk_deframer_push_coded launch: %s", hipGetErrorString((hipError_t)e));
    }
    static const char *const label[][2] = {
        {"deframe_coded_hunt_kernel + deframe_coded_decode_kernel<global>", "deframe_coded_hunt_kernel + deframe_coded_decode_kernel<lds>"},
        {"deframe_coded_hunt_kernel + deframe_coded_decode_punct_kernel<global>", "deframe_coded_hunt_kernel + deframe_coded_decode_punct_kernel<lds>"},
        {"deframe_coded_hunt_kernel + deframe_coded_decode_ilv_kernel<global>", "deframe_coded_hunt_kernel + deframe_coded_decode_ilv_kernel<lds>"}};
    c->last_kernel = decode ? label[c->df_layout.kind][route.lds] : "deframe_coded_hunt_kernel";
    return QPSK_OK;
}


/* ------------------------------------------------------------------ framer */
/* FRAMER (include/qpsk_hip.h): the dibits of a body on air, B; who = the entry point's name.  The pattern is looked at only when coded */
static int frame_body(const char *who, int nbytes, int coding, const Pattern &pattern, CodedLayout *l, int *nbody)
{
    if (nbytes < 1 || nbytes > FRAME_MAX_BYTES) return fail(QPSK_ERR_ARG, "%s: nbytes = %d outside 1..%d", who, nbytes, FRAME_MAX_BYTES);
    if (coding != QPSK_FRAME_UNCODED && coding != QPSK_FRAME_CODED) return fail(QPSK_ERR_ARG, "%s: unknown coding %d", who, coding);
    if (coding == QPSK_FRAME_UNCODED) {
        *nbody = 4 * (nbytes + 2);
        return QPSK_OK;
    }
    if (int rc = layout_add_pattern(who, &pattern, l)) return rc;
    /* K >= 1 sent bit per period and 8 (nbytes + 2) + 6 > 32 >= period steps: at least one dibit */
    *nbody = (int)coded_ndibits(*l, 8 * (nbytes + 2) + 6);
    return QPSK_OK;
}

int qpsk_frame_len(int nsync, int nbytes, int coding, int period, uint32_t keep0, uint32_t keep1)
{
    if (nsync < 1 || nsync > SYNC_MAX_WORD) return fail(QPSK_ERR_ARG, "qpsk_frame_len: nsync = %d outside 1..%d", nsync, SYNC_MAX_WORD);
    CodedLayout l;
    int nbody = 0;
    if (int rc = frame_body("qpsk_frame_len", nbytes, coding, Pattern{period, keep0, keep1}, &l, &nbody)) return rc;
    return nsync + nbody;
}

/* The framer's keystream table holds at least n dibits.  It grows into a NEW buffer, filled by a blocking copy before anything can read it;
 * the old one is freed only behind a synchronisation of the context's stream, the one stream every launch that reads it was enqueued on
 * (qpsk_ctx_set_stream synchronises the stream it leaves), so no enqueued launch still reads a table that is freed.  A failed allocation
 * leaves the old table, and the context, as they were */
static int frame_keystream(qpsk_ctx *c, int n)
{
    if (c->frame_ks_len >= n) return QPSK_OK;
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(QPSK_ERR_ALLOC, "qpsk_frame_batch: hipMalloc(%d bytes of keystream): %s", n, hipGetErrorString(e));
    }
    std::vector<unsigned char> ks((size_t)n);
    qpsk_host_scramble_keystream(ks.data(), n);
    hipError_t e2 = hipMemcpy(p, ks.data(), (size_t)n, hipMemcpyHostToDevice);
    if (e2 == hipSuccess && c->frame_ks) e2 = hipStreamSynchronize(c->stream);
    if (e2 != hipSuccess) {
        hipFree(p);
        return fail(QPSK_ERR_HIP, "qpsk_frame_batch: keystream upload: %s", hipGetErrorString(e2));
    }
    hipFree(c->frame_ks);
    c->frame_ks = (uint8_t *)p;
    c->frame_ks_len = n;
    return QPSK_OK;
}

/* both framers: who = the entry point's name; stride = NULL for qpsk_frame_batch */
static int frame_impl(qpsk_ctx *c, const char *who, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                      const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, const int *stride, int lead, int gap,
                      int row_len, uint8_t *d_out, uint16_t *d_crc)
{
    if (!c || !d_payload || !h_sync || !d_out) return fail(QPSK_ERR_ARG, "%s: null context, payload, sync word or output", who);
    if (nsync < 1 || nsync > SYNC_MAX_WORD) return fail(QPSK_ERR_ARG, "%s: nsync = %d outside 1..%d", who, nsync, SYNC_MAX_WORD);
    CodedLayout l;      /* coded: behind the pattern; the uncoded format has no layout */
    int nbody = 0;
    if (int rc = frame_body(who, nbytes, coding, Pattern{period, keep0, keep1}, &l, &nbody)) return rc;
    if (nrows < 1 || per_row < 1 || per_row > FRAME_MAX_PER_ROW || (long long)nrows * per_row > INT_MAX)
        return fail(QPSK_ERR_ARG, "%s: nrows = %d, per_row = %d (1..%d, nrows * per_row < 2^31)", who, nrows, per_row, FRAME_MAX_PER_ROW);
    if (payload_pitch != 0 && payload_pitch < nbytes)
        return fail(QPSK_ERR_ARG, "%s: payload_pitch = %lld below nbytes = %d", who, payload_pitch, nbytes);
    if (lead < 0 || gap < 0) return fail(QPSK_ERR_ARG, "%s: lead = %d, gap = %d", who, lead, gap);
    const long long need = (long long)lead + (long long)per_row * (nsync + nbody) + (long long)(per_row - 1) * gap;
    if (row_len < 1 || row_len > FRAME_MAX_ROW || need > row_len)
        return fail(QPSK_ERR_ARG, "%s: lead %d + %d packets of %d dibits + gaps of %d = %lld do not fit row_len = %d (up to %d)", who, lead,
                    per_row, nsync + nbody, gap, need, row_len, FRAME_MAX_ROW);
    const size_t npk = (size_t)nrows * (size_t)per_row, pitch = payload_pitch ? (size_t)payload_pitch : (size_t)nbytes;
    const uintptr_t i0 = (uintptr_t)d_payload, i1 = i0 + (npk - 1) * pitch + (size_t)nbytes;
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)nrows * (size_t)row_len;
    if (o0 < i1 && i0 < o1) return fail(QPSK_ERR_ARG, "%s: d_out overlaps d_payload", who);
    if (d_crc) {
        const uintptr_t r0 = (uintptr_t)d_crc, r1 = r0 + 2 * npk;
        if (((uintptr_t)d_crc & 1) || (r0 < i1 && i0 < r1) || (r0 < o1 && o0 < r1))
            return fail(QPSK_ERR_ARG, "%s: d_crc is not 2-byte aligned, or overlaps d_payload or d_out", who);
    }
    /* the stride: the uncoded format has none; 1 is no interleaving at all and, here alone, takes the kernel of the layer below, frame_kernel<coded> */
    if (stride && coding == QPSK_FRAME_UNCODED && *stride != 1) return fail(QPSK_ERR_ARG, "%s: stride = %d with QPSK_FRAME_UNCODED (1 only)", who, *stride);
    if (stride && coding == QPSK_FRAME_CODED) {
        if (int rc = layout_add_stride(who, 8 * (nbytes + 2) + 6, stride, &l)) return rc;
        if (l.ilv.s == 1) l.kind = CODED_PUNCT;
    }
    if (bind(c)) return QPSK_ERR_HIP;
    if (int rc = frame_keystream(c, row_len > nbody ? row_len : nbody)) return rc;
    FrameArgs a{};
    a.payload = d_payload;
    a.pitch = pitch;
    a.out = d_out;
    a.crc = d_crc;
    a.ks = c->frame_ks;
    a.npackets = (int)npk;
    a.per_row = per_row;
    a.nbytes = nbytes;
    a.nsync = nsync;
    a.nbody = nbody;
    a.lead = lead;
    a.gap = gap;
    a.row_len = row_len;
    a.bytes_per_lane = (nbytes + 63) / 64;
    a.coded = coding == QPSK_FRAME_CODED;
    /* lane l's share of the CRC covers payload bytes [l c, min((l + 1) c, nbytes)): x^(8 k), k = the bytes behind them; then the init value's */
    uint16_t adv[65];
    for (int l = 0; l < 64; l++) {
        const int end = (l + 1) * a.bytes_per_lane < nbytes ? (l + 1) * a.bytes_per_lane : nbytes;
        adv[l] = crc_advance(nbytes - end);
    }
    adv[64] = crc_shift(0xFFFFu, nbytes);
    KERNEL_TRY(launch_frame(a, l, h_sync, adv, c->stream));
    c->last_kernel = !a.coded ? "frame_kernel<uncoded>" : l.kind == CODED_ILV ? "frame_kernel<coded,ilv>" : "frame_kernel<coded>";
    return QPSK_OK;
}

int qpsk_frame_batch(qpsk_ctx *c, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                     const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, int lead, int gap,
                     int row_len, uint8_t *d_out, uint16_t *d_crc)
{
    return frame_impl(c, "qpsk_frame_batch", d_payload, payload_pitch, nrows, per_row, nbytes, h_sync, nsync, coding, period, keep0, keep1, nullptr,
                      lead, gap, row_len, d_out, d_crc);
}

int qpsk_frame_batch_ilv(qpsk_ctx *c, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                         const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, int stride, int lead, int gap,
                         int row_len, uint8_t *d_out, uint16_t *d_crc)
{
    return frame_impl(c, "qpsk_frame_batch_ilv", d_payload, payload_pitch, nrows, per_row, nbytes, h_sync, nsync, coding, period, keep0, keep1,
                      &stride, lead, gap, row_len, d_out, d_crc);
}

/* ------------------------------------------------------------ the Reed-Solomon outer code (REED-SOLOMON in include/qpsk_hip.h) */
int qpsk_rs_generator(int nroots, uint8_t *h_g)
{
    if (!h_g) return fail(QPSK_ERR_ARG, "qpsk_rs_generator: null output");
    if (nroots < 1 || nroots > RS_MAX_ROOTS) return fail(QPSK_ERR_ARG, "qpsk_rs_generator: nroots = %d outside 1..%d", nroots, RS_MAX_ROOTS);
    rs_generator(nroots, h_g);
    return QPSK_OK;
}

/* a pitch argument: 0 = tight, otherwise at least the row and small enough for nrows rows to stay inside 63 bits */
static bool rs_pitch(long long pitch, int row, int nrows, size_t *out)
{
    if (pitch != 0 && (pitch < row || pitch > (LLONG_MAX >> 1) / nrows)) return false;
    *out = pitch ? (size_t)pitch : (size_t)row;
    return true;
}

static bool rs_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

int qpsk_rs_encode_batch(qpsk_ctx *c, const uint8_t *d_data, long long data_pitch, int nrows, int k, int nroots, uint8_t *d_out,
                         long long out_pitch)
{
    if (!c || !d_data || !d_out) return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: null context, data or output");
    if (nrows < 1 || k < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || k + nroots > 255)
        return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: nrows = %d, k = %d, nroots = %d (nrows >= 1, k >= 1, 1 <= nroots <= %d, k + nroots <= 255)",
                    nrows, k, nroots, RS_MAX_ROOTS);
    const int n = k + nroots;
    size_t ip = 0, op = 0;
    if (!rs_pitch(data_pitch, k, nrows, &ip) || !rs_pitch(out_pitch, n, nrows, &op))
        return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: data_pitch = %lld (0 or >= k = %d), out_pitch = %lld (0 or >= n = %d)", data_pitch, k,
                    out_pitch, n);
    const uintptr_t i0 = (uintptr_t)d_data, i1 = i0 + (size_t)(nrows - 1) * ip + (size_t)k;
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)(nrows - 1) * op + (size_t)n;
    if (rs_overlap(i0, i1, o0, o1)) return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: d_out overlaps d_data");
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_rs_encode(d_data, ip, nrows, k, nroots, d_out, op, c->stream));
    c->last_kernel = "rs_encode_kernel";
    return QPSK_OK;
}

int qpsk_rs_decode_batch(qpsk_ctx *c, const uint8_t *d_in, long long in_pitch, int nrows, int n, int nroots, const uint8_t *d_erase,
                         uint8_t *d_out, long long out_pitch, int32_t *d_info)
{
    if (!c || !d_in) return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: null context or input");
    if (!d_out && !d_info) return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_out and d_info are both NULL");
    if (nrows < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || n <= nroots || n > 255)
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: nrows = %d, n = %d, nroots = %d (nrows >= 1, 1 <= nroots <= %d, nroots < n <= 255)", nrows,
                    n, nroots, RS_MAX_ROOTS);
    size_t ip = 0, op = 0;
    if (!rs_pitch(in_pitch, n, nrows, &ip) || !rs_pitch(out_pitch, n, nrows, &op))
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: in_pitch = %lld, out_pitch = %lld (each 0 or >= n = %d)", in_pitch, out_pitch, n);
    const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)(nrows - 1) * ip + (size_t)n;
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)(nrows - 1) * op + (size_t)n;
    const uintptr_t e0 = (uintptr_t)d_erase, e1 = e0 + (size_t)nrows * (size_t)n;
    const uintptr_t f0 = (uintptr_t)d_info, f1 = f0 + 16 * (size_t)nrows;
    /* in place: exactly the input rows, each wave reads its whole row before it writes it */
    if (d_out && !(d_out == d_in && op == ip) && rs_overlap(i0, i1, o0, o1))
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_out overlaps d_in (allowed: d_out == d_in with the same pitch)");
    if (d_out && d_erase && rs_overlap(e0, e1, o0, o1)) return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_out overlaps d_erase");
    if (d_info && (((uintptr_t)d_info & 3) || rs_overlap(f0, f1, i0, i1) || (d_out && rs_overlap(f0, f1, o0, o1)) ||
                   (d_erase && rs_overlap(f0, f1, e0, e1))))
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_info is not 4-byte aligned, or overlaps d_in, d_out or d_erase");
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_rs_decode(d_in, ip, nrows, n, nroots, d_erase, d_out, op, d_info, c->stream));
    c->last_kernel = "rs_decode_kernel";
    return QPSK_OK;
}

/* test hook (tests/test_viterbi_chunks_gpu.py): host bookkeeping only */
int qpsk_test_viterbi_launches(qpsk_ctx *c, int *out)
{
    if (!c || !out) return fail(QPSK_ERR_ARG, "qpsk_test_viterbi_launches: null argument");
    *out = c->viterbi_launches;
    return QPSK_OK;
}

/* test hook (tests/test_deframe_positions_gpu.py): the stream positions of both deframers move on by delta, as if delta more dibits had
 * been pushed whose words and packets all lay behind the carried tail.  Plain copies of the headers, no kernel */
int qpsk_test_deframer_advance(qpsk_ctx *c, long long delta)
{
    if (!c) return fail(QPSK_ERR_ARG, "qpsk_test_deframer_advance: null context");
    if (delta < 0 || delta > (1LL << 62)) return fail(QPSK_ERR_ARG, "qpsk_test_deframer_advance: delta = %lld outside 0..2^62", delta);
    if (!c->df_state) return fail(QPSK_ERR_STATE, "qpsk_test_deframer_advance: no deframer reset yet");
    if (!c->df_ready) return fail(QPSK_ERR_STATE, "qpsk_test_deframer_advance: the deframer's state is undefined after a failed push; reset it");
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t S = (size_t)c->df_nstreams;
    std::vector<DeframeHeader> hd(S);
    HIP_TRY(hipMemcpy2D(hd.data(), sizeof(DeframeHeader), c->df_state, c->df_stride, sizeof(DeframeHeader), S, hipMemcpyDeviceToHost));
    for (const auto &h : hd) {
        if (h.len < (long long)c->df_nsync - 1)      /* the hunt takes a tail of nsync - 1 dibits for granted once len says so */
            return fail(QPSK_ERR_STATE, "qpsk_test_deframer_advance: a stream has seen %lld dibits, fewer than nsync - 1 = %d", h.len, c->df_nsync - 1);
        if (h.len > LLONG_MAX - delta - (1LL << 32))
            return fail(QPSK_ERR_ARG, "qpsk_test_deframer_advance: the positions would leave 64 bits");
    }
    for (auto &h : hd) { h.len += delta; h.h += delta; h.ppos += delta; }
    HIP_TRY(hipMemcpy2D(c->df_state, c->df_stride, hd.data(), sizeof(DeframeHeader), sizeof(DeframeHeader), S, hipMemcpyHostToDevice));
    return QPSK_OK;
}

/* ---------------------------------------------------------------- memory */
int qpsk_dev_alloc(qpsk_ctx *c, void **d_ptr, size_t bytes)
{
    if (!c || !d_ptr) return fail(QPSK_ERR_ARG, "null argument");
    if (bind(c)) return QPSK_ERR_HIP;
    hipError_t e = hipMalloc(d_ptr, bytes);
    if (e != hipSuccess) return fail(QPSK_ERR_ALLOC, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return QPSK_OK;
}

int qpsk_dev_free(qpsk_ctx *c, void *d_ptr)
{
    if (!c) return fail(QPSK_ERR_ARG, "null argument");
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(d_ptr));
    return QPSK_OK;
}

int qpsk_dev_upload(qpsk_ctx *c, void *d_dst, const void *h_src, size_t bytes)
{
    if (!c || !d_dst || !h_src) return fail(QPSK_ERR_ARG, "null argument");
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QPSK_OK;
}

int qpsk_dev_download(qpsk_ctx *c, void *h_dst, const void *d_src, size_t bytes)
{
    if (!c || !h_dst || !d_src) return fail(QPSK_ERR_ARG, "null argument");
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return check_status(c);   /* the bytes just handed over may come from a call whose kernel flagged its results */
}

/* test hook: order-independent hash of the device sin/cos over float bit patterns [first, first+count) in both signs */
int qpsk_selftest_sincos_hash(qpsk_ctx *c, uint32_t first, uint32_t count, unsigned long long *h_out)
{
    if (!c || !h_out) return fail(QPSK_ERR_ARG, "null argument");
    if (bind(c)) return QPSK_ERR_HIP;
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, sizeof *d));
    HIP_TRY(hipMemsetAsync(d, 0, sizeof *d, c->stream));
    KERNEL_TRY(launch_sincos_hash(first, count, d, c->stream));
    HIP_TRY(hipMemcpyAsync(h_out, d, sizeof *d, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(d));
    return QPSK_OK;
}

} /* extern "C" */
