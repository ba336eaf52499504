/*
 * api_ctx.cpp -- the C ABI of include/qpsk_hip.h, the context's own part: create and destroy, tuning, the status word, setters
 * and getters, device memory.  The receive calls, the streams, the coded path and the packet path are api_rx.cpp,
 * api_streams.cpp, api_coded.cpp and api_packets.cpp; api_ctx.h is what they share.
 * No arithmetic of the receive path happens in this layer: per-configuration numbers come from host_math.c (as in
 * the reference, on the host), everything per sample runs in the kernels.
 * There is deliberately no CPU fallback: without a usable GPU every entry
 * point fails with QPSK_ERR_NO_DEVICE / QPSK_ERR_HIP.
 */
#include "api_ctx.h"

using namespace qpsk;

static thread_local char g_err[512] = "";

int qpsk::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

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

int qpsk::ensure(qpsk_ctx *c, DevBuf &b, size_t bytes)
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
int qpsk::check_status(qpsk_ctx *c)
{
    const int st = __atomic_exchange_n(c->status.h_status, 0, __ATOMIC_ACQ_REL);
    if (st != STATUS_PIPE_TIMEOUT) c->streams.stream_work_unchecked = false;
    if (st == STATUS_PIPE_TIMEOUT) {
        /* a kernel gave up a bounded wait.  Running streams are affected only if a STREAM call has enqueued work since the status word was
         * last looked at (device-pointer stream calls do not synchronise: their kernels' verdict arrives here, through whichever call
         * synchronises next); a batch call's timeout with no stream work in flight leaves the streams' carried state alone (ADVICE r5:
         * this function used to poison them for any call) */
        if (c->streams.nstreams > 0 && c->streams.stream_work_unchecked) c->streams.poison();
        c->streams.stream_work_unchecked = false;
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
    if (!c || !c->status.h_status) return fail(QPSK_ERR_ARG, "null context");
    __atomic_store_n(c->status.h_status, code, __ATOMIC_RELEASE);
    return QPSK_OK;
}

int qpsk::bind(const qpsk_ctx *c)
{
    HIP_TRY(hipSetDevice(c->device));
    return QPSK_OK;
}

/* make d_gains[0] the context's own (alpha, beta) again after a bandwidth sweep replaced it */
int qpsk::use_context_gains(qpsk_ctx *c)
{
    const float g[2] = {c->alpha, c->beta};
    if (c->h_gains.size() != 2 || c->h_gains[0] != g[0] || c->h_gains[1] != g[1]) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->h_gains.assign(g, g + 2);
        HIP_TRY(hipMemcpyAsync(c->d_gains, c->h_gains.data(), sizeof g, hipMemcpyHostToDevice, c->stream));
    }
    return QPSK_OK;
}

/* the new state of a reset that replaces a group's (api_ctx.h) */
int qpsk::replace_state(qpsk_ctx *c, const char *who, const char *noun, int count, size_t stride, uint8_t **state)
{
    void *p = nullptr;
    if (stride > SIZE_MAX / (size_t)count || hipMalloc(&p, stride * (size_t)count) != hipSuccess) {
        (void)hipGetLastError();
        return fail(QPSK_ERR_ALLOC, "%s: %d %s of %zu bytes of state", who, count, noun, stride);
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        hipFree(p);
        return fail(QPSK_ERR_HIP, "%s: hipStreamSynchronize failed", who);
    }
    *state = (uint8_t *)p;
    return QPSK_OK;
}

/* the two steps of a polyphase stage's reset and the end of its push (api_ctx.h) */
int qpsk::taps_finite(const char *who, const float *h_proto, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!isfinite(h_proto[i])) return fail(QPSK_ERR_ARG, "%s: h_proto[%d] is not finite", who, (int)i);
    return QPSK_OK;
}

int qpsk::polyphase_reset(qpsk_ctx *c, PolyphaseState *fresh, const char *who, const char *sizes, const float *h_head, size_t nhead, size_t nhist,
                          const void *h_tail, size_t ntail)
{
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    if (bind(c)) return QPSK_ERR_HIP;
    const size_t hist_at = (nhead + 1) & ~(size_t)1, floats = hist_at + 2 * nhist;
    float *f = nullptr;
    if (hipMalloc((void **)&f, floats * sizeof(float) + ntail) != hipSuccess) {
        (void)hipGetLastError();
        return fail(QPSK_ERR_ALLOC, "%s: hipMalloc of the state (%s)", who, sizes);
    }
    hipError_t e = hipStreamSynchronize(c->stream);      /* pushes on the old state may still run */
    if (e == hipSuccess) e = hipMemcpy(f, h_head, nhead * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && nhist) e = hipMemset(f + hist_at, 0, 2 * nhist * sizeof(float));
    if (e == hipSuccess && ntail) e = hipMemcpy(f + floats, h_tail, ntail, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(f);
        return fail(QPSK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    fresh->state = reinterpret_cast<uint8_t *>(f);
    fresh->proto = f;
    fresh->hist[0] = nhist ? f + hist_at : nullptr;
    fresh->hist[1] = nhist ? f + hist_at + nhist : nullptr;
    fresh->ready = true;
    return QPSK_OK;
}

int qpsk::polyphase_end_push(qpsk_ctx *c, PolyphaseState &st, const char *kernel, const float2 *in, size_t in_pitch, size_t K, int rows, size_t n)
{
    c->last_kernel = kernel;
    const float2 *hist = reinterpret_cast<const float2 *>(st.hist[st.cur]);
    if (K > 0 && n > 0) KERNEL_TRY(launch_polyphase_history(hist, in, in_pitch, K, rows, n, st.flip(), c->stream));
    st.ready = true;
    return QPSK_OK;
}

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
    KERNEL_TRY(prepare_channel());
    KERNEL_TRY(prepare_synth());
    KERNEL_TRY(prepare_resample());
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
        hipHostMalloc((void **)&c->status.h_status, sizeof(int), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->status.d_status, c->status.h_status, 0) != hipSuccess) {
        qpsk_ctx_destroy(c);
        return fail(QPSK_ERR_ALLOC, "hipMalloc of configuration buffers failed");
    }
    *c->status.h_status = 0;
    if (hipHostMalloc((void **)&c->streams.h_done, sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->streams.d_done, c->streams.h_done, 0) != hipSuccess) {
        qpsk_ctx_destroy(c);
        return fail(QPSK_ERR_ALLOC, "pinned counter");
    }
    *c->streams.h_done = 0;
    int rc = upload_config(c);
    if (rc != QPSK_OK) { qpsk_ctx_destroy(c); return rc; }
    *out = c;
    return QPSK_OK;
}

void qpsk_ctx_destroy(qpsk_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipFree(c->d_taps);
    hipFree(c->d_gains);
    if (c->status.h_status) hipHostFree(c->status.h_status);
    if (c->streams.h_done) hipHostFree(c->streams.h_done);
    for (DevBuf *b : {&c->index, &c->filtered, &c->mixed, &c->keystream, &c->sympad, &c->mislist, &c->datacostas, &c->vitdec, &c->softgain, &c->dfstage})
        b->release();
    for (auto &kv : c->twiddles) hipFree(kv.second);
    hipFree(c->d_fast);
    c->hist.release();
    c->streams.release();
    c->tx.release();
    c->df.release();
    c->framer.release();
    c->vs.release();
    c->outer.release();
    c->nodesync.release();
    c->dispersal.release();
    c->channel.release();
    c->synth.release();
    c->resample.release();
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
extern "C" int qpsk_set_error(int code, const char *msg)
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
