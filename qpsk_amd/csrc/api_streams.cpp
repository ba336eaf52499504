/*
 * api_streams.cpp -- the running streams of the C ABI (qpsk_streams_*: carried filter, decimation, loop and carrier state from
 * block to block, stream_route and what executes it) and the transmit side (qpsk_tx_*).  Owns qpsk_ctx::streams and qpsk_ctx::tx.
 */
#include "api_ctx.h"

using namespace qpsk;

/* --------------------------------------------------------------- streams */
/* no streams (qpsk_streams_reset on another count, qpsk_ctx_destroy): behind a synchronisation of the context's stream */
void Streams::release()
{
    if (h_stage) hipHostFree(h_stage);
    hipFree(d_stage);
    h_stage = d_stage = nullptr;
    stage_cap = 0;
    hipFree(s_memory); hipFree(s_dec); hipFree(s_loop); hipFree(s_mixer); hipFree(s_ctab); hipFree(s_cstate);
    s_memory = s_dec = s_loop = s_mixer = s_ctab = s_cstate = nullptr;
    poison();      /* nothing is carried; qpsk_streams_reset takes the flag back once it has completed */
    nstreams = 0;
}

/* A stream call enqueues several launches and keeps host-side books about them (which carrier table is current, the relay's turn, a
 * table half built).  If it fails between its launches -- or a kernel reports that it gave up (QPSK_ERR_HIP from the status word) -- the
 * carried state of the streams is undefined: the shared carrier is dropped and every later stream call is refused until
 * qpsk_streams_reset().  Argument errors and flagged NUMBERS (QPSK_ERR_RANGE: NaN samples, a phase beyond the bounded wrap) do not
 * poison: the kernels completed and the state is what the reference's would be or fenced as documented. */
static int stream_call_done(qpsk_ctx *c, int rc)
{
    if (rc == QPSK_ERR_HIP || rc == QPSK_ERR_ALLOC) c->streams.poison();
    return rc;
}

static int streams_usable(qpsk_ctx *c, const char *who)
{
    if (c->streams.nstreams <= 0) return fail(QPSK_ERR_STATE, "call qpsk_streams_reset() first");
    if (c->streams.streams_poisoned)
        return fail(QPSK_ERR_STATE, "%s: an earlier stream call failed between its launches; the streams' carried state is undefined until qpsk_streams_reset()", who);
    c->streams.stream_work_unchecked = true;      /* every caller goes on to enqueue stream work (or to read what such work left) */
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
    const long long nl = (long long)c->streams.nstreams * c->prm.frame_size;
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
    bool wanted = c->streams.nstreams >= from;
    /* short blocks (the one-launch kernel's range), shared carrier: a workgroup's time shrinks with the block, so the kernel pays from
     * ~1.4 M samples per block of all streams on -- 106.7 us against 151.9 (one launch per block) and 117.1 (kernels apart) at
     * 1024 x 2048, 61.8 against 95.9 and 80.6 at 2048 x 1024, 41.7 against 71.7 and 61.8 at 4096 x 512; below that the one-launch
     * kernel is ahead (profiles/r04_streams_short_blocks.txt) */
    if (pcm && shared_carrier && c->prm.frame_size <= stream_block_max_frame())
        wanted = (long long)c->streams.nstreams * c->prm.frame_size >= 1400000LL && c->streams.nstreams >= 256;
    return c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0 && tuned(c->tune.generic, 0) == 0 && (c->cycles == 8 || c->cycles == 4) &&
           (c->prm.timing_mode == QPSK_TIMING_HIST || c->prm.timing_mode == QPSK_TIMING_FIXED) && c->prm.frame_size % stream_scan_tile() == 0 &&
           tuned(c->tune.stream_scan, wanted ? 1 : 0) != 0;
}

/* pcm: in is int16 PCM, otherwise complex float samples; want_sym: the caller takes the symbols (the one-launch kernel always writes them) */
static void stream_route(const qpsk_ctx *c, bool pcm, const void *in, bool want_sym, StreamRoute *rt)
{
    *rt = StreamRoute{};
    rt->carrier = pcm && c->streams.carrier_shared && tuned(c->tune.stream_carrier, 1) != 0;      /* the one carrier is in use */
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
    c->streams.streams_poisoned = true;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nstreams != c->streams.nstreams) {
        c->streams.release();
        const size_t n = (size_t)nstreams;
        if (hipMalloc((void **)&c->streams.s_memory, sizeof(float) * 2 * QPSK_NTAPS * n) != hipSuccess ||
            hipMalloc((void **)&c->streams.s_dec, sizeof(float) * 2 * c->nsym * n) != hipSuccess ||
            hipMalloc((void **)&c->streams.s_loop, sizeof(float) * 2 * n) != hipSuccess ||
            hipMalloc((void **)&c->streams.s_ctab, sizeof(float) * 2 * 2 * (size_t)c->prm.frame_size) != hipSuccess ||
            hipMalloc((void **)&c->streams.s_cstate, sizeof(float) * 8) != hipSuccess ||
            hipMalloc((void **)&c->streams.s_mixer, sizeof(float) * 4 * n) != hipSuccess) {
            c->streams.release();
            return fail(QPSK_ERR_ALLOC, "hipMalloc of stream state failed");
        }
        c->streams.nstreams = nstreams;
    }
    const size_t n = (size_t)nstreams;
    HIP_TRY(hipMemsetAsync(c->streams.s_memory, 0, sizeof(float) * 2 * QPSK_NTAPS * n, c->stream));
    HIP_TRY(hipMemsetAsync(c->streams.s_dec, 0, sizeof(float) * 2 * c->nsym * n, c->stream));
    HIP_TRY(hipMemsetAsync(c->streams.s_loop, 0, sizeof(float) * 2 * n, c->stream));
    /* fbb_rx_phase = cmplx(0.0f); fbb_rx_rect = cmplxconj(TAU * hz / FS)  (qpsk.c:341-342) */
    float rect[2];
    qpsk_host_rect(mixer_hz, c->prm.fs, rect);
    std::vector<float> m(4 * n);
    for (size_t i = 0; i < n; i++) { m[4 * i] = 1.0f; m[4 * i + 1] = 0.0f; m[4 * i + 2] = rect[0]; m[4 * i + 3] = rect[1]; }
    HIP_TRY(hipMemcpyAsync(c->streams.s_mixer, m.data(), sizeof(float) * m.size(), hipMemcpyHostToDevice, c->stream));
    /* one carrier for all of them: the first block's phases now, every later block's by the block before it (streamscan.hip MODE 2) */
    const float cst[8] = {1.0f, 0.0f, rect[0], rect[1], 1.0f, 0.0f, 0.0f, 0.0f};
    HIP_TRY(hipMemcpyAsync(c->streams.s_cstate, cst, sizeof cst, hipMemcpyHostToDevice, c->stream));
    c->streams.carrier_shared = false;
    c->streams.carrier_blocks = 0;
    c->streams.carrier_scans = 0;
    c->streams.carrier_pending = nullptr;
    if (c->prm.frame_size % 2 == 0 && (stream_scan_ok(c, true, true) || stream_block_ok(c, true))) {      /* (a kernel that uses it would take these streams) */
        KERNEL_TRY(launch_carrier_table(c->streams.s_cstate, c->streams.s_ctab, c->prm.frame_size, false, c->stream));
        c->streams.carrier_shared = true;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* the one-launch kernel's wave counter: whatever an earlier, failed call left between the host's expectation and the device's count
     * (a polled call whose synchronisation failed had already advanced done_expect), the stream is idle now: back in step */
    if (c->streams.h_done) c->streams.done_expect = *(volatile unsigned *)c->streams.h_done;
    (void)__atomic_exchange_n(c->status.h_status, 0, __ATOMIC_ACQ_REL);      /* a status word left by the call that poisoned the streams belongs to it */
    c->streams.streams_poisoned = false;
    return QPSK_OK;
}

/* the shared carrier ends: every stream's mixer state = the phase the next block starts from (before any other reader of s_mixer) */
static int carrier_to_streams(qpsk_ctx *c)
{
    if (!c->streams.carrier_shared) return QPSK_OK;
    KERNEL_TRY(launch_carrier_broadcast(c->streams.s_cstate, c->streams.s_mixer, c->streams.nstreams, c->stream));
    c->streams.carrier_shared = false;
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
    *cur = c->streams.s_ctab + L2 * (c->streams.carrier_blocks & 1u);
    *next = c->streams.s_ctab + L2 * ((c->streams.carrier_blocks + 1u) & 1u);
    return QPSK_OK;
}

int qpsk_streams_set_loop_state(qpsk_ctx *c, const float *h_state)
{
    if (!c || !h_state) return fail(QPSK_ERR_ARG, "null argument");
    if (int ru = streams_usable(c, "qpsk_streams_set_loop_state")) return ru;
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(c->streams.s_loop, h_state, sizeof(float) * 2 * (size_t)c->streams.nstreams, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QPSK_OK;
}

int qpsk_streams_get_loop_state(qpsk_ctx *c, float *h_state)
{
    if (!c || !h_state) return fail(QPSK_ERR_ARG, "null argument");
    if (int ru = streams_usable(c, "qpsk_streams_get_loop_state")) return ru;
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(h_state, c->streams.s_loop, sizeof(float) * 2 * (size_t)c->streams.nstreams, hipMemcpyDeviceToHost, c->stream));
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
    a.cstate = ctab ? c->streams.s_cstate : nullptr;
    a.pcm = pcm;
    a.cplx = reinterpret_cast<const float2 *>(cplx);
    a.mixer = c->streams.s_mixer;
    a.memory = reinterpret_cast<float2 *>(c->streams.s_memory);
    a.dec = reinterpret_cast<float2 *>(c->streams.s_dec);
    a.loop = c->streams.s_loop;
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
    a.status = c->status.d_status;
    a.done = count ? c->streams.d_done : nullptr;
    KERNEL_TRY(launch_stream_block(a, c->streams.nstreams, c->stream, inl));
    if (ctab) c->streams.carrier_blocks++;      /* the tables flip only once the launch that fills the next one is in the stream */
    c->last_kernel = "stream_block_kernel";
    return QPSK_OK;
}

static int streams_copy_loop(qpsk_ctx *c, float *d_freq, float *d_phase)
{
    const int n = c->streams.nstreams;
    if (d_phase) HIP_TRY(hipMemcpy2DAsync(d_phase, sizeof(float), c->streams.s_loop, 2 * sizeof(float), sizeof(float), n, hipMemcpyDeviceToDevice, c->stream));
    if (d_freq) HIP_TRY(hipMemcpy2DAsync(d_freq, sizeof(float), c->streams.s_loop + 1, 2 * sizeof(float), sizeof(float), n, hipMemcpyDeviceToDevice, c->stream));
    return QPSK_OK;
}

/* A block of the running streams from the rrc_fir() call on (qpsk.c:125-212), in the context's `filtered` and `index` buffers (stream_run()
 * has sized them).  scanned: stream_scan_kernel has left the filtered block there, planar by decimation phase, and the index, and has
 * updated the delay lines; otherwise d_in is the complex block to filter. */
static int streams_from_filter(qpsk_ctx *c, const float *d_in, bool scanned, uint8_t *d_sym, float *d_freq, float *d_phase,
                               float *d_costas, int32_t *d_index)
{
    const int n = c->streams.nstreams, L = c->prm.frame_size, N = c->nsym;
    float *filt = (float *)c->filtered.p;
    int32_t *idx = (int32_t *)c->index.p;
    if (!scanned) {
        /* qpsk.c:125 */
        KERNEL_TRY(fir_full_rate(c, d_in, c->streams.s_memory, filt, n, L));
        KERNEL_TRY(launch_delay_line(d_in, c->streams.s_memory, n, L, c->stream));
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
    if (int rc = costas_over_symbols(c, c->streams.s_dec, n, N, N, c->streams.s_loop, d_sym, d_costas, filt, idx, scanned)) return rc;
    if (d_index) HIP_TRY(hipMemcpyAsync(d_index, idx, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    c->last_kernel = scanned ? "stream_scan_kernel + costas_pipe_kernel"
                             : tuned(c->tune.generic, 0) ? "filter, timing, costas_kernel, decimate_kernel" : "filter, timing, costas_pipe_kernel";
    return streams_copy_loop(c, d_freq, d_phase);
}

/* Executes a route.  d_pcm / d_cplx: the block the route was made for, in device memory, exactly one of them */
static int stream_run(qpsk_ctx *c, const StreamRoute &rt, const int16_t *d_pcm, const float *d_cplx, uint8_t *d_sym, float *d_freq,
                      float *d_phase, float *d_costas, int32_t *d_index)
{
    const int n = c->streams.nstreams, L = c->prm.frame_size;
    if (rt.mixer) {
        if (int rc = ensure(c, c->mixed, sizeof(float) * 2 * (size_t)n * L)) return rc;
        /* qpsk.c:114-120 */
        if (int rb = carrier_to_streams(c)) return rb;
        KERNEL_TRY(launch_mixer(d_pcm, (float *)c->mixed.p, c->streams.s_mixer, n, L, c->stream));
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
        KERNEL_TRY(launch_stream_scan(d_pcm, d_cplx, c->streams.s_mixer, c->streams.s_memory, (float *)c->filtered.p, c->d_taps, (int32_t *)c->index.p, n, L,
                                      c->status.d_status, c->stream, ctab, ctab_next, c->streams.s_cstate, ctab ? c->streams.carrier_scans : 0u, c->cycles));
        if (ctab) {      /* the bookkeeping describes launches that ARE in the stream: the tables flip, the relay's turn advances, the rest of the
                          * next table is owed (a failure between here and the launch that pays it poisons the streams: stream_call_done) */
            c->streams.carrier_blocks++;
            c->streams.carrier_scans++;
            c->streams.carrier_pending = ctab_next;
        }
    }
    const int rc = streams_from_filter(c, d_cplx, rt.kind == SK_SCAN, d_sym, d_freq, d_phase, d_costas, d_index);
    if (c->streams.carrier_pending) {      /* the loop kernel was never reached: the table is finished all the same */
        float *tab = c->streams.carrier_pending;
        c->streams.carrier_pending = nullptr;
        KERNEL_TRY(launch_carrier_table(c->streams.s_cstate, tab, L, true, c->stream));
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
    const size_t n = (size_t)c->streams.nstreams, L = (size_t)c->prm.frame_size, N = (size_t)c->nsym;
    /* arena layout, every part 16-byte aligned: in = [loop 8n | pcm 2nL], out = [sym nN | costas 8nN | loop 8n | index 4n] */
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_loop = 0, o_pcm = al(8 * n), in_bytes = o_pcm + al(2 * n * L);
    const size_t o_sym = in_bytes, o_cos = o_sym + al(n * N), o_lout = o_cos + al(8 * n * N), o_idx = o_lout + al(8 * n),
                 total = o_idx + al(4 * n);
    if (c->streams.stage_cap < total) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->streams.h_stage) hipHostFree(c->streams.h_stage);
        hipFree(c->streams.d_stage);
        c->streams.h_stage = c->streams.d_stage = nullptr;
        c->streams.stage_cap = 0;
        if (hipHostMalloc((void **)&c->streams.h_stage, total, hipHostMallocDefault) != hipSuccess ||
            hipMalloc((void **)&c->streams.d_stage, total) != hipSuccess)
            return fail(QPSK_ERR_ALLOC, "staging buffers of %zu bytes", total);
        c->streams.stage_cap = total;
    }
    if (h_loop_io) memcpy(c->streams.h_stage + o_loop, h_loop_io, 8 * n);
    memcpy(c->streams.h_stage + o_pcm, h_pcm, 2 * n * L);
    /* the route of the block where the kernels apart would read it, in the device arena (16-byte aligned, symbols always wanted) */
    StreamRoute rt;
    stream_route(c, true, c->streams.d_stage + o_pcm, true, &rt);
    bool polled = false;
    if (rt.kind == SK_BLOCK && !rt.mixer) {
        /* one launch, no copy engine: the kernel reads the PCM (and the loop state) from the pinned staging buffer and leaves its
         * results there -- a kilobyte in, a few hundred bytes out per stream */
        unsigned char *m = nullptr;
        HIP_TRY(hipHostGetDevicePointer((void **)&m, c->streams.h_stage, 0));
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
            c->streams.done_expect += 2u * (unsigned)n;
            const volatile unsigned *dn = c->streams.h_done;
            struct timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            for (unsigned spins = 0; (int)(*dn - c->streams.done_expect) < 0; ) {
                cpu_relax();
                if ((++spins & 4095u) == 0) {
                    clock_gettime(CLOCK_MONOTONIC, &t1);
                    if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > 2.0) break;
                }
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            if ((int)(*dn - c->streams.done_expect) < 0) {
                HIP_TRY(hipStreamSynchronize(c->stream));
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                if ((int)(*dn - c->streams.done_expect) < 0) {
                    const unsigned have = *dn, want = c->streams.done_expect;
                    c->streams.done_expect = have;
                    (void)check_status(c);      /* take the kernel's own word, if it left one, out of the status word */
                    return fail(QPSK_ERR_HIP, "stream_block_kernel: %u of %u waves reported completion; the block's results are invalid",
                                2u * (unsigned)n - (want - have), 2u * (unsigned)n);
                }
            }
        }
    } else {
        const size_t up0 = h_loop_io ? o_loop : o_pcm;
        HIP_TRY(hipMemcpyAsync(c->streams.d_stage + up0, c->streams.h_stage + up0, in_bytes - up0, hipMemcpyHostToDevice, c->stream));
        if (h_loop_io) HIP_TRY(hipMemcpyAsync(c->streams.s_loop, c->streams.d_stage + o_loop, 8 * n, hipMemcpyDeviceToDevice, c->stream));
        if (int rc = stream_run(c, rt, (const int16_t *)(c->streams.d_stage + o_pcm), nullptr, c->streams.d_stage + o_sym, nullptr, nullptr,
                                h_costas ? (float *)(c->streams.d_stage + o_cos) : nullptr, (int32_t *)(c->streams.d_stage + o_idx)))
            return rc;
        HIP_TRY(hipMemcpyAsync(c->streams.d_stage + o_lout, c->streams.s_loop, 8 * n, hipMemcpyDeviceToDevice, c->stream));
        /* one copy down: from the symbols to the index (costas_frame[] in between travels even when it is not wanted
         * only if it was computed: without it the two parts around it go separately) */
        if (h_costas) {
            HIP_TRY(hipMemcpyAsync(c->streams.h_stage + o_sym, c->streams.d_stage + o_sym, total - o_sym, hipMemcpyDeviceToHost, c->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(c->streams.h_stage + o_sym, c->streams.d_stage + o_sym, al(n * N), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(c->streams.h_stage + o_lout, c->streams.d_stage + o_lout, total - o_lout, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (!polled) HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c)) return st;
    memcpy(h_sym, c->streams.h_stage + o_sym, n * N);
    if (h_costas) memcpy(h_costas, c->streams.h_stage + o_cos, 8 * n * N);
    if (h_loop_io) memcpy(h_loop_io, c->streams.h_stage + o_lout, 8 * n);
    if (h_index) memcpy(h_index, c->streams.h_stage + o_idx, 4 * n);
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
void Transmitters::release()
{
    hipFree(t_hist); hipFree(t_mixer);
    tx_b.release();
    *this = Transmitters();
}

int qpsk_tx_reset(qpsk_ctx *c, int nstreams, double tx_hz)
{
    if (!c || nstreams <= 0) return fail(QPSK_ERR_ARG, "qpsk_tx_reset: bad argument");
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)nstreams;
    const size_t hist_bytes = (size_t)tx_history_symbols() * n;
    if (nstreams != c->tx.ntx) {
        hipFree(c->tx.t_hist); hipFree(c->tx.t_mixer);
        c->tx.t_hist = nullptr;
        c->tx.t_mixer = nullptr;
        c->tx.ntx = 0;
        if (hipMalloc((void **)&c->tx.t_hist, hist_bytes) != hipSuccess ||
            hipMalloc((void **)&c->tx.t_mixer, sizeof(float) * 4 * n) != hipSuccess)
            return fail(QPSK_ERR_ALLOC, "hipMalloc of transmitter state failed");
        c->tx.ntx = nstreams;
    }
    /* memset(tx_filter, 0, ...): no symbol sent yet (code 4), i.e. a delay line of zeros */
    HIP_TRY(hipMemsetAsync(c->tx.t_hist, 4, hist_bytes, c->stream));
    /* fbb_tx_phase = cmplx(0.0f); fbb_tx_rect = cmplx(TAU * hz / FS)  (qpsk.c:316,320) */
    float rect[2];
    qpsk_host_rect_tx(tx_hz, c->prm.fs, rect);
    std::vector<float> m(4 * n);
    for (size_t i = 0; i < n; i++) { m[4 * i] = 1.0f; m[4 * i + 1] = 0.0f; m[4 * i + 2] = rect[0]; m[4 * i + 3] = rect[1]; }
    HIP_TRY(hipMemcpyAsync(c->tx.t_mixer, m.data(), sizeof(float) * m.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QPSK_OK;
}

int qpsk_tx_symbols(qpsk_ctx *c, const uint8_t *d_symbols, int nsym, int16_t *d_pcm, float *d_baseband)
{
    if (!c || !d_symbols || (!d_pcm && !d_baseband)) return fail(QPSK_ERR_ARG, "qpsk_tx_symbols: null argument");
    if (c->tx.ntx <= 0) return fail(QPSK_ERR_STATE, "call qpsk_tx_reset() first");
    if (nsym <= 0) return fail(QPSK_ERR_ARG, "nsym = %d", nsym);
    if (bind(c)) return QPSK_ERR_HIP;
    const int n = c->tx.ntx, len = nsym * c->cycles;
    const size_t bytes = sizeof(float) * 2 * (size_t)n * len;
    float *shaped = d_baseband;
    if (!shaped) {
        int rc = ensure(c, c->tx.tx_b, bytes);
        if (rc) return rc;
        shaped = (float *)c->tx.tx_b.p;
    }
    /* qpsk.c:273-282 + 232-238 + 243: Gray map, zero-stuffing and rrc_fir(tx_filter, ...) in one kernel;
     * :248-261 up-mix */
    KERNEL_TRY(launch_tx_shape(d_symbols, c->tx.t_hist, c->d_taps, shaped, n, nsym, c->cycles, c->stream));
    if (d_pcm) KERNEL_TRY(launch_tx_upmix(shaped, d_pcm, c->tx.t_mixer, n, len, c->stream));
    return QPSK_OK;
}
