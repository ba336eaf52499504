/*
 * api_rx.cpp -- the receive side of the C ABI on batches of frames: which kernel takes a batch (rx_route), the timing
 * estimates, every qpsk_rx_batch* entry point, and the stage calls (filter, timing, carrier estimate, Costas, FFT).
 * Owns qpsk_ctx::hist, the one-pass histogram route's guess.  The one unit that reads QPSK_PIPE_PROFILE.
 */
#include "api_ctx.h"

using namespace qpsk;

/* layout bits a product build honours: 4 no spare waves, 8 C++ Costas step, 64/128 lane-mapping variants.  The
 * result-changing ablation bits (1 skip the filter arithmetic, 2 skip the recurrence) and the cycle accounting (32)
 * exist only in the measurement build (make profile, -DQPSK_PIPE_PROFILE) */
#ifdef QPSK_PIPE_PROFILE
static const int PIPE_VARIANT_MASK = ~0;
#else
static const int PIPE_VARIANT_MASK = 4 | 8 | 16 | 64 | 128 | 256 | 512 | 1024 | 8192;
#endif

/* test hook: the one-pass histogram route's books after a synchronisation -- out[0] = the guess the next call will take (-1: none), out[1] = frames
 * the last one-pass call's guess missed, out[2..4] = the statistics the host reads (majority, frames, missed) */
int qpsk_test_hist_state(qpsk_ctx *c, int32_t *out)
{
    if (!c || !out) return fail(QPSK_ERR_ARG, "null argument");
    out[0] = out[1] = out[2] = out[3] = out[4] = -1;
    if (!c->hist.d_hint) return QPSK_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int32_t h[2];
    HIP_TRY(hipMemcpy(h, c->hist.d_hint, sizeof h, hipMemcpyDeviceToHost));
    out[0] = c->hist.hint_valid ? h[0] : -1;
    out[1] = h[1];
    out[2] = c->hist.h_hist_stats[0]; out[3] = c->hist.h_hist_stats[1]; out[4] = c->hist.h_hist_stats[2];
    return QPSK_OK;
}

/* test hook: the runs launch_rrc_fir_stream cuts nframes delay lines of `length` samples into on this context's device -- out = {ntiles,
 * parts, tpp} (kernels.h, FirRuns).  Host arithmetic only: nothing is launched, last_kernel stays */
int qpsk_test_fir_runs(qpsk_ctx *c, int nframes, int length, int32_t out[3])
{
    if (!c || !out) return fail(QPSK_ERR_ARG, "qpsk_test_fir_runs: null argument");
    if (nframes < 1 || length < 1) return fail(QPSK_ERR_ARG, "qpsk_test_fir_runs: nframes %d length %d", nframes, length);
    const FirRuns r = rrc_fir_stream_runs(nframes, length, c->ncu);
    out[0] = r.ntiles; out[1] = r.parts; out[2] = r.tpp;
    return QPSK_OK;
}

void HistGuess::release()
{
    if (d_hint) hipFree(d_hint);
    if (h_hist_stats) hipHostFree(h_hist_stats);
    *this = HistGuess();
}

/* ---------------------------------------------------------------- tiling */
/* full-rate rrc_fir() of a batch of delay lines (rrc_fir.c:17-30): the generated stream with the taps in SGPRs when the
 * filter is symmetric (firstream.hip), the compiler-scheduled kernel for any other tap set (kernels.hip) */
static bool fir_takes_stream(const qpsk_ctx *c) { return c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0; }

int qpsk::fir_full_rate(qpsk_ctx *c, const float *x, const float *memory, float *y, int nframes, int length, size_t in_pitch)
{
    if (fir_takes_stream(c))
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

int qpsk::fft_timing_indices(qpsk_ctx *c, const float *d_in, int nframes, int32_t *d_index, float *d_y, double *d_X, size_t pitch, double *d_bin)
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
                                          c->status.d_status, c->stream, pitch, c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0));
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
    if (!c->hist.d_hint) {
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
        c->hist.d_hint = hint;
        c->hist.h_hist_stats = h_stats;
        c->hist.d_hist_stats = d_stats;
        c->hist.hint_valid = false;
    }
    const int op = tuned(c->tune.hist_onepass, -1);
    /* the route pays only while the guess holds for EVERY frame: a frame it misses goes through the fall-back pass, whose one
     * workgroup takes 0.4 ms whatever the count (a serial chain again) against the 0.07 ms the route saves.  Every histogram-mode call
     * leaves behind how many frames of its batch were off the batch's majority index (or missed by its guess): zero = try the route */
    const int seen = __atomic_load_n(&c->hist.h_hist_stats[1], __ATOMIC_ACQUIRE), off_majority = __atomic_load_n(&c->hist.h_hist_stats[2], __ATOMIC_ACQUIRE);
    const bool guess_is_good = seen > 0 && off_majority == 0;
    if (op == 0 || !c->hist.hint_valid || !(op == 1 || guess_is_good) || !rx_hist_shape_ok(a)) return QPSK_OK;
    if (int rc = ensure(c, c->index, sizeof(int32_t) * (size_t)a.nframes)) return rc;
    if (int rc = ensure(c, c->mislist, sizeof(int32_t) * (size_t)a.nframes)) return rc;
    /* the miss counter starts from zero whatever the last call left: index_majority_kernel resets it, but a call that failed between its
     * launches never got that far, and rx_hist_kernel appends from the count it finds */
    int32_t *mis_count = c->hist.d_hint + 1;
    HIP_TRY(hipMemsetAsync(mis_count, 0, sizeof(int32_t), c->stream));
    KERNEL_TRY(launch_rx_hist(a, (int32_t *)c->index.p, c->hist.d_hint, (int32_t *)c->mislist.p, mis_count, c->status.d_status, c->stream));
    /* the fall-back pass: the generic chunked kernel over the listed frames with their true indices (its grid is sized for the
     * whole batch: the list's length is known on the device only; workgroups beyond it retire at once) */
    FusedArgs af = a;
    af.index = (const int32_t *)c->index.p;
    af.frame_list = (const int32_t *)c->mislist.p;
    af.frame_list_count = mis_count;
    af.G = 4;
    af.S = 64;
    KERNEL_TRY(launch_rx_fused(af, c->stream));
    KERNEL_TRY(launch_index_majority((const int32_t *)c->index.p, a.nframes, c->hist.d_hint, mis_count, c->hist.d_hist_stats, c->stream));
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
        KERNEL_TRY(launch_rx_lean(a, rt.G, rt.layout, c->status.d_status, c->stream));
        c->last_kernel = a.est_tw ? "rx_lean_kernel (FFT timing estimate inside the launch)" : "rx_lean_kernel";
        break;
    case K_PIPE2:
        KERNEL_TRY(launch_rx_pipe2(a, rt.G, rt.layout, c->status.d_status, c->stream));
        c->last_kernel = "rx_pipe2_kernel";
        break;
    case K_FUSED_PIPE:
        KERNEL_TRY(launch_rx_fused_pipe(a, rt.nf, c->status.d_status, c->stream));
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
    a.status = c->status.d_status;
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
    if (hist_guess && c->hist.d_hint && idx && tuned(c->tune.hist_onepass, -1) != 0) {
        /* the batch's majority index as the next histogram-mode call's guess (one workgroup, in stream order) */
        KERNEL_TRY(launch_index_majority(idx, nframes, c->hist.d_hint, c->hist.d_hint + 1, c->hist.d_hist_stats, c->stream));
        c->hist.hint_valid = true;
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
    /* an absent d_out, or an empty one (nout = 0), overlaps nothing */
    if (overlap(Span{d_out, (size_t)nframes * (size_t)nout, "d_out"}, Span{d_data, (size_t)nframes * (size_t)nsym, "d_data"}))
        return fail(QPSK_ERR_ARG, "qpsk_sync_batch: d_out overlaps d_data");
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
int qpsk::costas_over_symbols(qpsk_ctx *c, float *d_symbols, int nframes, int nsym, int dstride, float *d_state,
                              uint8_t *d_sym, float *d_costas, const float *refill, const int32_t *refill_index, bool refill_planar)
{
    float *carrier_tab = c->streams.carrier_pending;
    c->streams.carrier_pending = nullptr;
    if (tuned(c->tune.generic, 0)) {
        if (carrier_tab) KERNEL_TRY(launch_carrier_table(c->streams.s_cstate, carrier_tab, c->prm.frame_size, true, c->stream));
        KERNEL_TRY(launch_costas(d_symbols, nframes, nsym, dstride, 1, c->d_gains, c->min_freq, c->max_freq, d_state, d_state,
                                 d_sym, d_costas, c->status.d_status, c->stream));
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
    a.status = c->status.d_status;
    if (carrier_tab) {
        a.carrier_state = c->streams.s_cstate;
        a.carrier_tab = reinterpret_cast<float2 *>(carrier_tab);
        a.carrier_frame = c->prm.frame_size;
    }
    a.dbg = tuned(c->tune.pipe_variant, 0) & PIPE_VARIANT_MASK;
    int nf = (nframes + c->ncu * pipe_frames(1) - 1) / (c->ncu * pipe_frames(1));
    if (nf < 1) nf = 1;
    if (nf > pipe_max_nf()) nf = pipe_max_nf();
    KERNEL_TRY(launch_costas_pipe(a, nf, c->status.d_status, c->stream));
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
    c->last_kernel = fir_takes_stream(c) ? "rrc_fir_stream_kernel" : "rrc_fir_kernel";
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
    KERNEL_TRY(launch_timing_scan(d_in, nframes, c->prm.frame_size, c->d_taps, d_index, d_hist, c->status.d_status, c->stream, 0,
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
                                  d_line, c->status.d_status, c->taps_symmetric && tuned(c->tune.fir_generic, 0) == 0, c->stream));
    c->last_kernel = "carrier_est_kernel";
    return QPSK_OK;
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
