/*
 * api_channel.cpp -- the two polyphase filter banks in the C ABI.  The channeliser (CHANNELISER in include/qpsk_hip.h; kernels: channel.hip):
 * the stage in front of qpsk_streams_rx_cplx, one wideband capture into the rows that call takes.  The synthesis bank (SYNTHESIS BANK;
 * kernels: synth.hip), its transmit twin: channel rows into one wideband capture.  Owns qpsk_ctx::channel and qpsk_ctx::synth and nothing else;
 * neither bank's calls touch the other's state.
 */
#include "api_ctx.h"

using namespace qpsk;

/* tw[j] = ((float)cos(TAU j / M), (float)sin(TAU j / M)), j < M / 2: fft_lds.h's table rounded to fp32 */
static void channel_twiddles(int M, float *tw)
{
    const double tau = 2.0 * 3.14159265358979323846;
    for (int j = 0; j < M / 2; j++) {
        tw[2 * j] = (float)cos(tau * (double)j / (double)M);
        tw[2 * j + 1] = (float)sin(tau * (double)j / (double)M);
    }
}

int qpsk_channel_twiddles(int M, float *h_tw)
{
    static const char *const who = "qpsk_channel_twiddles";
    if (channel_log2(M) < 0) return fail(QPSK_ERR_ARG, "%s: M = %d is no power of two in 2..%d", who, M, CHANNEL_MAX_M);
    if (!h_tw) return fail(QPSK_ERR_ARG, "%s: null h_tw", who);
    channel_twiddles(M, h_tw);
    return QPSK_OK;
}

/* both banks' reset (who: the entry point; bank: the bank's group of the context c, NULL with a NULL c, which is refused last).  distinct: the
 * synthesis bank's rule for the selection -- no channel twice, hence nsel <= M */
static int bank_reset(qpsk_ctx *c, Channeliser *bank, const char *who, int M, int P, const float *h_proto, const int32_t *h_chan, int nsel,
                      bool distinct)
{
    /* what the arguments alone decide comes first: it needs neither a context nor a device */
    if (channel_log2(M) < 0) return fail(QPSK_ERR_ARG, "%s: M = %d is no power of two in 2..%d", who, M, CHANNEL_MAX_M);
    if (P < 1 || P > CHANNEL_MAX_P) return fail(QPSK_ERR_ARG, "%s: P = %d outside 1..%d", who, P, CHANNEL_MAX_P);
    if (!h_proto) return fail(QPSK_ERR_ARG, "%s: null h_proto", who);
    if (int rc = taps_finite(who, h_proto, (size_t)M * P)) return rc;
    if (!h_chan) nsel = M;
    const int max_sel = distinct ? M : CHANNEL_MAX_SEL;
    if (nsel < 1 || nsel > max_sel) return fail(QPSK_ERR_ARG, "%s: nsel = %d outside 1..%d", who, nsel, max_sel);
    std::vector<int32_t> chan((size_t)nsel);
    std::vector<bool> named(distinct ? (size_t)M : 0);
    for (int i = 0; i < nsel; i++) {
        chan[i] = h_chan ? h_chan[i] : i;
        if (chan[i] < 0 || chan[i] >= M) return fail(QPSK_ERR_ARG, "%s: h_chan[%d] = %d outside 0..M - 1 = %d", who, i, (int)chan[i], M - 1);
        if (distinct) {
            if (named[(size_t)chan[i]]) return fail(QPSK_ERR_ARG, "%s: h_chan[%d] = %d names a channel a second time", who, i, (int)chan[i]);
            named[(size_t)chan[i]] = true;
        }
    }
    /* the state: proto [P M] floats and tw [M / 2][2], the two histories [(P - 1) M][2] each, chan [nsel] */
    const size_t nproto = (size_t)M * P, nhist = (size_t)M * (P - 1) * 2;
    std::vector<float> head(nproto + (size_t)M);
    memcpy(head.data(), h_proto, nproto * sizeof(float));
    channel_twiddles(M, head.data() + nproto);
    char sizes[64];
    snprintf(sizes, sizeof sizes, "M = %d, P = %d, nsel = %d", M, P, nsel);
    Channeliser fresh;
    if (int rc = polyphase_reset(c, &fresh, who, sizes, head.data(), head.size(), nhist, chan.data(), chan.size() * sizeof(int32_t))) return rc;
    fresh.M = M;
    fresh.P = P;
    fresh.nsel = nsel;
    fresh.tw = fresh.proto + nproto;
    fresh.chan = reinterpret_cast<int32_t *>(fresh.proto + head.size() + 2 * nhist);
    bank->release();
    *bank = fresh;
    return QPSK_OK;
}

int qpsk_channel_reset(qpsk_ctx *c, int M, int P, const float *h_proto, const int32_t *h_chan, int nsel)
{
    return bank_reset(c, c ? &c->channel : nullptr, "qpsk_channel_reset", M, P, h_proto, h_chan, nsel, false);
}

/* the scratch outlives a reset: it is sized by the largest push, whatever the bank */
int qpsk_synth_reset(qpsk_ctx *c, int M, int P, const float *h_proto, const int32_t *h_chan, int nsel)
{
    return bank_reset(c, c ? &c->synth.bank : nullptr, "qpsk_synth_reset", M, P, h_proto, h_chan, nsel, true);
}

int qpsk_synth_push(qpsk_ctx *c, const float *d_in, long long in_pitch, int T, float *d_x)
{
    static const char *const who = "qpsk_synth_push";
    if (!d_in || !d_x) return fail(QPSK_ERR_ARG, "%s: null d_in or d_x", who);
    if (T < 1) return fail(QPSK_ERR_ARG, "%s: T = %d", who, T);
    size_t ip = 0;
    if (!pitch_ok(in_pitch, T, LLONG_MAX >> 4, &ip)) return fail(QPSK_ERR_ARG, "%s: in_pitch = %lld (0, or >= T = %d)", who, in_pitch, T);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    Channeliser &b = c->synth.bank;
    if (!b.ready) return fail(QPSK_ERR_STATE, "%s: no synthesis bank (qpsk_synth_reset first; a failed push ends it)", who);
    if ((long long)T * b.M > SYNTH_MAX_SAMPLES)
        return fail(QPSK_ERR_ARG, "%s: T M = %lld samples in one push, more than %lld", who, (long long)T * b.M, SYNTH_MAX_SAMPLES);
    if (ip > SIZE_MAX / 16 / (size_t)b.nsel) return fail(QPSK_ERR_ARG, "%s: the input leaves the address space", who);
    const size_t xn = (size_t)T * b.M, cplx = 2 * sizeof(float);
    const Span in = {d_in, rows_extent(b.nsel, ip * cplx, (long long)T * (long long)cplx), "d_in"}, out = {d_x, xn * cplx, "d_x"};
    if (overlap(out, in)) return fail(QPSK_ERR_ARG, "%s: d_x overlaps d_in", who);
    if (bind(c)) return QPSK_ERR_HIP;
    /* a scratch that has to grow waits for the stream once (ensure); a growth that fails leaves the bank and its history as they were */
    if (int rc = ensure(c, c->synth.scratch, xn * cplx)) return rc;
    float2 *V = reinterpret_cast<float2 *>(c->synth.scratch.p);
    const float2 *hist = b.begin_push();
    KERNEL_TRY(launch_synth_transform(reinterpret_cast<const float2 *>(d_in), ip, T, b.M, reinterpret_cast<const float2 *>(b.tw), b.chan, b.nsel, V,
                                      c->stream));
    KERNEL_TRY(launch_synth_filter(V, hist, T, b.M, b.P, b.proto, reinterpret_cast<float2 *>(d_x), c->stream));
    return polyphase_end_push(c, b, "synth_filter_kernel", V, xn, xn, 1, (size_t)b.M * (b.P - 1));
}

int qpsk_channel_push(qpsk_ctx *c, const float *d_x, int T, float *d_out, long long out_pitch)
{
    static const char *const who = "qpsk_channel_push";
    if (!d_x || !d_out) return fail(QPSK_ERR_ARG, "%s: null d_x or d_out", who);
    if (T < 1) return fail(QPSK_ERR_ARG, "%s: T = %d", who, T);
    size_t op = 0;
    if (!pitch_ok(out_pitch, T, LLONG_MAX >> 4, &op)) return fail(QPSK_ERR_ARG, "%s: out_pitch = %lld (0, or >= T = %d)", who, out_pitch, T);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    Channeliser &ch = c->channel;
    if (!ch.ready) return fail(QPSK_ERR_STATE, "%s: no channeliser (qpsk_channel_reset first; a failed push ends it)", who);
    if ((long long)T * ch.M > CHANNEL_MAX_SAMPLES)
        return fail(QPSK_ERR_ARG, "%s: T M = %lld samples in one push, more than %lld", who, (long long)T * ch.M, CHANNEL_MAX_SAMPLES);
    if (op > SIZE_MAX / 16 / (size_t)ch.nsel) return fail(QPSK_ERR_ARG, "%s: the output leaves the address space", who);
    const size_t xn = (size_t)T * ch.M, cplx = 2 * sizeof(float);
    const Span in = {d_x, xn * cplx, "d_x"}, out = {d_out, rows_extent(ch.nsel, op * cplx, (long long)T * (long long)cplx), "d_out"};
    if (overlap(out, in)) return fail(QPSK_ERR_ARG, "%s: d_out overlaps d_x", who);
    if (bind(c)) return QPSK_ERR_HIP;
    const float2 *x = reinterpret_cast<const float2 *>(d_x);
    KERNEL_TRY(launch_channel_push(x, T, ch.M, ch.P, ch.proto, reinterpret_cast<const float2 *>(ch.tw), ch.begin_push(), ch.chan, ch.nsel,
                                   reinterpret_cast<float2 *>(d_out), op, c->stream));
    return polyphase_end_push(c, ch, "channel_push_kernel", x, xn, xn, 1, (size_t)ch.M * (ch.P - 1));
}
