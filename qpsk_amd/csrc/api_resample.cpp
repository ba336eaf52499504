/*
 * api_resample.cpp -- the batched polyphase rational resampler in the C ABI (RESAMPLER in include/qpsk_hip.h; kernels: resample.hip): the
 * stage between a capture's rate and the modem's, rows in at one rate and out at L / D of it.  Owns qpsk_ctx::resample and nothing else.
 */
#include "api_ctx.h"

using namespace qpsk;

/* floor(a / b), b > 0 */
static long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

/* the inputs a push of nout outputs consumes at the position r */
static long long resample_inputs(int r, int L, int D, int nout) { return floor_div((long long)r + (long long)(nout - 1) * D, L) + 1; }

/* what nout alone decides */
static int nout_ok(const char *who, int nout)
{
    if (nout < 1 || nout > RESAMPLE_MAX_OUT) return fail(QPSK_ERR_ARG, "%s: nout = %d outside 1..%d", who, nout, RESAMPLE_MAX_OUT);
    return QPSK_OK;
}

/* ... and what it decides with the resampler's D and L: the kernel's t + L stays below 2^31 */
static int span_ok(const char *who, const Resampler &rs, int nout)
{
    if ((long long)nout * rs.D + rs.L >= (1ll << 31))
        return fail(QPSK_ERR_ARG, "%s: nout D + L = %lld, 2^31 or more", who, (long long)nout * rs.D + rs.L);
    const long long tiles = ((long long)nout + RESAMPLE_TILE - 1) / RESAMPLE_TILE;
    if (tiles * rs.nstreams > INT_MAX)      /* 4 TiB of output */
        return fail(QPSK_ERR_ARG, "%s: %d streams of %d outputs are more than 2^31 - 1 tiles of %d", who, rs.nstreams, nout, RESAMPLE_TILE);
    return QPSK_OK;
}

int qpsk_resample_reset(qpsk_ctx *c, int nstreams, int L, int D, int P, const float *h_proto)
{
    static const char *const who = "qpsk_resample_reset";
    /* what the arguments alone decide comes first: it needs neither a context nor a device */
    if (nstreams < 1 || nstreams > RESAMPLE_MAX_STREAMS) return fail(QPSK_ERR_ARG, "%s: nstreams = %d outside 1..%d", who, nstreams, RESAMPLE_MAX_STREAMS);
    if (L < 1 || L > RESAMPLE_MAX_L) return fail(QPSK_ERR_ARG, "%s: L = %d outside 1..%d", who, L, RESAMPLE_MAX_L);
    if (D < 1 || D > RESAMPLE_MAX_D) return fail(QPSK_ERR_ARG, "%s: D = %d outside 1..%d", who, D, RESAMPLE_MAX_D);
    if (P < 1 || P > RESAMPLE_MAX_P) return fail(QPSK_ERR_ARG, "%s: P = %d outside 1..%d", who, P, RESAMPLE_MAX_P);
    if (!h_proto) return fail(QPSK_ERR_ARG, "%s: null h_proto", who);
    if (int rc = taps_finite(who, h_proto, (size_t)L * P)) return rc;
    /* the state: proto [L P] floats, the two histories [nstreams][P][2] each */
    char sizes[64];
    snprintf(sizes, sizeof sizes, "nstreams = %d, L = %d, P = %d", nstreams, L, P);
    Resampler fresh;
    if (int rc = polyphase_reset(c, &fresh, who, sizes, h_proto, (size_t)L * P, (size_t)nstreams * P * 2, nullptr, 0)) return rc;
    fresh.nstreams = nstreams;
    fresh.L = L;
    fresh.D = D;
    fresh.P = P;
    c->resample.release();
    c->resample = fresh;
    return QPSK_OK;
}

int qpsk_resample_need(qpsk_ctx *c, int nout)
{
    static const char *const who = "qpsk_resample_need";
    if (int rc = nout_ok(who, nout)) return rc;
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    const Resampler &rs = c->resample;
    if (!rs.ready) return fail(QPSK_ERR_STATE, "%s: no resampler (qpsk_resample_reset first; a failed push ends it)", who);
    if (int rc = span_ok(who, rs, nout)) return rc;
    return (int)resample_inputs(rs.r, rs.L, rs.D, nout);      /* below 2^31 behind span_ok */
}

int qpsk_resample_push(qpsk_ctx *c, const float *d_in, long long in_pitch, int nin, int nout, float *d_out, long long out_pitch)
{
    static const char *const who = "qpsk_resample_push";
    if (!d_out) return fail(QPSK_ERR_ARG, "%s: null d_out", who);
    if (int rc = nout_ok(who, nout)) return rc;
    if (nin < 0) return fail(QPSK_ERR_ARG, "%s: nin = %d", who, nin);
    if (nin > 0 && !d_in) return fail(QPSK_ERR_ARG, "%s: null d_in with nin = %d", who, nin);
    size_t ip = 0, op = 0;
    if (!pitch_ok(in_pitch, nin, LLONG_MAX >> 4, &ip)) return fail(QPSK_ERR_ARG, "%s: in_pitch = %lld (0, or >= nin = %d)", who, in_pitch, nin);
    if (!pitch_ok(out_pitch, nout, LLONG_MAX >> 4, &op)) return fail(QPSK_ERR_ARG, "%s: out_pitch = %lld (0, or >= nout = %d)", who, out_pitch, nout);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    Resampler &rs = c->resample;
    if (!rs.ready) return fail(QPSK_ERR_STATE, "%s: no resampler (qpsk_resample_reset first; a failed push ends it)", who);
    if (int rc = span_ok(who, rs, nout)) return rc;
    const long long K = resample_inputs(rs.r, rs.L, rs.D, nout);
    if (nin != K) return fail(QPSK_ERR_ARG, "%s: nin = %d, but the next %d outputs consume %lld (qpsk_resample_need)", who, nin, nout, K);
    if (ip > SIZE_MAX / 16 / (size_t)rs.nstreams || op > SIZE_MAX / 16 / (size_t)rs.nstreams)
        return fail(QPSK_ERR_ARG, "%s: the rows leave the address space", who);
    const size_t cplx = 2 * sizeof(float);
    const Span in = {nin ? d_in : nullptr, nin ? rows_extent(rs.nstreams, ip * cplx, (long long)nin * (long long)cplx) : 0, "d_in"};
    const Span out = {d_out, rows_extent(rs.nstreams, op * cplx, (long long)nout * (long long)cplx), "d_out"};
    if ((uintptr_t)d_out > UINTPTR_MAX - out.bytes || (in.p && (uintptr_t)d_in > UINTPTR_MAX - in.bytes))
        return fail(QPSK_ERR_ARG, "%s: the rows leave the address space", who);
    if (overlap(out, in)) return fail(QPSK_ERR_ARG, "%s: d_out overlaps d_in", who);
    if (bind(c)) return QPSK_ERR_HIP;
    const float2 *x = reinterpret_cast<const float2 *>(nin ? d_in : nullptr);
    KERNEL_TRY(launch_resample_push(x, ip, nin, rs.begin_push(), rs.proto, rs.nstreams, rs.L, rs.D, rs.P, rs.r, nout,
                                    reinterpret_cast<float2 *>(d_out), op, c->stream));
    rs.r += (int)((long long)nout * rs.D - K * rs.L);
    return polyphase_end_push(c, rs, "resample_push_kernel", x, ip, (size_t)nin, rs.nstreams, (size_t)rs.P);      /* K = 0 leaves the history */
}
