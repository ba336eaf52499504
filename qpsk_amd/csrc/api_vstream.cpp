/*
 * api_vstream.cpp -- the streaming Viterbi decoder of the C ABI (VITERBI STREAM in include/qpsk_hip.h; kernels: viterbi_stream.hip) and its
 * transmit twin qpsk_conv_encode_stream_batch.  Owns qpsk_ctx::vs and nothing else: no scratch buffer of the context, not the deframer, not the
 * receive streams, not the histogram guess.  The positions of the streams are host numbers (every stream is pushed with the same steps), so
 * what a call emits is known here, without a look at the device.
 */
#include "api_ctx.h"

using namespace qpsk;

/* no decoder (qpsk_ctx_destroy, a reset that replaces it): behind a synchronisation of the context's stream */
void ViterbiStream::release()
{
    hipFree(state);
    *this = ViterbiStream();
}

/* the first bit not yet emitted, with `total` steps in (FLUSH): the last decision point's T - D, 0 before anything was emitted */
static long long vstream_emitted(const ViterbiStream &v, long long total)
{
    return total < v.window ? 0 : std::max<long long>(0, total / v.window * v.window - v.depth);
}

/* the bits the decision points in (total, total + n] emit */
static long long vstream_emits(const ViterbiStream &v, long long n) { return vstream_emitted(v, v.total + n) - vstream_emitted(v, v.total); }

/* the trellis steps of a push of ntx dibits, or 0: not whole periods, or outside 1..131072 */
static int vstream_steps(const ViterbiStream &v, int ntx)
{
    if (ntx < 1 || (2LL * ntx) % v.punct.K) return 0;
    const long long n = 2LL * ntx / v.punct.K * v.punct.period;
    return n >= 1 && n <= VITERBI_MAX_STEPS ? (int)n : 0;
}

/* the launch arguments that do not depend on the call's buffers */
static VStreamArgs vstream_args(const ViterbiStream &v)
{
    VStreamArgs a = {};
    a.nring = (v.depth + v.window) / 64;
    a.dblk = v.depth / 64;
    a.wblk = v.window / 64;
    a.state = v.state;
    a.state_stride = v.stride;
    a.punct = v.punct;
    return a;
}

int qpsk_viterbi_stream_reset(qpsk_ctx *c, int nstreams, int depth, int window, int period, uint32_t keep0, uint32_t keep1)
{
    static const char *const who = "qpsk_viterbi_stream_reset";
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    const Pattern pattern = {period, keep0, keep1};
    CodedLayout l;
    if (int rc = layout_add_pattern(who, &pattern, &l)) return rc;
    if (nstreams < 1) return fail(QPSK_ERR_ARG, "%s: nstreams = %d", who, nstreams);
    if (depth < 64 || window < 64 || depth % 64 || window % 64 || (long long)depth + window > VSTREAM_MAX_SPAN)
        return fail(QPSK_ERR_ARG, "%s: depth = %d, window = %d (multiples of 64, each >= 64, depth + window <= %d)", who, depth, window,
                    VSTREAM_MAX_SPAN);
    if (bind(c)) return QPSK_ERR_HIP;
    ViterbiStream v;
    v.nstreams = nstreams;
    v.depth = depth;
    v.window = window;
    v.punct = l.punct;
    v.punctured = !(period == 1 && keep0 == 1u && keep1 == 1u);
    v.stride = vstream_state_stride((depth + window) / 64);
    if (int rc = replace_state(c, who, "streams", nstreams, v.stride, &v.state)) return rc;      /* a failure leaves the decoder the context has */
    c->vs.release();
    c->vs = v;
    KERNEL_TRY(launch_vstream_init(vstream_args(c->vs), nstreams, c->stream));
    c->last_kernel = "viterbi_stream_init_kernel";
    return QPSK_OK;
}

int qpsk_viterbi_stream_emits(qpsk_ctx *c, int ntx)
{
    if (!c) return fail(QPSK_ERR_ARG, "qpsk_viterbi_stream_emits: null context");
    if (!c->vs.state) return fail(QPSK_ERR_STATE, "qpsk_viterbi_stream_emits: no qpsk_viterbi_stream_reset yet");
    const int n = vstream_steps(c->vs, ntx);
    if (!n) return fail(QPSK_ERR_ARG, "qpsk_viterbi_stream_emits: ntx = %d is not whole periods of %d sent bits, or not 1..%d steps", ntx, c->vs.punct.K, VITERBI_MAX_STEPS);
    return (int)vstream_emits(c->vs, n);
}

/* what push and flush ask of their outputs; nbits = the bits the call emits */
static int vstream_outputs(const char *who, long long nbits, const uint8_t *d_bits, long long *bits_pitch, const int32_t *d_info)
{
    if (!d_bits && !d_info) return fail(QPSK_ERR_ARG, "%s: every output is NULL", who);
    if ((uintptr_t)d_info % 4) return fail(QPSK_ERR_ARG, "%s: d_info is not 4-byte aligned", who);
    const long long need = (nbits + 7) / 8;
    if (*bits_pitch == 0) *bits_pitch = need;      /* (not pitch_ok: without d_bits any pitch passes) */
    if (d_bits && *bits_pitch < need) return fail(QPSK_ERR_ARG, "%s: bits_pitch = %lld (0, or >= %lld bytes for the %lld bits of this call)", who, *bits_pitch, need, nbits);
    return QPSK_OK;
}

int qpsk_viterbi_stream_push(qpsk_ctx *c, const int8_t *d_soft, long long row_pitch, int ntx, uint8_t *d_bits, long long bits_pitch,
                             int32_t *d_info, int *h_nbits)
{
    static const char *const who = "qpsk_viterbi_stream_push";
    if (!c || !d_soft) return fail(QPSK_ERR_ARG, "%s: null context or input", who);
    ViterbiStream &v = c->vs;
    if (!v.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_viterbi_stream_reset yet", who);
    const int n = vstream_steps(v, ntx);
    if (!n) return fail(QPSK_ERR_ARG, "%s: ntx = %d is not whole periods of %d sent bits, or not 1..%d steps", who, ntx, v.punct.K, VITERBI_MAX_STEPS);
    size_t pitch = 0;
    if (!pitch_ok(row_pitch, ntx, LLONG_MAX, &pitch)) return fail(QPSK_ERR_ARG, "%s: row_pitch = %lld (0, or >= ntx %d)", who, row_pitch, ntx);
    if ((uintptr_t)d_soft % 2) return fail(QPSK_ERR_ARG, "%s: d_soft is not 2-byte aligned", who);
    if (v.total > LLONG_MAX - n) return fail(QPSK_ERR_ARG, "%s: the position would leave 64 bits", who);
    const long long nbits = vstream_emits(v, n);
    if (int rc = vstream_outputs(who, nbits, d_bits, &bits_pitch, d_info)) return rc;
    if (bind(c)) return QPSK_ERR_HIP;
    VStreamArgs a = vstream_args(v);
    a.soft = d_soft;
    a.pitch = pitch;
    a.n = n;
    a.pc = (int)(v.total % 64);
    a.slot = (int)((v.total - v.advanced) / 64 % a.nring);
    a.have = (int)std::min<long long>(v.total / 64, a.nring);
    a.wphase = (int)(v.total / 64 % a.wblk);
    a.bits = d_bits;
    a.bits_pitch = (size_t)bits_pitch;
    a.info = d_info;
    KERNEL_TRY(launch_vstream_push(a, v.nstreams, v.punctured, c->stream));
    v.total += n;
    c->last_kernel = v.punctured ? "viterbi_stream_punct_kernel" : "viterbi_stream_kernel";
    if (h_nbits) *h_nbits = (int)nbits;
    return QPSK_OK;
}

int qpsk_viterbi_stream_flush(qpsk_ctx *c, int flags, uint8_t *d_bits, long long bits_pitch, int32_t *d_info, int *h_nbits)
{
    static const char *const who = "qpsk_viterbi_stream_flush";
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    ViterbiStream &v = c->vs;
    if (!v.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_viterbi_stream_reset yet", who);
    if (flags & ~QPSK_VITERBI_STREAM_TERMINATED) return fail(QPSK_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    static_assert(QPSK_VITERBI_STREAM_TERMINATED == VSTREAM_TERMINATED, "the kernel takes the header's flag value");
    const long long first = vstream_emitted(v, v.total), nbits = v.total - first;      /* < depth + window */
    if (int rc = vstream_outputs(who, nbits, d_bits, &bits_pitch, d_info)) return rc;
    if (bind(c)) return QPSK_ERR_HIP;
    VStreamArgs a = vstream_args(v);
    a.flags = flags;
    a.pc = (int)(v.total % 64);
    const long long blocks = (v.total - v.advanced + 63) / 64;      /* of the ring's numbering, the partial one included */
    a.slot = blocks ? (int)((blocks - 1) % a.nring) : 0;
    a.have = (int)((v.total + 63) / 64 - first / 64);
    a.bits = d_bits;
    a.bits_pitch = (size_t)bits_pitch;
    a.info = d_info;
    KERNEL_TRY(launch_vstream_flush(a, v.nstreams, c->stream));
    v.total = v.advanced = 0;
    c->last_kernel = "viterbi_stream_flush_kernel";
    if (h_nbits) *h_nbits = (int)nbits;
    return QPSK_OK;
}

/* test hook (tests/test_viterbi_stream_gpu.py): host bookkeeping behind a synchronisation */
int qpsk_test_viterbi_stream_advance(qpsk_ctx *c, long long delta)
{
    static const char *const who = "qpsk_test_viterbi_stream_advance";
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    if (delta < 0 || delta > (1LL << 62)) return fail(QPSK_ERR_ARG, "%s: delta = %lld outside 0..2^62", who, delta);
    ViterbiStream &v = c->vs;
    if (!v.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_viterbi_stream_reset yet", who);
    if (delta % v.window) return fail(QPSK_ERR_ARG, "%s: delta = %lld is not a multiple of the window %d", who, delta, v.window);
    if (v.total < v.depth + v.window) return fail(QPSK_ERR_STATE, "%s: the streams have seen %lld steps, fewer than depth + window = %d", who, v.total, v.depth + v.window);
    if (v.total > LLONG_MAX - delta) return fail(QPSK_ERR_ARG, "%s: the position would leave 64 bits", who);
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    v.total += delta;
    v.advanced += delta;
    return QPSK_OK;
}

int qpsk_conv_encode_stream_batch(qpsk_ctx *c, const uint8_t *d_bits, int nrows, int nbits, int period, uint32_t keep0, uint32_t keep1,
                                  const uint8_t *d_state_in, uint8_t *d_state_out, uint8_t *d_dibits)
{
    static const char *const who = "qpsk_conv_encode_stream_batch";
    if (!c || !d_bits || !d_dibits) return fail(QPSK_ERR_ARG, "%s: null argument", who);
    const Pattern pattern = {period, keep0, keep1};
    CodedLayout l;
    if (int rc = layout_add_pattern(who, &pattern, &l)) return rc;
    if (nrows <= 0 || nbits <= 0 || nbits > VITERBI_MAX_STEPS) return fail(QPSK_ERR_ARG, "%s: nrows = %d, nbits = %d (1..%d)", who, nrows, nbits, VITERBI_MAX_STEPS);
    const long long nsent = coded_nsent(l, nbits);
    if (nbits % period || nsent < 2 || (nsent & 1))
        return fail(QPSK_ERR_ARG, "%s: nbits = %d is not whole periods of %d steps that send whole dibits (%lld sent bits)", who, nbits, period, nsent);
    if (overlap(Span{d_state_in, (size_t)nrows, "d_state_in"}, Span{d_state_out, (size_t)nrows, "d_state_out"}))      /* nrows >= 1; either may be absent */
        return fail(QPSK_ERR_ARG, "%s: d_state_out overlaps d_state_in", who);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_conv_encode_stream(d_bits, nrows, nbits, l.punct, d_state_in, d_state_out, d_dibits, c->stream));
    c->last_kernel = "conv_encode_stream_kernel";
    return QPSK_OK;
}
