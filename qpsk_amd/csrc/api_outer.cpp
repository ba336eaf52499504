/*
 * api_outer.cpp -- the outer link of a continuous stream in the C ABI (OUTER LINK in include/qpsk_hip.h; kernels: outer.hip): word sync, polarity
 * resolution and the byte deinterleaver behind qpsk_viterbi_stream_push, and the interleaver that is its transmit twin.  Owns qpsk_ctx::outer and
 * nothing else: no scratch buffer of the context, not the stream decoder.  Every stream is pushed with the same bits, so the bits since the
 * reset are a host number; where a stream's lock stands is the device's.
 */
#include "api_ctx.h"

using namespace qpsk;

/* no link (qpsk_ctx_destroy, a reset that replaces it): behind a synchronisation of the context's stream */
void OuterLink::release()
{
    hipFree(state);
    *this = OuterLink();
}

/* the geometry a reset and the interleaver share */
static int outer_geometry(const char *who, int n, int branches)
{
    if (n < 2 || n > 255) return fail(QPSK_ERR_ARG, "%s: n = %d outside 2..255", who, n);
    if (branches < 1 || branches > 32 || n % branches) return fail(QPSK_ERR_ARG, "%s: branches = %d (1..32, a divisor of n = %d)", who, branches, n);
    return QPSK_OK;
}

static OuterArgs outer_args(const OuterLink &o)
{
    OuterArgs a = {};
    a.n = o.n;
    a.branches = o.branches;
    a.sync = o.sync;
    a.lock = o.lock;
    a.drop = o.drop;
    a.flags = o.flags;
    a.state = o.state;
    a.state_stride = o.stride;
    a.total = o.total;
    a.group = o.group;
    return a;
}

/* both resets: group = 0 is the ungrouped link */
static int outer_reset(const char *who, qpsk_ctx *c, int nstreams, int n, int branches, int sync, int lock, int drop, int flags, int group)
{
    static_assert(QPSK_OUTER_POLARITY == OUTER_POLARITY && QPSK_OUTER_MSB_FIRST == OUTER_MSB_FIRST, "the kernel takes the header's flag values");
    /* what the arguments alone decide comes first: it needs neither a context nor a device */
    if (nstreams < 1) return fail(QPSK_ERR_ARG, "%s: nstreams = %d", who, nstreams);
    if (int rc = outer_geometry(who, n, branches)) return rc;
    if (sync < 0 || sync > 255) return fail(QPSK_ERR_ARG, "%s: sync = %d is not one byte", who, sync);
    if (lock < 1 || lock > 16) return fail(QPSK_ERR_ARG, "%s: lock = %d outside 1..16", who, lock);
    if (drop < 0 || drop > 16) return fail(QPSK_ERR_ARG, "%s: drop = %d outside 0..16", who, drop);
    if (flags & ~(QPSK_OUTER_POLARITY | QPSK_OUTER_MSB_FIRST)) return fail(QPSK_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    if (group && (group < 3 || group > 16)) return fail(QPSK_ERR_ARG, "%s: group = %d (0, or 3..16)", who, group);
    if (group && lock < group) return fail(QPSK_ERR_ARG, "%s: lock = %d below group = %d (a look-ahead shorter than a group leaves its phase open)", who, lock, group);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    if (bind(c)) return QPSK_ERR_HIP;
    OuterLink o;
    o.nstreams = nstreams;
    o.n = n;
    o.branches = branches;
    o.sync = sync;
    o.lock = lock;
    o.drop = drop;
    o.flags = flags;
    o.group = group;
    o.stride = outer_state_stride(n, branches, lock);
    if (int rc = replace_state(c, who, "streams", nstreams, o.stride, &o.state)) return rc;      /* a failure leaves the link the context has */
    c->outer.release();
    c->outer = o;
    KERNEL_TRY(launch_outer_init(outer_args(c->outer), nstreams, c->stream));
    c->last_kernel = "outer_init_kernel";
    return QPSK_OK;
}

int qpsk_outer_reset(qpsk_ctx *c, int nstreams, int n, int branches, int sync, int lock, int drop, int flags)
{
    return outer_reset("qpsk_outer_reset", c, nstreams, n, branches, sync, lock, drop, flags, 0);
}

int qpsk_outer_reset_group(qpsk_ctx *c, int nstreams, int n, int branches, int sync, int lock, int drop, int flags, int group)
{
    return outer_reset("qpsk_outer_reset_group", c, nstreams, n, branches, sync, lock, drop, flags, group);
}

int qpsk_outer_max_words(qpsk_ctx *c, int nbits)
{
    static const char *const who = "qpsk_outer_max_words";
    if (nbits < 1 || nbits > OUTER_MAX_BITS) return fail(QPSK_ERR_ARG, "%s: nbits = %d outside 1..%d", who, nbits, OUTER_MAX_BITS);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    const OuterLink &o = c->outer;
    if (!o.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_outer_reset yet", who);
    return o.lock + (nbits + 8 * o.n - 1) / (8 * o.n);
}

int qpsk_outer_push(qpsk_ctx *c, const uint8_t *d_bits, long long bits_pitch, int nbits, int max_words, int32_t *d_count, uint8_t *d_words,
                    long long word_pitch, long long *d_pos, uint8_t *d_flags, int32_t *d_info)
{
    static const char *const who = "qpsk_outer_push";
    if (!c || !d_bits || !d_count) return fail(QPSK_ERR_ARG, "%s: null context, input or d_count", who);
    OuterLink &o = c->outer;
    if (!o.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_outer_reset yet", who);
    if (nbits < 1 || nbits > OUTER_MAX_BITS) return fail(QPSK_ERR_ARG, "%s: nbits = %d outside 1..%d", who, nbits, OUTER_MAX_BITS);
    const long long need = (nbits + 7) / 8;
    size_t bp = 0, wp = 0;      /* the pitches in force; what is too large for the address space is refused below, in its own words */
    if (!pitch_ok(bits_pitch, need, LLONG_MAX, &bp)) return fail(QPSK_ERR_ARG, "%s: bits_pitch = %lld (0, or >= %lld bytes for the %d bits of this call)", who, bits_pitch, need, nbits);
    if (max_words < 0) return fail(QPSK_ERR_ARG, "%s: max_words = %d", who, max_words);
    if (!pitch_ok(word_pitch, o.n, LLONG_MAX, &wp)) return fail(QPSK_ERR_ARG, "%s: word_pitch = %lld (0, or >= n = %d)", who, word_pitch, o.n);
    if ((uintptr_t)d_count % 4 || (uintptr_t)d_info % 4) return fail(QPSK_ERR_ARG, "%s: d_count or d_info is not 4-byte aligned", who);
    if ((uintptr_t)d_pos % 8) return fail(QPSK_ERR_ARG, "%s: d_pos is not 8-byte aligned", who);
    if (o.total > LLONG_MAX - nbits) return fail(QPSK_ERR_ARG, "%s: the position would leave 64 bits", who);
    const size_t S = (size_t)o.nstreams, slots = S * (size_t)max_words;
    if (wp > SIZE_MAX / 2 / (slots ? slots : 1) || bp > SIZE_MAX / 2 / S) return fail(QPSK_ERR_ARG, "%s: the buffers leave the address space", who);
    /* no output may share a byte with the input or with another output; here a buffer is whole pitches, the last row's padding included */
    const Span bufs[] = {{d_bits, S * bp, "d_bits"},   {d_count, S * 4, "d_count"}, {d_words, slots * wp, "d_words"},
                         {d_pos, slots * 8, "d_pos"},  {d_flags, slots, "d_flags"}, {d_info, S * 16, "d_info"}};
    if (int rc = first_overlap(who, bufs, 6)) return rc;
    if (bind(c)) return QPSK_ERR_HIP;
    OuterArgs a = outer_args(o);
    a.bits = d_bits;
    a.bits_pitch = bp;
    a.nbits = nbits;
    a.max_words = max_words;
    a.count = d_count;
    a.words = d_words;
    a.word_pitch = wp;
    a.pos = d_pos;
    a.wflags = d_flags;
    a.info = d_info;
    KERNEL_TRY(launch_outer_push(a, o.nstreams, c->stream));
    o.total += nbits;
    c->last_kernel = "outer_push_kernel";
    return QPSK_OK;
}

/* test hook (tests/test_outer_gpu.py): host bookkeeping behind a synchronisation */
int qpsk_test_outer_advance(qpsk_ctx *c, long long delta)
{
    static const char *const who = "qpsk_test_outer_advance";
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    if (delta < 0 || delta > (1LL << 62) || delta % 8) return fail(QPSK_ERR_ARG, "%s: delta = %lld (a multiple of 8 in 0..2^62)", who, delta);
    OuterLink &o = c->outer;
    if (!o.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_outer_reset yet", who);
    if (o.total > LLONG_MAX - delta) return fail(QPSK_ERR_ARG, "%s: the position would leave 64 bits", who);
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    o.total += delta;
    return QPSK_OK;
}

int qpsk_outer_interleave_batch(qpsk_ctx *c, const uint8_t *d_words, int nrows, int nwords, int n, int branches, const uint8_t *d_hist_in,
                                uint8_t *d_hist_out, uint8_t *d_out)
{
    static const char *const who = "qpsk_outer_interleave_batch";
    /* what the arguments alone decide comes first: it needs neither a context nor a device */
    if (!d_words || !d_out) return fail(QPSK_ERR_ARG, "%s: null d_words or d_out", who);
    if (int rc = outer_geometry(who, n, branches)) return rc;
    if (nrows < 1 || nwords < 1 || nwords > (1 << 20)) return fail(QPSK_ERR_ARG, "%s: nrows = %d, nwords = %d (1..2^20)", who, nrows, nwords);
    const size_t words = (size_t)nrows * (size_t)nwords * (size_t)n, hist = (size_t)nrows * (size_t)(branches - 1) * (size_t)n;
    const Span in = {d_words, words, "d_words"}, hin = {d_hist_in, hist, "d_hist_in"}, out = {d_out, words, "d_out"}, hout = {d_hist_out, hist, "d_hist_out"};
    if (overlap(out, in) || overlap(out, hin)) return fail(QPSK_ERR_ARG, "%s: d_out overlaps an input", who);
    if (overlap(hout, in) || overlap(hout, hin)) return fail(QPSK_ERR_ARG, "%s: d_hist_out overlaps an input", who);
    if (overlap(hout, out)) return fail(QPSK_ERR_ARG, "%s: d_hist_out overlaps d_out", who);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_outer_interleave(d_words, nrows, nwords, n, branches, d_hist_in, d_hist_out, d_out, c->stream));
    c->last_kernel = "outer_interleave_kernel";
    return QPSK_OK;
}
