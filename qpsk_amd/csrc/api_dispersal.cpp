/*
 * api_dispersal.cpp -- DVB's energy dispersal in the C ABI (DVB TRANSPORT in include/qpsk_hip.h; kernel: dispersal.hip): the stage behind
 * qpsk_rs_decode_batch on a DVB-S-shaped link, and in front of qpsk_rs_encode_batch on the way out.  Owns qpsk_ctx::dispersal and nothing
 * else.  The keystream is qpsk_scramble_batch's (host_math.c, pinned to the reference's scramble()), repacked eight bits to the byte.
 */
#include "api_ctx.h"

using namespace qpsk;

/* no table (qpsk_ctx_destroy): behind a synchronisation of the context's stream */
void Dispersal::release()
{
    hipFree(table);
    *this = Dispersal();
}

/* what the arguments of both calls decide by themselves */
static int dispersal_geometry(const char *who, int len, int group, int flags)
{
    static_assert(QPSK_DISPERSAL_MSB_FIRST == DISPERSAL_MSB_FIRST, "the kernel's unit takes the header's flag value");
    if (len < 2 || len > 255) return fail(QPSK_ERR_ARG, "%s: len = %d outside 2..255", who, len);
    if (group < 1 || group > DISPERSAL_MAX_GROUP) return fail(QPSK_ERR_ARG, "%s: group = %d outside 1..%d", who, group, DISPERSAL_MAX_GROUP);
    if (flags & ~QPSK_DISPERSAL_MSB_FIRST) return fail(QPSK_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    return QPSK_OK;
}

/* PR[0 .. group len - 2]: dibit d of the scrambler's keystream is K[2 d] | K[2 d + 1] << 1, so a byte is four dibits */
static void dispersal_bytes(int len, int group, int flags, uint8_t *pr)
{
    const int nbytes = group * len - 1;
    std::vector<unsigned char> ks((size_t)nbytes * 4);
    qpsk_host_scramble_keystream(ks.data(), nbytes * 4);
    for (int t = 0; t < nbytes; t++) {
        unsigned v = 0;
        for (int i = 0; i < 8; i++) {
            const unsigned bit = (ks[4 * t + (i >> 1)] >> (i & 1)) & 1u;
            v |= bit << ((flags & QPSK_DISPERSAL_MSB_FIRST) ? 7 - i : i);
        }
        pr[t] = (uint8_t)v;
    }
}

int qpsk_dispersal_sequence(int len, int group, int flags, uint8_t *out)
{
    static const char *const who = "qpsk_dispersal_sequence";
    if (int rc = dispersal_geometry(who, len, group, flags)) return rc;
    if (!out) return fail(QPSK_ERR_ARG, "%s: null out", who);
    dispersal_bytes(len, group, flags, out);
    return group * len - 1;
}

int qpsk_dispersal_batch(qpsk_ctx *c, const uint8_t *d_in, long long in_pitch, int nrows, int len, int group, int flags, const uint8_t *d_flags,
                         int first, uint8_t *d_out, long long out_pitch)
{
    static const char *const who = "qpsk_dispersal_batch";
    /* what the arguments alone decide comes first: it needs neither a context nor a device */
    if (!d_in || !d_out) return fail(QPSK_ERR_ARG, "%s: null d_in or d_out", who);
    if (int rc = dispersal_geometry(who, len, group, flags)) return rc;
    if (nrows < 1) return fail(QPSK_ERR_ARG, "%s: nrows = %d", who, nrows);
    size_t ip = 0, op = 0;      /* the pitches in force; what is too large for the address space is refused below, in its own words */
    if (!pitch_ok(in_pitch, len, LLONG_MAX, &ip)) return fail(QPSK_ERR_ARG, "%s: in_pitch = %lld (0, or >= len = %d)", who, in_pitch, len);
    if (!pitch_ok(out_pitch, len, LLONG_MAX, &op)) return fail(QPSK_ERR_ARG, "%s: out_pitch = %lld (0, or >= len = %d)", who, out_pitch, len);
    if (d_flags ? first != 0 : (first < 0 || first >= group))
        return fail(QPSK_ERR_ARG, d_flags ? "%s: first = %d with d_flags (the rows' indices are d_flags', first must be 0)" : "%s: first = %d outside 0..group - 1", who, first);
    if (ip > SIZE_MAX / 2 / (size_t)nrows || op > SIZE_MAX / 2 / (size_t)nrows) return fail(QPSK_ERR_ARG, "%s: the buffers leave the address space", who);
    /* in place is allowed, any other shared byte is not */
    const Span in = {d_in, rows_extent(nrows, ip, len), "d_in"}, out = {d_out, rows_extent(nrows, op, len), "d_out"}, fl = {d_flags, (size_t)nrows, "d_flags"};
    if (!(d_out == d_in && op == ip) && overlap(out, in))
        return fail(QPSK_ERR_ARG, "%s: d_out overlaps d_in (in place is d_out == d_in with equal pitches)", who);
    if (overlap(fl, in)) return fail(QPSK_ERR_ARG, "%s: d_flags overlaps d_in", who);
    if (overlap(fl, out)) return fail(QPSK_ERR_ARG, "%s: d_flags overlaps d_out", who);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    if (bind(c)) return QPSK_ERR_HIP;
    Dispersal &d = c->dispersal;
    if (!d.table && hipMalloc(&d.table, (size_t)DISPERSAL_MAX_GROUP * 256) != hipSuccess) {
        (void)hipGetLastError();
        d.table = nullptr;
        return fail(QPSK_ERR_ALLOC, "%s: hipMalloc of the table", who);
    }
    if (d.len != len || d.group != group || d.flags != flags) {
        /* row k of the table: the sync byte's mask, then PR[k len .. k len + len - 2] */
        const int tp = dispersal_table_pitch(len);
        std::vector<uint8_t> pr((size_t)group * len), table((size_t)group * tp, 0);
        dispersal_bytes(len, group, flags, pr.data() + 1);
        pr[0] = 0xFF;
        for (int k = 0; k < group; k++) {
            memcpy(&table[(size_t)k * tp], &pr[(size_t)k * len], (size_t)len);
            if (k) table[(size_t)k * tp] = 0;      /* the generator runs through the sync bytes of packets 1 .. G - 1 and leaves them alone */
        }
        d.len = 0;      /* no table until the copy has succeeded */
        HIP_TRY(hipStreamSynchronize(c->stream));      /* a call on the old table may still run */
        HIP_TRY(hipMemcpy(d.table, table.data(), table.size(), hipMemcpyHostToDevice));
        d.len = len;
        d.group = group;
        d.flags = flags;
    }
    KERNEL_TRY(launch_dispersal(d_in, ip, nrows, len, group, d.table, d_flags, first, d_out, op, c->stream));
    c->last_kernel = "dispersal_kernel";
    return QPSK_OK;
}
