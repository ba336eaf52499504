/*
 * api_cross.cpp -- the packet erasure code in the C ABI (PACKET ERASURE CODE in include/qpsk_hip.h; kernels: rs_cross.hip): REED-SOLOMON's
 * code across the packets of a group, and the bookkeeping that sorts a push's packets into groups.  Owns no state of the context: the
 * three calls read its stream and set last_kernel, nothing else.
 */
#include "api_ctx.h"

using namespace qpsk;

namespace {

int code_ok(const char *who, int ngroups, int k, int nroots, int len, int skip)
{
    if (ngroups < 1) return fail(QPSK_ERR_ARG, "%s: ngroups = %d", who, ngroups);
    if (k < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || k + nroots > 255)
        return fail(QPSK_ERR_ARG, "%s: k = %d, nroots = %d (k >= 1, 1 <= nroots <= %d, k + nroots <= 255)", who, k, nroots, RS_MAX_ROOTS);
    if (len < 1 || skip < 0 || skip >= len) return fail(QPSK_ERR_ARG, "%s: len = %d, skip = %d (len >= 1, 0 <= skip < len)", who, len, skip);
    return QPSK_OK;
}

} // namespace

int qpsk_rs_cross_encode_batch(qpsk_ctx *c, uint8_t *d_group, long long pitch, int ngroups, int k, int nroots, int len, int skip)
{
    static const char *const who = "qpsk_rs_cross_encode_batch";
    if (!c || !d_group) return fail(QPSK_ERR_ARG, "%s: null context or d_group", who);
    if (int rc = code_ok(who, ngroups, k, nroots, len, skip)) return rc;
    size_t gp = 0;
    if (!pitch_ok(pitch, len, rs_pitch_limit((long long)ngroups * (k + nroots)), &gp)) return fail(QPSK_ERR_ARG, "%s: pitch = %lld (0, or >= len = %d)", who, pitch, len);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_rs_cross_encode(d_group, gp, ngroups, k, nroots, len, skip, c->stream));
    c->last_kernel = "rs_cross_encode_kernel";
    return QPSK_OK;
}

int qpsk_rs_cross_decode_batch(qpsk_ctx *c, const uint8_t *d_group, long long pitch, int ngroups, int n, int nroots, int len, int skip,
                               const uint8_t *d_have, uint8_t *d_out, long long out_pitch, int32_t *d_info, uint8_t *d_colfail)
{
    static const char *const who = "qpsk_rs_cross_decode_batch";
    if (!c || !d_group || !d_have) return fail(QPSK_ERR_ARG, "%s: null context, d_group or d_have", who);
    if (!d_out && !d_info) return fail(QPSK_ERR_ARG, "%s: d_out and d_info are both NULL", who);
    if (int rc = code_ok(who, ngroups, n - nroots, nroots, len, skip)) return rc;
    const long long rows = (long long)ngroups * n;
    size_t gp = 0, op = 0;
    if (!pitch_ok(pitch, len, rs_pitch_limit(rows), &gp) || !pitch_ok(out_pitch, len, rs_pitch_limit(rows), &op))
        return fail(QPSK_ERR_ARG, "%s: pitch = %lld, out_pitch = %lld (each 0, or >= len = %d)", who, pitch, out_pitch, len);
    if ((uintptr_t)d_info & 3) return fail(QPSK_ERR_ARG, "%s: d_info is not 4-byte aligned", who);
    const Span in = {d_group, rows_extent(rows, gp, len), "d_group"}, out = {d_out, rows_extent(rows, op, len), "d_out"};
    /* in place: exactly the input's packets; a lane reads its column before it writes it, and columns do not meet */
    if (d_out && !(d_out == d_group && op == gp) && overlap(in, out))
        return fail(QPSK_ERR_ARG, "%s: d_out overlaps d_group (allowed: d_out == d_group with the same pitch)", who);
    const Span rest[] = {{d_have, (size_t)rows, "d_have"}, {d_info, 16 * (size_t)ngroups, "d_info"},
                         {d_colfail, (size_t)ngroups * (size_t)(len - skip), "d_colfail"}};
    for (const Span &r : rest)
        if (overlap(r, in) || overlap(r, out)) return fail(QPSK_ERR_ARG, "%s: %s overlaps d_group or d_out", who, r.name);
    if (int rc = first_overlap(who, rest, 3)) return rc;
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_rs_cross_decode(d_group, gp, ngroups, n, nroots, len, skip, d_have, d_out, op, d_info, d_colfail, c->stream));
    c->last_kernel = "rs_cross_decode_kernel";
    return QPSK_OK;
}

int qpsk_rs_cross_place_batch(qpsk_ctx *c, const uint8_t *d_bytes, long long byte_pitch, const int32_t *d_count, const uint8_t *d_crc_ok,
                              int nstreams, int max_packets, int len, int n, int ngroups, const int32_t *d_base, uint8_t *d_group,
                              long long pitch, uint8_t *d_have)
{
    static const char *const who = "qpsk_rs_cross_place_batch";
    if (!c || !d_bytes || !d_count || !d_crc_ok || !d_group || !d_have)
        return fail(QPSK_ERR_ARG, "%s: null context, d_bytes, d_count, d_crc_ok, d_group or d_have", who);
    if (nstreams < 1 || max_packets < 1 || len < 1) return fail(QPSK_ERR_ARG, "%s: nstreams = %d, max_packets = %d, len = %d (each >= 1)", who, nstreams, max_packets, len);
    if (n < 1 || n > 255 || ngroups < 1 || (long long)ngroups * n > 256)
        return fail(QPSK_ERR_ARG, "%s: n = %d, ngroups = %d (1 <= n <= 255, ngroups >= 1, ngroups n <= 256: a sequence number is one byte)", who, n, ngroups);
    const long long window = (long long)ngroups * n, slots = (long long)nstreams * max_packets;
    size_t bp = 0, gp = 0;
    if (!pitch_ok(byte_pitch, len, rs_pitch_limit(slots), &bp) || !pitch_ok(pitch, len, rs_pitch_limit((long long)nstreams * window), &gp))
        return fail(QPSK_ERR_ARG, "%s: byte_pitch = %lld, pitch = %lld (each 0, or >= len = %d)", who, byte_pitch, pitch, len);
    if (((uintptr_t)d_count | (uintptr_t)d_base) & 3) return fail(QPSK_ERR_ARG, "%s: d_count or d_base is not 4-byte aligned", who);
    /* no output may share a byte with an input or with the other output */
    const Span s[] = {{d_group, rows_extent(nstreams * window, gp, len), "d_group"}, {d_have, (size_t)nstreams * (size_t)window, "d_have"}};
    const Span ins[] = {{d_bytes, rows_extent(slots, bp, len), "d_bytes"}, {d_count, 4 * (size_t)nstreams, "d_count"}, {d_crc_ok, (size_t)slots, "d_crc_ok"},
                        {d_base, 4 * (size_t)nstreams, "d_base"}};
    if (overlap(s[0], s[1])) return fail(QPSK_ERR_ARG, "%s: d_have overlaps d_group", who);
    for (const Span &o : s)
        for (const Span &i : ins)
            if (overlap(o, i)) return fail(QPSK_ERR_ARG, "%s: %s overlaps %s", who, o.name, i.name);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_rs_cross_place(d_bytes, bp, d_count, d_crc_ok, nstreams, max_packets, len, n, ngroups, d_base, d_group, gp, d_have, c->stream));
    c->last_kernel = "rs_cross_place_kernel";
    return QPSK_OK;
}
