/*
 * api_nodesync.cpp -- the node sync of the C ABI (NODE SYNC in include/qpsk_hip.h; kernels: nodesync.hip): the candidate transform in front of
 * qpsk_viterbi_stream_push and the monitor that reads that call's d_info.  Owns qpsk_ctx::nodesync and nothing else: no scratch buffer of the
 * context, not the stream decoder, whose d_info it is only handed as a device pointer.  Every link is pushed with the same dibits, so how
 * much of the carried history is real is a host number; which candidate a link stands on is the device's.
 */
#include "api_ctx.h"

using namespace qpsk;

/* no node sync (qpsk_ctx_destroy, a reset that replaces it): behind a synchronisation of the context's stream */
void NodeSync::release()
{
    hipFree(state);
    *this = NodeSync();
}

static NodeSyncArgs nodesync_args(const NodeSync &n)
{
    NodeSyncArgs a = {};
    a.nrot = n.nrot;
    a.nshift = n.nshift;
    a.span = n.span;
    a.settle = n.settle;
    a.thr_num = n.thr_num;
    a.thr_den = n.thr_den;
    a.drop = n.drop;
    a.state = n.state;
    a.have = n.have;
    return a;
}

int qpsk_nodesync_shifts(int period, uint32_t keep0, uint32_t keep1)
{
    const Pattern pattern = {period, keep0, keep1};
    CodedLayout l;
    if (int rc = layout_add_pattern("qpsk_nodesync_shifts", &pattern, &l)) return rc;
    return l.punct.K % 2 ? l.punct.K : l.punct.K / 2;
}

int qpsk_nodesync_reset(qpsk_ctx *c, int nlinks, int nrot, int nshift, int span, int settle, int thr_num, int thr_den, int drop)
{
    static const char *const who = "qpsk_nodesync_reset";
    /* what the arguments alone decide comes first: it needs neither a context nor a device */
    if (nlinks < 1) return fail(QPSK_ERR_ARG, "%s: nlinks = %d", who, nlinks);
    if (nrot != 1 && nrot != 2 && nrot != 4) return fail(QPSK_ERR_ARG, "%s: nrot = %d (1, 2 or 4)", who, nrot);
    if (nshift < 1 || nshift > NODESYNC_MAX_SHIFT) return fail(QPSK_ERR_ARG, "%s: nshift = %d outside 1..%d", who, nshift, NODESYNC_MAX_SHIFT);
    if (span < 1 || span > (1 << 24)) return fail(QPSK_ERR_ARG, "%s: span = %d outside 1..2^24", who, span);
    if (settle < 0 || settle > (1 << 24)) return fail(QPSK_ERR_ARG, "%s: settle = %d outside 0..2^24", who, settle);
    if (thr_num < 0 || thr_num > 65535 || thr_den < 1 || thr_den > 65535)
        return fail(QPSK_ERR_ARG, "%s: threshold %d / %d (0..65535 over 1..65535)", who, thr_num, thr_den);
    if (drop < 1 || drop > 16) return fail(QPSK_ERR_ARG, "%s: drop = %d outside 1..16", who, drop);
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    if (bind(c)) return QPSK_ERR_HIP;
    NodeSync n;
    n.nlinks = nlinks;
    n.nrot = nrot;
    n.nshift = nshift;
    n.span = span;
    n.settle = settle;
    n.thr_num = thr_num;
    n.thr_den = thr_den;
    n.drop = drop;
    if (int rc = replace_state(c, who, "links", nlinks, NODESYNC_STRIDE, &n.state)) return rc;      /* a failure leaves the node sync the context has */
    c->nodesync.release();
    c->nodesync = n;
    KERNEL_TRY(launch_nodesync_init(nodesync_args(c->nodesync), nlinks, nullptr, false, c->stream));
    c->last_kernel = "nodesync_init_kernel";
    return QPSK_OK;
}

int qpsk_nodesync_set(qpsk_ctx *c, const int32_t *d_cand)
{
    static const char *const who = "qpsk_nodesync_set";
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context", who);
    NodeSync &n = c->nodesync;
    if (!n.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_nodesync_reset yet", who);
    if ((uintptr_t)d_cand % 4) return fail(QPSK_ERR_ARG, "%s: d_cand is not 4-byte aligned", who);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_nodesync_init(nodesync_args(n), n.nlinks, d_cand, true, c->stream));
    c->last_kernel = "nodesync_init_kernel";
    return QPSK_OK;
}

int qpsk_nodesync_push(qpsk_ctx *c, const int8_t *d_soft_in, long long in_pitch, int ntx, const int32_t *d_vinfo, int8_t *d_soft_out,
                       long long out_pitch, int32_t *d_info)
{
    static const char *const who = "qpsk_nodesync_push";
    if (!c || !d_soft_in || !d_soft_out) return fail(QPSK_ERR_ARG, "%s: null context, input or d_soft_out", who);
    NodeSync &n = c->nodesync;
    if (!n.state) return fail(QPSK_ERR_STATE, "%s: no qpsk_nodesync_reset yet", who);
    if (ntx < 1 || ntx < n.nshift - 1 || ntx > NODESYNC_MAX_NTX)
        return fail(QPSK_ERR_ARG, "%s: ntx = %d outside max(1, nshift - 1 = %d)..%d", who, ntx, n.nshift - 1, NODESYNC_MAX_NTX);
    size_t ip = 0, op = 0;      /* the pitches in force, which the message shows: ntx for a 0 */
    const bool in_ok = pitch_ok(in_pitch, ntx, LLONG_MAX, &ip), out_ok = pitch_ok(out_pitch, ntx, LLONG_MAX, &op);
    if (!in_ok || !out_ok)
        return fail(QPSK_ERR_ARG, "%s: in_pitch = %lld, out_pitch = %lld (0, or >= ntx %d)", who, (long long)ip, (long long)op, ntx);
    if ((uintptr_t)d_soft_in % 2 || (uintptr_t)d_soft_out % 2) return fail(QPSK_ERR_ARG, "%s: d_soft_in or d_soft_out is not 2-byte aligned", who);
    if ((uintptr_t)d_vinfo % 4 || (uintptr_t)d_info % 4) return fail(QPSK_ERR_ARG, "%s: d_vinfo or d_info is not 4-byte aligned", who);
    const size_t L = (size_t)n.nlinks;
    if (ip > SIZE_MAX / 4 / L || op > SIZE_MAX / 4 / L) return fail(QPSK_ERR_ARG, "%s: the buffers leave the address space", who);
    /* both pointers are given and ntx >= 1: neither range is absent or empty */
    const Span in = {d_soft_in, 2 * rows_extent(n.nlinks, ip, ntx), "d_soft_in"}, out = {d_soft_out, 2 * rows_extent(n.nlinks, op, ntx), "d_soft_out"};
    if (overlap(in, out)) return fail(QPSK_ERR_ARG, "%s: d_soft_out overlaps d_soft_in", who);
    if (bind(c)) return QPSK_ERR_HIP;
    NodeSyncArgs a = nodesync_args(n);
    a.soft_in = d_soft_in;
    a.in_pitch = ip;
    a.ntx = ntx;
    a.vinfo = d_vinfo;
    a.soft_out = d_soft_out;
    a.out_pitch = op;
    a.info = d_info;
    KERNEL_TRY(launch_nodesync_push(a, n.nlinks, c->stream));
    n.have = (int)std::min<long long>((long long)n.have + ntx, n.nshift - 1);
    c->last_kernel = "nodesync_push_kernel";
    return QPSK_OK;
}
