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
    /* the new state first: a failed allocation leaves the context, and a node sync it has, as they were */
    if (NODESYNC_STRIDE > SIZE_MAX / (size_t)nlinks || hipMalloc(&n.state, NODESYNC_STRIDE * (size_t)nlinks) != hipSuccess) {
        (void)hipGetLastError();
        return fail(QPSK_ERR_ALLOC, "%s: %d links of %zu bytes of state", who, nlinks, NODESYNC_STRIDE);
    }
    /* pushes of the old node sync may still run */
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        hipFree(n.state);
        return fail(QPSK_ERR_HIP, "%s: hipStreamSynchronize failed", who);
    }
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

/* do [p, p + np) and [q, q + nq) share a byte? */
static bool nodesync_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
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
    if (in_pitch == 0) in_pitch = ntx;
    if (out_pitch == 0) out_pitch = ntx;
    if (in_pitch < ntx || out_pitch < ntx) return fail(QPSK_ERR_ARG, "%s: in_pitch = %lld, out_pitch = %lld (0, or >= ntx %d)", who, in_pitch, out_pitch, ntx);
    if ((uintptr_t)d_soft_in % 2 || (uintptr_t)d_soft_out % 2) return fail(QPSK_ERR_ARG, "%s: d_soft_in or d_soft_out is not 2-byte aligned", who);
    if ((uintptr_t)d_vinfo % 4 || (uintptr_t)d_info % 4) return fail(QPSK_ERR_ARG, "%s: d_vinfo or d_info is not 4-byte aligned", who);
    const size_t L = (size_t)n.nlinks;
    if ((size_t)in_pitch > SIZE_MAX / 4 / L || (size_t)out_pitch > SIZE_MAX / 4 / L) return fail(QPSK_ERR_ARG, "%s: the buffers leave the address space", who);
    /* the bytes the rows span, without what lies behind the last one */
    const size_t in_bytes = 2 * ((L - 1) * (size_t)in_pitch + (size_t)ntx), out_bytes = 2 * ((L - 1) * (size_t)out_pitch + (size_t)ntx);
    if (nodesync_overlap(d_soft_in, in_bytes, d_soft_out, out_bytes)) return fail(QPSK_ERR_ARG, "%s: d_soft_out overlaps d_soft_in", who);
    if (bind(c)) return QPSK_ERR_HIP;
    NodeSyncArgs a = nodesync_args(n);
    a.soft_in = d_soft_in;
    a.in_pitch = (size_t)in_pitch;
    a.ntx = ntx;
    a.vinfo = d_vinfo;
    a.soft_out = d_soft_out;
    a.out_pitch = (size_t)out_pitch;
    a.info = d_info;
    KERNEL_TRY(launch_nodesync_push(a, n.nlinks, c->stream));
    n.have = (int)std::min<long long>((long long)n.have + ntx, n.nshift - 1);
    c->last_kernel = "nodesync_push_kernel";
    return QPSK_OK;
}
