/*
 * api_coded.cpp -- the coded path's batch calls of the C ABI: soft decisions, the layouts of a coded row (puncturing,
 * interleaving), the convolutional encoders, the Viterbi decoders and the Reed-Solomon outer code.  Holds no state of its
 * own beyond the context's scratch buffers.  The one unit that reads QPSK_VITERBI_PROFILE.
 */
#include "api_ctx.h"

using namespace qpsk;

/* soft decisions and signal quality per row of costas_frame[] (soft.hip; definition in include/qpsk_hip.h).  Rows up to SOFT_ONE_PASS_MAX
 * symbols that need both the sums and the soft output are read once (soft_onepass_kernel); longer rows take sums, then soft */
int qpsk_soft_batch(qpsk_ctx *c, const float *d_costas, long long row_pitch, int nrows, int nsym, int skip, int mode, float scale,
                    const float *d_gain_in, const int32_t *d_lag, const int32_t *d_rot, int first, int nout, int8_t *d_soft,
                    float *d_quality, double *d_sums)
{
    if (!c || !d_costas) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: null context or input");
    if (!d_soft && !d_quality && !d_sums) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: every output is NULL");
    if (nrows <= 0 || nsym <= 0 || nsym > SOFT_MAX_NSYM)
        return fail(QPSK_ERR_ARG, "qpsk_soft_batch: nrows = %d, nsym = %d (1..%d)", nrows, nsym, SOFT_MAX_NSYM);
    if (skip < 0 || skip >= nsym) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: skip = %d outside 0..%d", skip, nsym - 1);
    if (mode != QPSK_SOFT_UNIT && mode != QPSK_SOFT_LLR) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: unknown mode %d", mode);
    if (!(scale > 0.0f && scale <= 3.402823466e+38f)) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: scale = %g is not finite and > 0", (double)scale);
    size_t pitch = 0;
    if (!pitch_ok(row_pitch, nsym, LLONG_MAX, &pitch)) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: row_pitch = %lld (0, or >= nsym %d)", row_pitch, nsym);
    if ((uintptr_t)d_costas % 8) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: d_costas is not 8-byte aligned");
    if (d_soft) {
        if (nout < 0 || first < 0 || (long long)first + nout > nsym)
            return fail(QPSK_ERR_ARG, "qpsk_soft_batch: first %d, nout %d do not fit a row of %d", first, nout, nsym);
        if ((uintptr_t)d_soft % 2) return fail(QPSK_ERR_ARG, "qpsk_soft_batch: d_soft is not 2-byte aligned");
        /* nout = 0 makes d_soft empty; an empty d_soft that points past the input's first byte and not past its last has always been refused */
        const Span in = {d_costas, 8 * rows_extent(nrows, pitch, nsym), "d_costas"}, out = {d_soft, 2 * (size_t)nrows * (size_t)nout, "d_soft"};
        if (overlap(out, in) || (nout == 0 && (const void *)d_soft != d_costas && overlap(Span{d_soft, 1, "d_soft"}, in)))
            return fail(QPSK_ERR_ARG, "qpsk_soft_batch: d_soft overlaps d_costas");
    }
    static_assert(QPSK_SOFT_UNIT == SOFT_MODE_UNIT && QPSK_SOFT_LLR == SOFT_MODE_LLR, "the kernels take the header's mode values");
    if (bind(c)) return QPSK_ERR_HIP;
    const bool need_sums = d_quality || d_sums || !d_gain_in;
    if (!d_soft) {
        KERNEL_TRY(launch_soft_sums(d_costas, pitch, nrows, nsym, skip, mode, scale, nullptr, d_quality, d_sums, c->status.d_status, c->stream));
        c->last_kernel = "soft_sums_kernel";
    } else if (!need_sums) {
        KERNEL_TRY(launch_soft_apply(d_costas, pitch, nrows, nsym, d_gain_in, true, d_lag, d_rot, first, nout, d_soft, c->status.d_status, c->stream));
        c->last_kernel = "soft_apply_kernel";
    } else if (nsym <= SOFT_ONE_PASS_MAX) {
        KERNEL_TRY(launch_soft_onepass(d_costas, pitch, nrows, nsym, skip, mode, scale, d_gain_in, d_lag, d_rot, first, nout, d_soft, d_quality,
                                       d_sums, c->status.d_status, c->stream));
        c->last_kernel = "soft_onepass_kernel";
    } else {
        float *gain = nullptr;
        if (!d_gain_in) {
            if (int rg = ensure(c, c->softgain, sizeof(float) * (size_t)nrows)) return rg;
            gain = (float *)c->softgain.p;
        }
        KERNEL_TRY(launch_soft_sums(d_costas, pitch, nrows, nsym, skip, mode, scale, gain, d_quality, d_sums, c->status.d_status, c->stream));
        KERNEL_TRY(launch_soft_apply(d_costas, pitch, nrows, nsym, d_gain_in ? d_gain_in : gain, d_gain_in != nullptr, d_lag, d_rot, first, nout,
                                     d_soft, c->status.d_status, c->stream));
        c->last_kernel = "soft_sums_kernel + soft_apply_kernel";
    }
    return QPSK_OK;
}

/* PUNCTURING (include/qpsk_hip.h): the pattern of a call, checked; who = the entry point's name */
static int punct_make(const char *who, int period, uint32_t keep0, uint32_t keep1, Puncture *p)
{
    if (period < 1 || period > 32) return fail(QPSK_ERR_ARG, "%s: period = %d outside 1..32", who, period);
    const uint32_t above = period == 32 ? 0u : ~((1u << period) - 1u);
    if ((keep0 | keep1) & above) return fail(QPSK_ERR_ARG, "%s: keep0 = 0x%x / keep1 = 0x%x has a bit at or above period %d", who, keep0, keep1, period);
    if (!(keep0 | keep1)) return fail(QPSK_ERR_ARG, "%s: keep0 and keep1 are both 0: nothing would be sent", who);
    *p = Puncture{period, keep0, keep1, __builtin_popcount(keep0) + __builtin_popcount(keep1)};
    return QPSK_OK;
}

/* INTERLEAVING (include/qpsk_hip.h): the stride of a call over the ntx transmitted dibits of its rows, checked; who = the entry point's name */
static int ilv_make(const char *who, long long ntx, int stride, Interleave *v)
{
    if (ntx < 1) return fail(QPSK_ERR_ARG, "%s: nothing is sent (ntx = 0), so there is nothing to interleave", who);
    const unsigned n = 2u * (unsigned)ntx;
    if (stride < 1 || (unsigned)stride >= std::max(n, 2u)) return fail(QPSK_ERR_ARG, "%s: stride = %d outside 1..%u", who, stride, std::max(n, 2u) - 1);
    if (qpsk_host_gcd((unsigned)stride, n) != 1) return fail(QPSK_ERR_ARG, "%s: stride = %d is not coprime to the row's %u bits", who, stride, n);
    *v = Interleave{n, (unsigned)stride, qpsk_host_mod_inverse((unsigned)stride, n)};
    return QPSK_OK;
}

/* The layout of a call's rows (kernels.h, CodedLayout) is made layer by layer, each layer checked as it is added, and the kind follows the
 * arguments the entry point has, never their values.  An entry point takes the two steps where its own checks have always had them: the
 * pattern first, the stride once nsteps is known to be in range.  NULL adds nothing.
 * layout_add_pattern: a plain *l becomes punctured */
int qpsk::layout_add_pattern(const char *who, const Pattern *pattern, CodedLayout *l)
{
    if (!pattern) return QPSK_OK;
    if (int rc = punct_make(who, pattern->period, pattern->keep0, pattern->keep1, &l->punct)) return rc;
    l->kind = CODED_PUNCT;
    return QPSK_OK;
}
/* layout_add_stride: *l becomes interleaved over the ntx dibits its nsteps steps have on air */
int qpsk::layout_add_stride(const char *who, int nsteps, const int *stride, CodedLayout *l)
{
    if (!stride) return QPSK_OK;
    if (int rc = ilv_make(who, coded_ndibits(*l, nsteps), *stride, &l->ilv)) return rc;
    l->kind = CODED_ILV;
    return QPSK_OK;
}
/* both at once, where nothing lies between them */
static int coded_layout_make(const char *who, int nsteps, const Pattern *pattern, const int *stride, CodedLayout *l)
{
    if (int rc = layout_add_pattern(who, pattern, l)) return rc;
    return layout_add_stride(who, nsteps, stride, l);
}

int qpsk_punct_ntx(int nsteps, int period, uint32_t keep0, uint32_t keep1)
{
    const Pattern pattern = {period, keep0, keep1};
    CodedLayout l;
    if (int rc = layout_add_pattern("qpsk_punct_ntx", &pattern, &l)) return rc;
    if (nsteps < 1 || nsteps > VITERBI_MAX_STEPS) return fail(QPSK_ERR_ARG, "qpsk_punct_ntx: nsteps = %d (1..%d)", nsteps, VITERBI_MAX_STEPS);
    return (int)coded_ndibits(l, nsteps);
}

int qpsk_ilv_stride(int nbits, int want)
{
    if (nbits < 2 || want < 1) return fail(QPSK_ERR_ARG, "qpsk_ilv_stride: nbits = %d (>= 2), want = %d (>= 1)", nbits, want);
    int s = std::min(want, nbits - 1);
    while (qpsk_host_gcd((unsigned)s, (unsigned)nbits) != 1) s++;      /* gcd(nbits - 1, nbits) = 1 ends it */
    return s;
}

/* the K = 7, rate-1/2 convolutional code (viterbi.hip; definition in include/qpsk_hip.h).  The three encoders: who = the entry point's name, the
 * layout from what it takes.  A punctured row of which nothing is sent is no launch; behind a stride coded_layout_make has refused it */
static int conv_encode_impl(qpsk_ctx *c, const char *who, const uint8_t *d_bits, int nrows, int nbits, int flags, const Pattern *pattern,
                            const int *stride, uint8_t *d_dibits)
{
    static const char *const label[] = {"conv_encode_kernel", "conv_encode_punct_kernel", "conv_encode_ilv_kernel"};
    if (!c || !d_bits || !d_dibits) return fail(QPSK_ERR_ARG, "%s: null argument", who);
    if (flags & ~QPSK_CONV_TAIL) return fail(QPSK_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    const int tail = (flags & QPSK_CONV_TAIL) ? 6 : 0;
    if (nrows <= 0 || nbits <= 0 || nbits > VITERBI_MAX_STEPS - tail)
        return fail(QPSK_ERR_ARG, "%s: nrows = %d, nbits = %d (1..%d)", who, nrows, nbits, VITERBI_MAX_STEPS - tail);
    CodedLayout l;
    if (int rc = coded_layout_make(who, nbits + tail, pattern, stride, &l)) return rc;
    if (bind(c)) return QPSK_ERR_HIP;
    if (coded_nsent(l, nbits + tail) == 0) return QPSK_OK;      /* every step of so short a row is deleted: nothing is sent */
    KERNEL_TRY(launch_conv_encode(d_bits, nrows, nbits, nbits + tail, l, d_dibits, c->stream));
    c->last_kernel = label[l.kind];
    return QPSK_OK;
}

int qpsk_conv_encode_batch(qpsk_ctx *c, const uint8_t *d_bits, int nrows, int nbits, int flags, uint8_t *d_dibits)
{
    return conv_encode_impl(c, "qpsk_conv_encode_batch", d_bits, nrows, nbits, flags, nullptr, nullptr, d_dibits);
}

int qpsk_conv_encode_punct_batch(qpsk_ctx *c, const uint8_t *d_bits, int nrows, int nbits, int flags, int period, uint32_t keep0, uint32_t keep1,
                                 uint8_t *d_dibits)
{
    const Pattern pattern = {period, keep0, keep1};
    return conv_encode_impl(c, "qpsk_conv_encode_punct_batch", d_bits, nrows, nbits, flags, &pattern, nullptr, d_dibits);
}

int qpsk_conv_encode_ilv_batch(qpsk_ctx *c, const uint8_t *d_bits, int nrows, int nbits, int flags, int period, uint32_t keep0, uint32_t keep1,
                               int stride, uint8_t *d_dibits)
{
    const Pattern pattern = {period, keep0, keep1};
    return conv_encode_impl(c, "qpsk_conv_encode_ilv_batch", d_bits, nrows, nbits, flags, &pattern, &stride, d_dibits);
}

/* Where the decision words (8 bytes per step) wait for the trace-back: in LDS when a row's fit the launch limit and -- the library's own
 * choice -- every row of the call is resident at once (160 KB of LDS per compute unit), so that the LDS never costs a second round of
 * workgroups; otherwise in the context's scratch buffer, rows in chunks of at most VITERBI_SCRATCH_MAX bytes of it */
static const size_t VITERBI_SCRATCH_MAX = (size_t)1 << 30;

/* the rule for `rows` rows of nsteps steps (api_ctx.h, ViterbiRoute) */
ViterbiRoute qpsk::viterbi_route(const qpsk_ctx *c, size_t rows, int nsteps)
{
    const size_t per_row = viterbi_scratch_bytes_per_row(nsteps);
    const bool fits = per_row <= (size_t)VITERBI_LDS_MAX_BYTES;
    const bool resident = fits && rows <= (size_t)c->ncu * (((size_t)160 << 10) / per_row);
    const bool lds = fits && tuned(c->tune.viterbi_lds, resident ? 1 : 0) != 0;
    size_t cap = std::max<size_t>(1, VITERBI_SCRATCH_MAX / per_row);
    if (!lds && c->tune.viterbi_chunk_rows >= 1) cap = std::min<size_t>(cap, (size_t)c->tune.viterbi_chunk_rows);
    return ViterbiRoute{per_row, lds, std::min<size_t>(rows, cap)};
}

/* the three decoders: who = the entry point's name, the layout from what it takes.  Behind a pattern the rows hold the ntx transmitted dibits
 * of nsteps steps, and row_pitch and d_flip go by ntx.  The pattern is checked first, as the entry points always have; the stride once nsteps
 * is known to be in range */
static int viterbi_impl(qpsk_ctx *c, const char *who, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, const Pattern *pattern,
                        const int *stride, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info)
{
    static const char *const label[][2] = {{"viterbi_kernel", "viterbi_lds_kernel"},
                                           {"viterbi_punct_kernel", "viterbi_punct_lds_kernel"},
                                           {"viterbi_ilv_kernel", "viterbi_ilv_lds_kernel"}};
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context or input", who);
    c->viterbi_launches = 0;      /* a refused call made none */
    CodedLayout l;
    if (int rc = layout_add_pattern(who, pattern, &l)) return rc;
    if (!d_soft) return fail(QPSK_ERR_ARG, "%s: null context or input", who);
    if (!d_bits && !d_info) return fail(QPSK_ERR_ARG, "%s: every output is NULL", who);
    if (nrows <= 0 || nsteps <= 0 || nsteps > VITERBI_MAX_STEPS)
        return fail(QPSK_ERR_ARG, "%s: nrows = %d, nsteps = %d (1..%d)", who, nrows, nsteps, VITERBI_MAX_STEPS);
#ifdef QPSK_VITERBI_PROFILE
    const int known = QPSK_VITERBI_OPEN_START | QPSK_VITERBI_OPEN_END | VITERBI_PROFILE_FORWARD_ONLY | VITERBI_PROFILE_CYCLES;
#else
    const int known = QPSK_VITERBI_OPEN_START | QPSK_VITERBI_OPEN_END;
#endif
    if (flags & ~known) return fail(QPSK_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    const long long nrow = coded_ndibits(l, nsteps);      /* the dibits of a row */
    size_t pitch = 0;
    if (!pitch_ok(row_pitch, nrow, LLONG_MAX, &pitch)) return fail(QPSK_ERR_ARG, "%s: row_pitch = %lld (0, or >= %s %lld)", who, row_pitch, pattern ? "ntx" : "nsteps", nrow);
    if ((uintptr_t)d_soft % 2) return fail(QPSK_ERR_ARG, "%s: d_soft is not 2-byte aligned", who);
    if ((uintptr_t)d_info % 4) return fail(QPSK_ERR_ARG, "%s: d_info is not 4-byte aligned", who);
    if (int rc = layout_add_stride(who, nsteps, stride, &l)) return rc;
    static_assert(QPSK_VITERBI_OPEN_START == VITERBI_OPEN_START && QPSK_VITERBI_OPEN_END == VITERBI_OPEN_END, "the kernel takes the header's flag values");
    if (bind(c)) return QPSK_ERR_HIP;
    const ViterbiRoute route = viterbi_route(c, (size_t)nrows, nsteps);
    /* one launch of rows [r0, r0 + n) */
    const auto launch = [&](size_t r0, int n, unsigned long long *scratch) {
        return launch_viterbi(d_soft + 2 * r0 * pitch, pitch, n, nsteps, l, d_flip, flags, scratch, route.lds,
                              d_bits ? d_bits + r0 * (((size_t)nsteps + 7) / 8) : nullptr, d_info ? d_info + 4 * r0 : nullptr, c->stream);
    };
    if (route.lds) {      /* nothing to chunk for: one launch */
        KERNEL_TRY(launch(0, nrows, nullptr));
        c->viterbi_launches = 1;
    } else {
        if (int rg = ensure(c, c->vitdec, route.chunk_rows * route.per_row)) return rg;
        for (size_t r0 = 0; r0 < (size_t)nrows; r0 += route.chunk_rows) {      /* stream order: a chunk's trace-back is over before the next one's forward pass */
            KERNEL_TRY(launch(r0, (int)std::min<size_t>(route.chunk_rows, (size_t)nrows - r0), (unsigned long long *)c->vitdec.p));
            c->viterbi_launches++;
        }
    }
    c->last_kernel = label[l.kind][route.lds];
    return QPSK_OK;
}

int qpsk_viterbi_batch(qpsk_ctx *c, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, const uint8_t *d_flip, int flags,
                       uint8_t *d_bits, int32_t *d_info)
{
    return viterbi_impl(c, "qpsk_viterbi_batch", d_soft, row_pitch, nrows, nsteps, nullptr, nullptr, d_flip, flags, d_bits, d_info);
}

int qpsk_viterbi_punct_batch(qpsk_ctx *c, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, int period, uint32_t keep0,
                             uint32_t keep1, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info)
{
    const Pattern pattern = {period, keep0, keep1};
    return viterbi_impl(c, "qpsk_viterbi_punct_batch", d_soft, row_pitch, nrows, nsteps, &pattern, nullptr, d_flip, flags, d_bits, d_info);
}

int qpsk_viterbi_ilv_batch(qpsk_ctx *c, const int8_t *d_soft, long long row_pitch, int nrows, int nsteps, int period, uint32_t keep0,
                           uint32_t keep1, int stride, const uint8_t *d_flip, int flags, uint8_t *d_bits, int32_t *d_info)
{
    const Pattern pattern = {period, keep0, keep1};
    return viterbi_impl(c, "qpsk_viterbi_ilv_batch", d_soft, row_pitch, nrows, nsteps, &pattern, &stride, d_flip, flags, d_bits, d_info);
}

/* ------------------------------------------------------------ the Reed-Solomon outer code (REED-SOLOMON in include/qpsk_hip.h) */
int qpsk_rs_generator(int nroots, uint8_t *h_g)
{
    if (!h_g) return fail(QPSK_ERR_ARG, "qpsk_rs_generator: null output");
    if (nroots < 1 || nroots > RS_MAX_ROOTS) return fail(QPSK_ERR_ARG, "qpsk_rs_generator: nroots = %d outside 1..%d", nroots, RS_MAX_ROOTS);
    rs_generator(nroots, h_g);
    return QPSK_OK;
}

int qpsk_rs_encode_batch(qpsk_ctx *c, const uint8_t *d_data, long long data_pitch, int nrows, int k, int nroots, uint8_t *d_out,
                         long long out_pitch)
{
    if (!c || !d_data || !d_out) return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: null context, data or output");
    if (nrows < 1 || k < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || k + nroots > 255)
        return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: nrows = %d, k = %d, nroots = %d (nrows >= 1, k >= 1, 1 <= nroots <= %d, k + nroots <= 255)",
                    nrows, k, nroots, RS_MAX_ROOTS);
    const int n = k + nroots;
    size_t ip = 0, op = 0;
    if (!pitch_ok(data_pitch, k, rs_pitch_limit(nrows), &ip) || !pitch_ok(out_pitch, n, rs_pitch_limit(nrows), &op))
        return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: data_pitch = %lld (0 or >= k = %d), out_pitch = %lld (0 or >= n = %d)", data_pitch, k,
                    out_pitch, n);
    if (overlap(Span{d_data, rows_extent(nrows, ip, k), "d_data"}, Span{d_out, rows_extent(nrows, op, n), "d_out"}))      /* both given, neither empty */
        return fail(QPSK_ERR_ARG, "qpsk_rs_encode_batch: d_out overlaps d_data");
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_rs_encode(d_data, ip, nrows, k, nroots, d_out, op, c->stream));
    c->last_kernel = "rs_encode_kernel";
    return QPSK_OK;
}

int qpsk_rs_decode_batch(qpsk_ctx *c, const uint8_t *d_in, long long in_pitch, int nrows, int n, int nroots, const uint8_t *d_erase,
                         uint8_t *d_out, long long out_pitch, int32_t *d_info)
{
    if (!c || !d_in) return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: null context or input");
    if (!d_out && !d_info) return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_out and d_info are both NULL");
    if (nrows < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || n <= nroots || n > 255)
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: nrows = %d, n = %d, nroots = %d (nrows >= 1, 1 <= nroots <= %d, nroots < n <= 255)", nrows,
                    n, nroots, RS_MAX_ROOTS);
    size_t ip = 0, op = 0;
    if (!pitch_ok(in_pitch, n, rs_pitch_limit(nrows), &ip) || !pitch_ok(out_pitch, n, rs_pitch_limit(nrows), &op))
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: in_pitch = %lld, out_pitch = %lld (each 0 or >= n = %d)", in_pitch, out_pitch, n);
    /* d_erase, d_out and d_info may each be absent, and an absent range overlaps nothing; none is empty */
    const Span in = {d_in, rows_extent(nrows, ip, n), "d_in"}, out = {d_out, rows_extent(nrows, op, n), "d_out"};
    const Span erase = {d_erase, (size_t)nrows * (size_t)n, "d_erase"}, info = {d_info, 16 * (size_t)nrows, "d_info"};
    /* in place: exactly the input rows, each wave reads its whole row before it writes it */
    if (!(d_out == d_in && op == ip) && overlap(in, out))
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_out overlaps d_in (allowed: d_out == d_in with the same pitch)");
    if (overlap(erase, out)) return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_out overlaps d_erase");
    if (((uintptr_t)d_info & 3) || overlap(info, in) || overlap(info, out) || overlap(info, erase))
        return fail(QPSK_ERR_ARG, "qpsk_rs_decode_batch: d_info is not 4-byte aligned, or overlaps d_in, d_out or d_erase");
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_rs_decode(d_in, ip, nrows, n, nroots, d_erase, d_out, op, d_info, c->stream));
    c->last_kernel = "rs_decode_kernel";
    return QPSK_OK;
}

/* test hook (tests/test_viterbi_chunks_gpu.py): host bookkeeping only */
int qpsk_test_viterbi_launches(qpsk_ctx *c, int *out)
{
    if (!c || !out) return fail(QPSK_ERR_ARG, "qpsk_test_viterbi_launches: null argument");
    *out = c->viterbi_launches;
    return QPSK_OK;
}
