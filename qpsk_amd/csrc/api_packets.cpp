/*
 * api_packets.cpp -- the packet path of the C ABI: the bit stages (CRC, interleaver, scrambler), the stream deframers in their uncoded
 * and coded modes, and the framer.  Owns qpsk_ctx::df and qpsk_ctx::framer.
 */
#include "api_ctx.h"

using namespace qpsk;

/* ------------------------------------------------------------ bit stages */
int qpsk_crc16_batch(qpsk_ctx *c, const uint8_t *d_data, int npackets, int nbytes, uint16_t *d_crc)
{
    if (!c || !d_data || !d_crc) return fail(QPSK_ERR_ARG, "qpsk_crc16_batch: null argument");
    if (npackets <= 0 || nbytes < 0) return fail(QPSK_ERR_ARG, "npackets %d nbytes %d", npackets, nbytes);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_crc16(d_data, npackets, nbytes, d_crc, c->stream));
    return QPSK_OK;
}

int qpsk_interleave_batch(qpsk_ctx *c, uint8_t *d_data, int npackets, int nbytes, int dir)
{
    if (!c || !d_data) return fail(QPSK_ERR_ARG, "qpsk_interleave_batch: null argument");
    if (npackets <= 0 || nbytes <= 0 || nbytes * 8 >= 65536 || (dir != 0 && dir != 1))
        return fail(QPSK_ERR_ARG, "npackets %d, nbytes %d (1..8191), dir %d (0|1)", npackets, nbytes, dir);
    if (bind(c)) return QPSK_ERR_HIP;
    KERNEL_TRY(launch_interleave(d_data, npackets, nbytes, qpsk_host_interleave_prime((unsigned)nbytes * 8u), dir, c->stream));
    return QPSK_OK;
}

int qpsk_scramble_batch(qpsk_ctx *c, uint8_t *d_sym, int npackets, int nsym)
{
    if (!c || !d_sym) return fail(QPSK_ERR_ARG, "qpsk_scramble_batch: null argument");
    if (npackets <= 0 || nsym <= 0) return fail(QPSK_ERR_ARG, "npackets %d nsym %d", npackets, nsym);
    if (bind(c)) return QPSK_ERR_HIP;
    int rc = ensure(c, c->keystream, (size_t)nsym);
    if (rc) return rc;
    if (c->keystream_len != nsym) {
        std::vector<unsigned char> ks((size_t)nsym);
        qpsk_host_scramble_keystream(ks.data(), nsym);
        HIP_TRY(hipMemcpy(c->keystream.p, ks.data(), (size_t)nsym, hipMemcpyHostToDevice));
        c->keystream_len = nsym;
    }
    KERNEL_TRY(launch_scramble(d_sym, (const uint8_t *)c->keystream.p, npackets, nsym, c->stream));
    return QPSK_OK;
}

/* ---------------------------------------------------------------- deframer */
/* no deframer (every reset, qpsk_ctx_destroy): behind a synchronisation of the context's stream */
void Deframer::release()
{
    hipFree(state); hipFree(tables);
    *this = Deframer();
}

static const int DF_ADV_OFFSET = 1040;      /* the tables: keystream bytes [0, nbytes + 2), then 64 uint16 */

/* r x^(8 k) mod the CRC-16 polynomial: k zero bytes through crc16()'s register, starting from r */
static uint16_t crc_shift(unsigned r, int k)
{
    for (int i = 0; i < 8 * k; i++) r = ((r << 1) ^ ((r & 0x8000u) ? 0x1021u : 0u)) & 0xFFFFu;
    return (uint16_t)r;
}
/* x^(8 k) */
static uint16_t crc_advance(int k) { return crc_shift(1u, k); }

static const int DFC_ADV_OFFSET = (DEFRAME_CODED_MAX_STEPS + 15) & ~15;      /* the coded mode's tables: keystream dibits [nsteps], then nbytes uint16 */

/* all four resets: who = the entry point's name; coded: the body is the coded dibits of 8 (nbytes + 2) + 6 trellis steps, held as int8 pairs, in the
 * layout of what the entry point takes.  The pattern is checked first, as the entry points always have; the stride behind everything else */
static int deframer_reset_impl(qpsk_ctx *c, const char *who, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes,
                               int max_packets, bool coded, int mode, float scale, const Pattern *pattern = nullptr, const int *stride = nullptr)
{
    if (!c) return fail(QPSK_ERR_ARG, "%s: null context or sync word", who);
    CodedLayout l;
    if (int rc = layout_add_pattern(who, pattern, &l)) return rc;
    if (!h_sync) return fail(QPSK_ERR_ARG, "%s: null context or sync word", who);
    if (nstreams <= 0) return fail(QPSK_ERR_ARG, "%s: nstreams = %d", who, nstreams);
    if (nsync < 1 || nsync > SYNC_MAX_WORD) return fail(QPSK_ERR_ARG, "%s: nsync = %d outside 1..%d", who, nsync, SYNC_MAX_WORD);
    if (min_score < 1 || min_score > nsync) return fail(QPSK_ERR_ARG, "%s: min_score = %d outside 1..%d", who, min_score, nsync);
    if (nbytes < 1 || nbytes > DEFRAME_MAX_BYTES) return fail(QPSK_ERR_ARG, "%s: nbytes = %d outside 1..%d", who, nbytes, DEFRAME_MAX_BYTES);
    if (max_packets < 1 || max_packets > DEFRAME_MAX_PACKETS)
        return fail(QPSK_ERR_ARG, "%s: max_packets = %d outside 1..%d", who, max_packets, DEFRAME_MAX_PACKETS);
    for (int i = 0; i < nsync; i++)
        if (h_sync[i] > 3) return fail(QPSK_ERR_ARG, "%s: sync[%d] = %d is not a dibit", who, i, (int)h_sync[i]);
    if (coded && mode != QPSK_SOFT_UNIT && mode != QPSK_SOFT_LLR) return fail(QPSK_ERR_ARG, "%s: unknown mode %d", who, mode);
    if (coded && !(scale > 0.0f && scale <= 3.402823466e+38f)) return fail(QPSK_ERR_ARG, "%s: scale = %g is not finite and > 0", who, (double)scale);
    const int nb = nbytes + 2, nsteps = 8 * nb + 6;
    /* dibits of a body: a punctured one is shorter than 8 nb + 6, so the pending buffer and the keystream table's bound hold as they are.
     * K >= 1 sent bit per period and nsteps > 32 >= period: at least one dibit */
    const int N = coded ? (int)coded_ndibits(l, nsteps) : 4 * nb;
    if (int rc = layout_add_stride(who, nsteps, stride, &l)) return rc;      /* a bad stride resets nothing */
    if (bind(c)) return QPSK_ERR_HIP;
    /* refused until this call has completed */
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->df.release();
    Deframer d;      /* the new deframer's books: the context's once everything below has completed */
    const size_t state_stride = (size_t)DEFRAME_PEND_OFFSET + (((size_t)N * (coded ? 2 : 1) + 15) & ~(size_t)15);
    const size_t tab_bytes = coded ? (size_t)DFC_ADV_OFFSET + 2 * (size_t)DEFRAME_MAX_BYTES : (size_t)DF_ADV_OFFSET + 128;
    if (hipMalloc(&c->df.state, state_stride * (size_t)nstreams) != hipSuccess || hipMalloc(&c->df.tables, tab_bytes) != hipSuccess) {
        c->df.release();
        (void)hipGetLastError();
        return fail(QPSK_ERR_ALLOC, "%s: %d streams of %zu bytes of state", who, nstreams, state_stride);
    }
    std::vector<unsigned char> ks((size_t)N);
    qpsk_host_scramble_keystream(ks.data(), N);
    std::vector<uint8_t> tab(tab_bytes, 0);
    if (coded) {
        memcpy(tab.data(), ks.data(), (size_t)N);
        uint16_t adv = 1;                                               /* x^(8 m), m = 0 .. nbytes - 1, a byte at a time */
        for (int m = 0; m < nbytes; m++, adv = crc_shift(adv, 1)) memcpy(&tab[DFC_ADV_OFFSET + 2 * m], &adv, 2);
        d.crc_init = crc_shift(0xFFFFu, nbytes);
    } else {
        for (int k = 0; k < nb; k++) tab[k] = (uint8_t)(ks[4 * k] | ks[4 * k + 1] << 2 | ks[4 * k + 2] << 4 | ks[4 * k + 3] << 6);
        const int per = (nb + 63) / 64;
        for (int l = 0; l < 64; l++) {
            const int end = (l + 1) * per < nbytes ? (l + 1) * per : nbytes;
            const uint16_t v = crc_advance(nbytes - end);
            memcpy(&tab[DF_ADV_OFFSET + 2 * l], &v, 2);
        }
    }
    for (int i = 0; i < nsync; i++) {
        const unsigned r = h_sync[i] ^ (h_sync[i] >> 1);
        if (r & 1u) d.sync_lo[i >> 6] |= 1ull << (i & 63);
        if (r & 2u) d.sync_hi[i >> 6] |= 1ull << (i & 63);
    }
    HIP_TRY(hipMemsetAsync(c->df.state, 0, state_stride * (size_t)nstreams, c->stream));
    HIP_TRY(hipMemcpyAsync(c->df.tables, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    d.state = c->df.state;      /* (allocated into the context, so that a failure above leaves them to the next reset) */
    d.tables = c->df.tables;
    d.stride = state_stride;
    d.nstreams = nstreams;
    d.nsync = nsync;
    d.min_score = min_score;
    d.nbytes = nbytes;
    d.max_packets = max_packets;
    d.coded = coded;
    d.mode = mode;
    d.scale = scale;
    d.nsteps = coded ? nsteps : 0;
    d.nbody = coded ? N : 0;
    d.layout = l;
    d.ready = true;
    c->df = d;
    return QPSK_OK;
}

int qpsk_deframer_reset(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets)
{
    return deframer_reset_impl(c, "qpsk_deframer_reset", nstreams, h_sync, nsync, min_score, nbytes, max_packets, false, 0, 1.0f);
}

int qpsk_deframer_reset_coded(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets,
                              int mode, float scale)
{
    return deframer_reset_impl(c, "qpsk_deframer_reset_coded", nstreams, h_sync, nsync, min_score, nbytes, max_packets, true, mode, scale);
}

/* the coded mode behind a puncturing pattern: the body is the ntx(8 (nbytes + 2) + 6) transmitted dibits; the pattern lives in the
 * deframer's state, and qpsk_deframer_push_coded decodes with the punctured kernels */
int qpsk_deframer_reset_coded_punct(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets,
                                    int mode, float scale, int period, uint32_t keep0, uint32_t keep1)
{
    const Pattern pattern = {period, keep0, keep1};
    return deframer_reset_impl(c, "qpsk_deframer_reset_coded_punct", nstreams, h_sync, nsync, min_score, nbytes, max_packets, true, mode, scale, &pattern);
}

/* the same behind a stride of INTERLEAVING as well: the body is as long, its bits lie at pi(k) on air, and qpsk_deframer_push_coded decodes
 * with the interleaved kernels */
int qpsk_deframer_reset_coded_ilv(qpsk_ctx *c, int nstreams, const uint8_t *h_sync, int nsync, int min_score, int nbytes, int max_packets,
                                  int mode, float scale, int period, uint32_t keep0, uint32_t keep1, int stride)
{
    const Pattern pattern = {period, keep0, keep1};
    return deframer_reset_impl(c, "qpsk_deframer_reset_coded_ilv", nstreams, h_sync, nsync, min_score, nbytes, max_packets, true, mode, scale,
                               &pattern, &stride);
}

/* what both pushes do behind their own argument checks (who = the entry point's name): the state checks, no output (the caller's
 * list; absent ones overlap nothing) may overlap the input of sym_bytes a symbol, the device, and the hunt's arguments from the context */
static int deframer_push_begin(qpsk_ctx *c, const char *who, bool coded, const void *in, size_t sym_bytes, int nsym,
                               std::initializer_list<Span> outs, DeframeHuntArgs &a)
{
    if (!c->df.state) return fail(QPSK_ERR_STATE, "%s: no %s yet", who, coded ? "qpsk_deframer_reset_coded" : "qpsk_deframer_reset");
    if (c->df.coded != coded)
        return fail(QPSK_ERR_STATE, "%s: the deframer was reset in %s mode (%s)", who, coded ? "uncoded" : "coded",
                    coded ? "qpsk_deframer_push" : "qpsk_deframer_push_coded");
    if (!c->df.ready) return fail(QPSK_ERR_STATE, "%s: the deframer's state is undefined after a failed push; reset it", who);
    /* no range is empty: the input is given and nsym >= 1, and behind a reset nstreams, max_packets and nbytes are all >= 1 */
    const Span input = {in, (size_t)c->df.nstreams * (size_t)nsym * sym_bytes, "the input"};
    for (const Span &o : outs)
        if (overlap(o, input)) return fail(QPSK_ERR_ARG, "%s: %s overlaps the input", who, o.name);
    if (bind(c)) return QPSK_ERR_HIP;
    a.nstreams = c->df.nstreams;
    a.nsym = nsym;
    a.nsync = c->df.nsync;
    a.min_score = c->df.min_score;
    a.state = c->df.state;
    a.state_stride = c->df.stride;
    for (int i = 0; i < 2; i++) { a.sync_lo[i] = c->df.sync_lo[i]; a.sync_hi[i] = c->df.sync_hi[i]; }
    return QPSK_OK;
}

int qpsk_deframer_push(qpsk_ctx *c, const float *d_costas, const uint8_t *d_data, int nsym, int32_t *d_count, uint8_t *d_bytes,
                       long long *d_pos, int32_t *d_rot, int32_t *d_score, uint8_t *d_crc_ok)
{
    if (!c) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: null context");
    if ((d_costas != nullptr) == (d_data != nullptr)) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: give exactly one of d_costas, d_data");
    if (!d_count) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: d_count is required");
    if (nsym < 1 || nsym > DEFRAME_MAX_NSYM) return fail(QPSK_ERR_ARG, "qpsk_deframer_push: nsym = %d outside 1..%d", nsym, DEFRAME_MAX_NSYM);
    const size_t S = (size_t)c->df.nstreams, M = (size_t)c->df.max_packets;
    DeframeArgs a{};
    if (int rc = deframer_push_begin(c, "qpsk_deframer_push", false, d_costas ? (const void *)d_costas : (const void *)d_data,
                                     d_costas ? 2 * sizeof(float) : 1, nsym,
                                     {{d_count, S * 4, "d_count"}, {d_bytes, S * M * (size_t)(c->df.nbytes + 2), "d_bytes"}, {d_pos, S * M * 8, "d_pos"},
                                      {d_rot, S * M * 4, "d_rot"}, {d_score, S * M * 4, "d_score"}, {d_crc_ok, S * M, "d_crc_ok"}}, a))
        return rc;
    a.data = d_data;
    a.costas = reinterpret_cast<const float2 *>(d_costas);
    a.nbytes = c->df.nbytes;
    a.max_packets = c->df.max_packets;
    a.bytes_per_lane = (c->df.nbytes + 2 + 63) / 64;
    a.keystream = c->df.tables;
    a.crc_adv = reinterpret_cast<const uint16_t *>(c->df.tables + DF_ADV_OFFSET);
    a.count = d_count;
    a.bytes = d_bytes;
    a.pos = d_pos;
    a.rot = d_rot;
    a.score = d_score;
    a.crc_ok = d_crc_ok;
    (void)hipGetLastError();
    const int e = launch_deframe(a, c->stream);
    if (e != 0) {
        c->df.ready = false;
        return fail(QPSK_ERR_HIP, "deframe_kernel launch: %s", hipGetErrorString((hipError_t)e));
    }
    c->last_kernel = "deframe_kernel";
    return QPSK_OK;
}

/* the coded mode's push (deframe_coded.hip): [the row's gain, unless the caller gives one] -> hunt + soft rows -> decode.  Everything that can
 * fail without a launch -- arguments, the three buffers -- comes before the first launch */
int qpsk_deframer_push_coded(qpsk_ctx *c, const float *d_costas, int nsym, const float *d_gain, int32_t *d_count, uint8_t *d_bytes,
                             long long *d_pos, int32_t *d_rot, int32_t *d_score, uint8_t *d_crc_ok, int32_t *d_info)
{
    if (!c) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: null context");
    c->viterbi_launches = 0;      /* a refused call made none */
    if (!d_costas) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: d_costas is required");
    if (!d_count) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: d_count is required");
    if (nsym < 1 || nsym > DEFRAME_MAX_NSYM) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: nsym = %d outside 1..%d", nsym, DEFRAME_MAX_NSYM);
    if ((uintptr_t)d_costas % 8) return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: d_costas is not 8-byte aligned");
    if ((uintptr_t)d_gain % 4 || (uintptr_t)d_count % 4 || (uintptr_t)d_rot % 4 || (uintptr_t)d_score % 4 || (uintptr_t)d_info % 4 || (uintptr_t)d_pos % 8)
        return fail(QPSK_ERR_ARG, "qpsk_deframer_push_coded: a misaligned array");
    const size_t S = (size_t)c->df.nstreams, M = (size_t)c->df.max_packets;
    DeframeCodedArgs a{};
    if (int rc = deframer_push_begin(c, "qpsk_deframer_push_coded", true, d_costas, 2 * sizeof(float), nsym,
                                     {{d_count, S * 4, "d_count"}, {d_bytes, S * M * (size_t)(c->df.nbytes + 2), "d_bytes"}, {d_pos, S * M * 8, "d_pos"},
                                      {d_rot, S * M * 4, "d_rot"}, {d_score, S * M * 4, "d_score"}, {d_crc_ok, S * M, "d_crc_ok"},
                                      {d_info, S * M * 16, "d_info"}}, a))
        return rc;
    const int Nc = c->df.nbody, pitch = (Nc + 1) & ~1;      /* the staging rows go by what is on air, the decision words by the steps */
    const int per = std::min<long long>(c->df.max_packets, (long long)nsym / (c->df.nsync + Nc) + 1);
    const size_t rows = S * (size_t)per;
    const bool decode = d_bytes || d_crc_ok || d_info;
    const ViterbiRoute route = viterbi_route(c, rows, c->df.nsteps);
    if (int rg = ensure(c, c->dfstage, rows * 2 * (size_t)pitch)) return rg;
    if (!d_gain)
        if (int rg = ensure(c, c->softgain, sizeof(float) * S)) return rg;
    if (decode && !route.lds)
        if (int rg = ensure(c, c->vitdec, route.chunk_rows * route.per_row)) return rg;

    a.costas = reinterpret_cast<const float2 *>(d_costas);
    a.gain = d_gain ? d_gain : (const float *)c->softgain.p;
    a.check_gain = d_gain != nullptr;
    a.nbytes = c->df.nbytes;
    a.max_packets = c->df.max_packets;
    a.nsteps = c->df.nsteps;
    a.per_stream = per;
    a.stage = (int8_t *)c->dfstage.p;
    a.flip = c->df.tables;
    a.crc_adv = reinterpret_cast<const uint16_t *>(c->df.tables + DFC_ADV_OFFSET);
    a.crc_init = c->df.crc_init;
    a.count = d_count;
    a.bytes = d_bytes;
    a.pos = d_pos;
    a.rot = d_rot;
    a.score = d_score;
    a.crc_ok = d_crc_ok;
    a.info = d_info;
    a.status = c->status.d_status;
    (void)hipGetLastError();
    if (!d_gain)      /* nothing of the deframer's has run yet: a failure here leaves its state as it was */
        KERNEL_TRY(launch_soft_sums(d_costas, (size_t)nsym, c->df.nstreams, nsym, 0, c->df.mode, c->df.scale, (float *)c->softgain.p, nullptr, nullptr,
                                    c->status.d_status, c->stream));
    const DeframeCodedBody body = {Nc, pitch};      /* the decode's launch adds the layout */
    int e = launch_deframe_coded_hunt(a, body, c->stream);
    for (size_t r0 = 0; e == 0 && decode && r0 < rows; r0 += route.chunk_rows) {      /* stream order: a chunk's trace-back is over before the next one's forward pass */
        const int n = (int)std::min<size_t>(route.chunk_rows, rows - r0);
        e = launch_deframe_coded_decode(a, body, c->df.layout, (int)r0, n, route.lds ? nullptr : (unsigned long long *)c->vitdec.p, route.lds, c->stream);
        if (e == 0) c->viterbi_launches++;
    }
    if (e != 0) {
        c->df.ready = false;
        return fail(QPSK_ERR_HIP, "qpsk_deframer_push_coded launch: %s", hipGetErrorString((hipError_t)e));
    }
    static const char *const label[][2] = {
        {"deframe_coded_hunt_kernel + deframe_coded_decode_kernel<global>", "deframe_coded_hunt_kernel + deframe_coded_decode_kernel<lds>"},
        {"deframe_coded_hunt_kernel + deframe_coded_decode_punct_kernel<global>", "deframe_coded_hunt_kernel + deframe_coded_decode_punct_kernel<lds>"},
        {"deframe_coded_hunt_kernel + deframe_coded_decode_ilv_kernel<global>", "deframe_coded_hunt_kernel + deframe_coded_decode_ilv_kernel<lds>"}};
    c->last_kernel = decode ? label[c->df.layout.kind][route.lds] : "deframe_coded_hunt_kernel";
    return QPSK_OK;
}


/* ------------------------------------------------------------------ framer */
void Framer::release()
{
    hipFree(ks);
    *this = Framer();
}

/* FRAMER (include/qpsk_hip.h): the dibits of a body on air, B; who = the entry point's name.  The pattern is looked at only when coded */
static int frame_body(const char *who, int nbytes, int coding, const Pattern &pattern, CodedLayout *l, int *nbody)
{
    if (nbytes < 1 || nbytes > FRAME_MAX_BYTES) return fail(QPSK_ERR_ARG, "%s: nbytes = %d outside 1..%d", who, nbytes, FRAME_MAX_BYTES);
    if (coding != QPSK_FRAME_UNCODED && coding != QPSK_FRAME_CODED) return fail(QPSK_ERR_ARG, "%s: unknown coding %d", who, coding);
    if (coding == QPSK_FRAME_UNCODED) {
        *nbody = 4 * (nbytes + 2);
        return QPSK_OK;
    }
    if (int rc = layout_add_pattern(who, &pattern, l)) return rc;
    /* K >= 1 sent bit per period and 8 (nbytes + 2) + 6 > 32 >= period steps: at least one dibit */
    *nbody = (int)coded_ndibits(*l, 8 * (nbytes + 2) + 6);
    return QPSK_OK;
}

int qpsk_frame_len(int nsync, int nbytes, int coding, int period, uint32_t keep0, uint32_t keep1)
{
    if (nsync < 1 || nsync > SYNC_MAX_WORD) return fail(QPSK_ERR_ARG, "qpsk_frame_len: nsync = %d outside 1..%d", nsync, SYNC_MAX_WORD);
    CodedLayout l;
    int nbody = 0;
    if (int rc = frame_body("qpsk_frame_len", nbytes, coding, Pattern{period, keep0, keep1}, &l, &nbody)) return rc;
    return nsync + nbody;
}

/* The framer's keystream table holds at least n dibits.  It grows into a NEW buffer, filled by a blocking copy before anything can read it;
 * the old one is freed only behind a synchronisation of the context's stream, the one stream every launch that reads it was enqueued on
 * (qpsk_ctx_set_stream synchronises the stream it leaves), so no enqueued launch still reads a table that is freed.  A failed allocation
 * leaves the old table, and the context, as they were */
static int frame_keystream(qpsk_ctx *c, int n)
{
    if (c->framer.ks_len >= n) return QPSK_OK;
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(QPSK_ERR_ALLOC, "qpsk_frame_batch: hipMalloc(%d bytes of keystream): %s", n, hipGetErrorString(e));
    }
    std::vector<unsigned char> ks((size_t)n);
    qpsk_host_scramble_keystream(ks.data(), n);
    hipError_t e2 = hipMemcpy(p, ks.data(), (size_t)n, hipMemcpyHostToDevice);
    if (e2 == hipSuccess && c->framer.ks) e2 = hipStreamSynchronize(c->stream);
    if (e2 != hipSuccess) {
        hipFree(p);
        return fail(QPSK_ERR_HIP, "qpsk_frame_batch: keystream upload: %s", hipGetErrorString(e2));
    }
    hipFree(c->framer.ks);
    c->framer.ks = (uint8_t *)p;
    c->framer.ks_len = n;
    return QPSK_OK;
}

/* both framers: who = the entry point's name; stride = NULL for qpsk_frame_batch */
static int frame_impl(qpsk_ctx *c, const char *who, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                      const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, const int *stride, int lead, int gap,
                      int row_len, uint8_t *d_out, uint16_t *d_crc)
{
    if (!c || !d_payload || !h_sync || !d_out) return fail(QPSK_ERR_ARG, "%s: null context, payload, sync word or output", who);
    if (nsync < 1 || nsync > SYNC_MAX_WORD) return fail(QPSK_ERR_ARG, "%s: nsync = %d outside 1..%d", who, nsync, SYNC_MAX_WORD);
    CodedLayout l;      /* coded: behind the pattern; the uncoded format has no layout */
    int nbody = 0;
    if (int rc = frame_body(who, nbytes, coding, Pattern{period, keep0, keep1}, &l, &nbody)) return rc;
    if (nrows < 1 || per_row < 1 || per_row > FRAME_MAX_PER_ROW || (long long)nrows * per_row > INT_MAX)
        return fail(QPSK_ERR_ARG, "%s: nrows = %d, per_row = %d (1..%d, nrows * per_row < 2^31)", who, nrows, per_row, FRAME_MAX_PER_ROW);
    size_t pitch = 0;
    if (!pitch_ok(payload_pitch, nbytes, LLONG_MAX, &pitch)) return fail(QPSK_ERR_ARG, "%s: payload_pitch = %lld below nbytes = %d", who, payload_pitch, nbytes);
    if (lead < 0 || gap < 0) return fail(QPSK_ERR_ARG, "%s: lead = %d, gap = %d", who, lead, gap);
    const long long need = (long long)lead + (long long)per_row * (nsync + nbody) + (long long)(per_row - 1) * gap;
    if (row_len < 1 || row_len > FRAME_MAX_ROW || need > row_len)
        return fail(QPSK_ERR_ARG, "%s: lead %d + %d packets of %d dibits + gaps of %d = %lld do not fit row_len = %d (up to %d)", who, lead,
                    per_row, nsync + nbody, gap, need, row_len, FRAME_MAX_ROW);
    /* d_payload and d_out are given and no range is empty (nrows, per_row, nbytes, row_len >= 1); d_crc may be absent */
    const size_t npk = (size_t)nrows * (size_t)per_row;
    const Span in = {d_payload, rows_extent((long long)npk, pitch, nbytes), "d_payload"}, out = {d_out, (size_t)nrows * (size_t)row_len, "d_out"};
    const Span crc = {d_crc, 2 * npk, "d_crc"};
    if (overlap(out, in)) return fail(QPSK_ERR_ARG, "%s: d_out overlaps d_payload", who);
    if (((uintptr_t)d_crc & 1) || overlap(crc, in) || overlap(crc, out))
        return fail(QPSK_ERR_ARG, "%s: d_crc is not 2-byte aligned, or overlaps d_payload or d_out", who);
    /* the stride: the uncoded format has none; 1 is no interleaving at all and, here alone, takes the kernel of the layer below, frame_kernel<coded> */
    if (stride && coding == QPSK_FRAME_UNCODED && *stride != 1) return fail(QPSK_ERR_ARG, "%s: stride = %d with QPSK_FRAME_UNCODED (1 only)", who, *stride);
    if (stride && coding == QPSK_FRAME_CODED) {
        if (int rc = layout_add_stride(who, 8 * (nbytes + 2) + 6, stride, &l)) return rc;
        if (l.ilv.s == 1) l.kind = CODED_PUNCT;
    }
    if (bind(c)) return QPSK_ERR_HIP;
    if (int rc = frame_keystream(c, row_len > nbody ? row_len : nbody)) return rc;
    FrameArgs a{};
    a.payload = d_payload;
    a.pitch = pitch;
    a.out = d_out;
    a.crc = d_crc;
    a.ks = c->framer.ks;
    a.npackets = (int)npk;
    a.per_row = per_row;
    a.nbytes = nbytes;
    a.nsync = nsync;
    a.nbody = nbody;
    a.lead = lead;
    a.gap = gap;
    a.row_len = row_len;
    a.bytes_per_lane = (nbytes + 63) / 64;
    a.coded = coding == QPSK_FRAME_CODED;
    /* lane l's share of the CRC covers payload bytes [l c, min((l + 1) c, nbytes)): x^(8 k), k = the bytes behind them; then the init value's */
    uint16_t adv[65];
    for (int l = 0; l < 64; l++) {
        const int end = (l + 1) * a.bytes_per_lane < nbytes ? (l + 1) * a.bytes_per_lane : nbytes;
        adv[l] = crc_advance(nbytes - end);
    }
    adv[64] = crc_shift(0xFFFFu, nbytes);
    KERNEL_TRY(launch_frame(a, l, h_sync, adv, c->stream));
    c->last_kernel = !a.coded ? "frame_kernel<uncoded>" : l.kind == CODED_ILV ? "frame_kernel<coded,ilv>" : "frame_kernel<coded>";
    return QPSK_OK;
}

int qpsk_frame_batch(qpsk_ctx *c, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                     const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, int lead, int gap,
                     int row_len, uint8_t *d_out, uint16_t *d_crc)
{
    return frame_impl(c, "qpsk_frame_batch", d_payload, payload_pitch, nrows, per_row, nbytes, h_sync, nsync, coding, period, keep0, keep1, nullptr,
                      lead, gap, row_len, d_out, d_crc);
}

int qpsk_frame_batch_ilv(qpsk_ctx *c, const uint8_t *d_payload, long long payload_pitch, int nrows, int per_row, int nbytes,
                         const uint8_t *h_sync, int nsync, int coding, int period, uint32_t keep0, uint32_t keep1, int stride, int lead, int gap,
                         int row_len, uint8_t *d_out, uint16_t *d_crc)
{
    return frame_impl(c, "qpsk_frame_batch_ilv", d_payload, payload_pitch, nrows, per_row, nbytes, h_sync, nsync, coding, period, keep0, keep1,
                      &stride, lead, gap, row_len, d_out, d_crc);
}

/* test hook (tests/test_deframe_positions_gpu.py): the stream positions of both deframers move on by delta, as if delta more dibits had
 * been pushed whose words and packets all lay behind the carried tail.  Plain copies of the headers, no kernel */
int qpsk_test_deframer_advance(qpsk_ctx *c, long long delta)
{
    if (!c) return fail(QPSK_ERR_ARG, "qpsk_test_deframer_advance: null context");
    if (delta < 0 || delta > (1LL << 62)) return fail(QPSK_ERR_ARG, "qpsk_test_deframer_advance: delta = %lld outside 0..2^62", delta);
    if (!c->df.state) return fail(QPSK_ERR_STATE, "qpsk_test_deframer_advance: no deframer reset yet");
    if (!c->df.ready) return fail(QPSK_ERR_STATE, "qpsk_test_deframer_advance: the deframer's state is undefined after a failed push; reset it");
    if (bind(c)) return QPSK_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t S = (size_t)c->df.nstreams;
    std::vector<DeframeHeader> hd(S);
    HIP_TRY(hipMemcpy2D(hd.data(), sizeof(DeframeHeader), c->df.state, c->df.stride, sizeof(DeframeHeader), S, hipMemcpyDeviceToHost));
    for (const auto &h : hd) {
        if (h.len < (long long)c->df.nsync - 1)      /* the hunt takes a tail of nsync - 1 dibits for granted once len says so */
            return fail(QPSK_ERR_STATE, "qpsk_test_deframer_advance: a stream has seen %lld dibits, fewer than nsync - 1 = %d", h.len, c->df.nsync - 1);
        if (h.len > LLONG_MAX - delta - (1LL << 32))
            return fail(QPSK_ERR_ARG, "qpsk_test_deframer_advance: the positions would leave 64 bits");
    }
    for (auto &h : hd) { h.len += delta; h.h += delta; h.ppos += delta; }
    HIP_TRY(hipMemcpy2D(c->df.state, c->df.stride, hd.data(), sizeof(DeframeHeader), sizeof(DeframeHeader), S, hipMemcpyHostToDevice));
    return QPSK_OK;
}
