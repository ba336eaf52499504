/*
 * deframe_coded.hip -- convolutionally coded packets out of continuous streams of costas_frame[] (include/qpsk_hip.h,
 * qpsk_deframer_push_coded): deframe_hunt.h's hunt with soft decisions where deframe.hip builds bytes, and viterbi.hip's decoder on the
 * packets the hunt completes.
 *
 *   deframe_coded_hunt_kernel     one wave per stream: the hunt of deframe_hunt.h (X, the bit planes, the wave-uniform walk over the
 *                                 candidate masks, the carried tail are described there) with the policy SoftPackets.  The body of a
 *                                 packet is Nc = nbody dibits (8 (nbytes + 2) + 6 at rate 1/2, fewer behind a puncturing pattern: the hunt
 *                                 only takes the number); the lanes quantise the body symbols that lie in this push's row (soft_quant.h:
 *                                 the turn by the packet's rotation and q(x) of qpsk_soft_batch, with this push's gain) lane-parallel,
 *                                 8-byte loads and 2-byte stores, into the packet's soft row.  An incomplete packet's row is the stream's
 *                                 pending buffer (int8 pairs: no float history is carried, every body symbol arrives in the push that
 *                                 completes the sync word or a later one).  A packet completed in this push with output row
 *                                 slot < max_packets gets staging row stream * per_stream + slot: the pending pairs are copied there, the
 *                                 rest is quantised into it, and pos / rot / score are written here.  The hunt never looks at a decoder's
 *                                 result.
 *   deframe_coded_decode_kernel   one wave per staging row; rows at or beyond the stream's count retire at once.  viterbi_row.h's forward
 *                                 pass and trace-back with the keystream as flip and flags 0; the trace-back hands every 64 decoded bits
 *                                 to PacketSink: lanes 0..7 take one byte each, store it (bytes below nbytes + 2) and add its share of the
 *                                 CRC -- crc16() is linear, byte k of nbytes contributes crc_byte(b) x^(8 (nbytes - 1 - k)), the factors
 *                                 come from a table -- and a wave xor behind the trace-back sums the shares.  One template, <LDS, KIND>,
 *                                 KIND = the kind of the deframer's CodedLayout (kernels.h), which picks viterbi_row.h's loader:
 *                                 CODED_PUNCT (qpsk_deframer_reset_coded_punct) decodes the Nc staged dibits as nsteps = 8 (nbytes + 2) + 6
 *                                 trellis steps, the keystream flipping the transmitted dibits; CODED_ILV (qpsk_deframer_reset_coded_ilv)
 *                                 is the same behind the stride's position map: the staged row is the body as it was on air, and the
 *                                 loader reads sent bit k and its keystream bit at pi(k).  The hunt is the same for all three: it only
 *                                 takes the body's length.
 *
 * A staging row is addressed by (stream, slot), the packet's place in the outputs, so there is no list to append to and no atomic:
 * per_stream = min(max_packets, nsym / (nsync + Nc) + 1) bounds what one push can complete in a stream (packet ends lie nsync + Nc
 * apart), and the decode grid covers nstreams * per_stream rows.  Staging rows lie stage_pitch = Nc rounded up to even dibits apart, so
 * that copy_pairs' 4-byte accesses stay aligned when a punctured Nc is odd.  Vector stores only.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "qpsk_device.h"
#include "deframe_bits.h"
#include "deframe_hunt.h"
#include "soft_quant.h"
#include "viterbi_row.h"

namespace qpsk {

namespace {

/* cnt body symbols from src, turned by r and quantised with g, as int8 pairs to dst (2-byte aligned); returns whether one was NaN / Inf */
__device__ __forceinline__ bool quantise_body(const float2 *__restrict__ src, int cnt, int r, float g, int8_t *__restrict__ dst, int lane)
{
    bool bad = false;
#pragma unroll 1
    for (int i0 = 0; i0 < cnt; i0 += 64) {      /* a wave-uniform trip count: the loop's control stays on the scalar unit */
        const int i = i0 + lane;
        if (i < cnt) *reinterpret_cast<unsigned short *>(dst + 2 * (size_t)i) = (unsigned short)soft_pair(src[i], r, g, bad);
    }
    return bad;
}

/* the pending buffer's first `have` pairs into a staging row (both 4-byte aligned) */
__device__ __forceinline__ void copy_pairs(const int8_t *__restrict__ src, int have, int8_t *__restrict__ dst, int lane)
{
#pragma unroll 1
    for (int i0 = 0; i0 < (have >> 1); i0 += 64) {
        const int i = i0 + lane;
        if (i < (have >> 1)) reinterpret_cast<unsigned *>(dst)[i] = reinterpret_cast<const unsigned *>(src)[i];
    }
    if ((have & 1) && lane == 0) reinterpret_cast<unsigned short *>(dst)[have - 1] = reinterpret_cast<const unsigned short *>(src)[have - 1];
}

/* the hunt's policy: packets as soft rows in the staging buffer, the pending body as int8 pairs */
struct SoftPackets {
    const DeframeCodedArgs &a;
    int stream, nbody, stage_pitch;
    const float2 *row;
    int8_t *pend;
    float g;
    bool bad;                     /* a NaN / Inf gain, or body sample among those quantised */
    __device__ __forceinline__ unsigned ring(long long i) const { return ring_at(row, i); }
    __device__ __forceinline__ void complete(int slot, long long pos, int rot, int score, int have, int row0)
    {
        const int lane = threadIdx.x & 63;
        int8_t *dst = a.stage + 2 * ((size_t)stream * a.per_stream + slot) * (size_t)stage_pitch;
        if (have > 0) copy_pairs(pend, have, dst, lane);
        bad |= quantise_body(row + row0, nbody - have, rot, g, dst + 2 * (size_t)have, lane);
        report(a, (size_t)stream * a.max_packets + slot, pos, rot, score, lane);
    }
    __device__ __forceinline__ void collect(int have, int row0, int cnt, int rot)
    {
        bad |= quantise_body(row + row0, cnt, rot, g, pend + 2 * (size_t)have, threadIdx.x & 63);
    }
};

__global__ void __launch_bounds__(64 * HUNT_WAVES)
deframe_coded_hunt_kernel(DeframeCodedArgs a, int nbody, int stage_pitch)
{
    const int stream = blockIdx.x * HUNT_WAVES + (int)(threadIdx.x >> 6);
    if (stream >= a.nstreams) return;
    uint8_t *st = a.state + (size_t)stream * a.state_stride;
    const float g = a.gain[stream];
    SoftPackets p = {a, stream, nbody, stage_pitch, a.costas + (size_t)stream * (size_t)a.nsym, reinterpret_cast<int8_t *>(st + DEFRAME_PEND_OFFSET),
                     g, a.check_gain && !finite_f(g)};
    deframe_hunt(a, stream, nbody, a.per_stream, st, p);
    if (__builtin_expect(p.bad, 0) && a.status) __hip_atomic_store(a.status, STATUS_SOFT_NONFINITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

/* the trace-back's sink: the packet's first nbytes + 2 bytes and the lanes' shares of its CRC (low half: crc16 of the payload without the
 * register's start value; high half: the received CRC) */
struct PacketSink {
    uint8_t *out;             /* this packet's nbytes + 2 bytes, or NULL */
    const uint16_t *adv;
    int nbytes;
    unsigned share;
    /* n (the block's steps) is not needed: Nc = 8 (nbytes + 2) + 6, so every byte below nbytes + 2 is whole and k < nbytes + 2 alone
     * leaves the six tail bits out */
    __device__ __forceinline__ void block(int blk, unsigned long long word, int /* n */, int lane)
    {
        const int k = (blk << 3) + lane;
        if (lane < 8 && k < nbytes + 2) {
            const unsigned b = (unsigned)(word >> (lane << 3)) & 255u;
            if (out) out[k] = (uint8_t)b;
            if (k < nbytes) share ^= crc_mulmod(crc_byte(b), adv[nbytes - 1 - k]);
            else share ^= b << (k == nbytes ? 24 : 16);
        }
    }
};

/* one wave per staging row, behind the loader of the layout's kind (viterbi_row.h, coded_loader).  CODED_PLAIN, rate 1/2: the staged row is
 * [nsteps] pairs (stage_pitch = nbody = nsteps, even); behind a pattern it holds the nbody transmitted dibits, as they were on air.
 * qpsk_ctx_last_kernel()'s labels deframe_coded_decode_punct_kernel<x> and deframe_coded_decode_ilv_kernel<x> name the instances
 * <x, CODED_PUNCT> and <x, CODED_ILV> of this template.  The body stays in the kernel: routed through a device function, the instances come
 * out with two more scalar registers than DESIGN.md 4.4.7 / 4.4.8 record */
template <bool LDS, int KIND>
__global__ void __launch_bounds__(64)
deframe_coded_decode_kernel(DeframeCodedArgs a, int row0, unsigned long long *scratch, DeframeCodedBody b, IlvMul pi)
{
    const int lane = threadIdx.x;
    const int e = row0 + (int)blockIdx.x;
    const int stream = e / a.per_stream, slot = e - stream * a.per_stream;
    if (slot >= a.count[stream]) return;                                 /* per_stream <= max_packets */
    const size_t r = (size_t)stream * a.max_packets + slot;
    const size_t nblk = ((size_t)a.nsteps + 63) >> 6;
    PacketSink sink = {a.bytes ? a.bytes + r * (size_t)(a.nbytes + 2) : nullptr, a.crc_adv, a.nbytes, 0u};
    unsigned long long *gdec = LDS ? nullptr : scratch + (size_t)blockIdx.x * (nblk << 6);
    int32_t *info = a.info ? a.info + 4 * r : nullptr;
    const int8_t *row = a.stage + 2 * (size_t)e * (size_t)(KIND == CODED_PLAIN ? a.nsteps : b.stage_pitch);
    if constexpr (KIND == CODED_ILV) {      /* built here from the argument itself: through coded_loader pi's scalar loads move ahead of the return above */
        const IlvLoader ld = {row, a.flip, b.punct, pi};
        viterbi_row<LDS>(ld, a.nsteps, 0, gdec, info, sink);
    } else {
        const auto ld = coded_loader<KIND>(row, a.flip, b.punct, IlvMul{});      /* pi: CODED_ILV's, not looked at here */
        viterbi_row<LDS>(ld, a.nsteps, 0, gdec, info, sink);
    }
    unsigned share = sink.share;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) share ^= (unsigned)__shfl_xor((int)share, o, 64);
    if (lane == 0 && a.crc_ok) a.crc_ok[r] = (uint8_t)(((share & 0xFFFFu) ^ a.crc_init) == (share >> 16));
}

template <int KIND>
static void launch_decode_kind(const DeframeCodedArgs &a, const DeframeCodedBody &b, const IlvMul &pi, int row0, int nrows, unsigned long long *scratch,
                               bool lds, size_t bytes, hipStream_t s)
{
    if (lds) hipLaunchKernelGGL((deframe_coded_decode_kernel<true, KIND>), dim3(nrows), dim3(64), bytes, s, a, row0, scratch, b, pi);
    else hipLaunchKernelGGL((deframe_coded_decode_kernel<false, KIND>), dim3(nrows), dim3(64), 0, s, a, row0, scratch, b, pi);
}

} // namespace

int launch_deframe_coded_hunt(const DeframeCodedArgs &a, const DeframeCodedBody &b, hipStream_t s)
{
    if (a.nstreams <= 0 || a.nsym <= 0 || a.per_stream < 1 || a.per_stream > a.max_packets || !a.costas || !a.gain || !a.stage || !a.count ||
        b.nbody < 1 || b.stage_pitch < b.nbody || (b.stage_pitch & 1))
        return (int)hipErrorInvalidValue;
    const dim3 grid((a.nstreams + HUNT_WAVES - 1) / HUNT_WAVES), block(64 * HUNT_WAVES);
    hipLaunchKernelGGL(deframe_coded_hunt_kernel, grid, block, 0, s, a, b.nbody, b.stage_pitch);
    return (int)hipGetLastError();
}

int launch_deframe_coded_decode(const DeframeCodedArgs &a, DeframeCodedBody b, const CodedLayout &l, int row0, int nrows, unsigned long long *scratch,
                                bool lds, hipStream_t s)
{
    if (row0 < 0 || nrows <= 0 || (long long)row0 + nrows > (long long)a.nstreams * a.per_stream || !a.stage || !a.count || !a.flip || !a.crc_adv)
        return (int)hipErrorInvalidValue;
    if (!coded_layout_fits(l, a.nsteps) || b.nbody != coded_ndibits(l, a.nsteps) || (l.kind == CODED_PLAIN ? b.stage_pitch != b.nbody : b.stage_pitch < b.nbody))
        return (int)hipErrorInvalidValue;
    const size_t bytes = viterbi_scratch_bytes_per_row(a.nsteps);
    if (lds ? bytes > (size_t)VITERBI_LDS_MAX_BYTES : !scratch) return (int)hipErrorInvalidValue;
    b.kind = l.kind;
    b.punct = l.punct;
    const IlvMul pi = ilv_mul(l.ilv.n, l.ilv.s);      /* CODED_ILV: sent bit k lies at pi.at(k); the other kinds do not read it */
    if (l.kind == CODED_ILV) launch_decode_kind<CODED_ILV>(a, b, pi, row0, nrows, scratch, lds, bytes, s);
    else if (l.kind == CODED_PUNCT) launch_decode_kind<CODED_PUNCT>(a, b, pi, row0, nrows, scratch, lds, bytes, s);
    else launch_decode_kind<CODED_PLAIN>(a, b, pi, row0, nrows, scratch, lds, bytes, s);
    return (int)hipGetLastError();
}

} // namespace qpsk
