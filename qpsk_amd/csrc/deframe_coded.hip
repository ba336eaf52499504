/*
 * deframe_coded.hip -- convolutionally coded packets out of continuous streams of costas_frame[] (include/qpsk_hip.h,
 * qpsk_deframer_push_coded): deframe.hip's hunt with soft decisions where that kernel builds bytes, and viterbi.hip's decoder on the
 * packets the hunt completes.
 *
 *   deframe_coded_hunt_kernel     one wave per stream, deframe_kernel's structure line for line (X, the bit planes, the wave-uniform walk
 *                                 over the candidate masks, the carried tail: see deframe.hip).  The body of a packet is Nc = nbody dibits
 *                                 (8 (nbytes + 2) + 6 at rate 1/2, fewer behind a puncturing pattern: the hunt only takes the number); the lanes quantise the body symbols that lie in this push's row (soft_quant.h: the turn by
 *                                 the packet's rotation and q(x) of qpsk_soft_batch, with this push's gain) lane-parallel, 8-byte loads and
 *                                 2-byte stores, into the packet's soft row.  An incomplete packet's row is the stream's pending buffer
 *                                 (int8 pairs: no float history is carried, every body symbol arrives in the push that completes the
 *                                 sync word or a later one).  A packet completed in this push with output row slot < max_packets gets
 *                                 staging row stream * per_stream + slot: the pending pairs are copied there, the rest is quantised
 *                                 into it, and pos / rot / score are written here.  The hunt never looks at a decoder's result.
 *   deframe_coded_decode_kernel   one wave per staging row; rows at or beyond the stream's count retire at once.  viterbi_row.h's forward
 *                                 pass and trace-back with the keystream as flip and flags 0; the trace-back hands every 64 decoded bits
 *                                 to PacketSink: lanes 0..7 take one byte each, store it (bytes below nbytes + 2) and add its share of the
 *                                 CRC -- crc16() is linear, byte k of nbytes contributes crc_byte(b) x^(8 (nbytes - 1 - k)), the factors
 *                                 come from a table -- and a wave xor behind the trace-back sums the shares.
 *
 * A staging row is addressed by (stream, slot), the packet's place in the outputs, so there is no list to append to and no atomic:
 * per_stream = min(max_packets, nsym / (nsync + Nc) + 1) bounds what one push can complete in a stream (packet ends lie nsync + Nc
 * apart), and the decode grid covers nstreams * per_stream rows.  Staging rows lie stage_pitch = Nc rounded up to even dibits apart, so
 * that copy_pairs' 4-byte accesses stay aligned when a punctured Nc is odd.  Vector stores only.
 *
 *   deframe_coded_decode_punct_kernel   (qpsk_deframer_reset_coded_punct) the same decode with viterbi_row.h's PunctLoader on the Nc staged
 *                                 dibits: nsteps = 8 (nbytes + 2) + 6 trellis steps, the keystream flips the transmitted dibits.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "qpsk_device.h"
#include "deframe_bits.h"
#include "soft_quant.h"
#include "viterbi_row.h"

namespace qpsk {

namespace {

constexpr int DC_WAVES = 4;       /* streams per workgroup: one wave each */
constexpr int DC_CHUNK = 4;       /* steps of 64 positions per load batch, as deframe_kernel */

__device__ __forceinline__ unsigned ring_at(const float2 *row, long long i) { return ring_of((unsigned)data_rule(row[i])); }

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

__device__ __forceinline__ void report(const DeframeCodedArgs &a, int stream, int slot, long long pos, int rot, int score, int lane)
{
    const size_t r = (size_t)stream * a.max_packets + slot;      /* the pointer tests stay scalar branches around lane 0's stores */
    if (a.pos) {
        if (lane == 0) a.pos[r] = pos;
    }
    if (a.rot) {
        if (lane == 0) a.rot[r] = rot;
    }
    if (a.score) {
        if (lane == 0) a.score[r] = score;
    }
}

__global__ void __launch_bounds__(64 * DC_WAVES)
deframe_coded_hunt_kernel(DeframeCodedArgs a, int nbody, int stage_pitch)
{
    const int lane = threadIdx.x & 63;
    const int stream = blockIdx.x * DC_WAVES + (int)(threadIdx.x >> 6);
    if (stream >= a.nstreams) return;
    const int n = a.nsync, N = nbody;
    const long long nsym = a.nsym;
    const float2 *row = a.costas + (size_t)stream * (size_t)nsym;
    uint8_t *st = a.state + (size_t)stream * a.state_stride;
    DeframeHeader *hd = reinterpret_cast<DeframeHeader *>(st);
    uint8_t *tail = st + DEFRAME_TAIL_OFFSET;
    int8_t *pend = reinterpret_cast<int8_t *>(st + DEFRAME_PEND_OFFSET);
    const float g = a.gain[stream];
    bool bad = a.check_gain && !finite_f(g);

    const long long len = hd->len;
    long long h = hd->h;
    int pending = hd->pending, have = hd->have;
    const int T = (int)(len < (long long)(n - 1) ? len : (long long)(n - 1));
    int count = 0;

    /* 1. the packet collecting since an earlier push */
    if (pending) {
        const long long ppos = hd->ppos;
        const int prot = hd->prot, pscore = hd->pscore;
        const int need = N - have;
        if (nsym >= need) {
            if (count < a.per_stream) {
                int8_t *dst = a.stage + 2 * ((size_t)stream * a.per_stream + count) * (size_t)stage_pitch;
                copy_pairs(pend, have, dst, lane);
                bad |= quantise_body(row, need, prot, g, dst + 2 * (size_t)have, lane);
                report(a, stream, count, ppos, prot, pscore, lane);
            }
            count++;
            pending = 0;
        } else {
            bad |= quantise_body(row, (int)nsym, prot, g, pend + 2 * (size_t)have, lane);
            have += (int)nsym;
        }
    }

    /* 2. the hunt over the positions whose word completes in this push: p_x in [0, P), global p = len - T + p_x; in-push offsets are
     *    32-bit (X < 2^22), hx = h - (len - T) */
    const long long base0 = len - T;
    const int X = T + (int)nsym;
    const int P = X - n + 1;
    if (!pending && P > 0 && h < base0 + P) {
        int hx = h > base0 ? (int)(h - base0) : 0;
        const int s0 = hx >> 6;                                          /* steps below h hold no candidate */
        const int steps = (P + 63) >> 6;
        auto xload = [&](int w) -> unsigned {
            const int j = 64 * w + lane;
            if (j >= X) return 0u;
            return j < T ? (unsigned)tail[j] : ring_at(row, j - T);
        };
        const unsigned long long m0 = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        const unsigned long long m1 = n > 64 ? (n == 128 ? ~0ull : ((1ull << (n - 64)) - 1ull)) : 0ull;
        bool moved = false;
        /* a chunk: steps s .. s + DC_CHUNK - 1 from plane words s .. s + DC_CHUNK + 1; the chunk after a packet starts at the step that
         * holds the new hx */
        for (int s = s0; s < steps;) {
            unsigned long long lo[DC_CHUNK + 2], hi[DC_CHUNK + 2];
            {
                unsigned v[DC_CHUNK + 2];
#pragma unroll
                for (int k = 0; k < DC_CHUNK + 2; k++) v[k] = k < 2 || s + k - 2 < steps ? xload(s + k) : 0u;
#pragma unroll
                for (int k = 0; k < DC_CHUNK + 2; k++) { lo[k] = ballot64(v[k] & 1u); hi[k] = ballot64(v[k] & 2u); }
            }
            int px = -1, pk = 0;
#pragma unroll
            for (int k = 0; k < DC_CHUNK; k++) {
                const int gx = 64 * (s + k);
                if (px >= 0 || s + k >= steps || gx + 63 < hx) continue;
                const unsigned long long x0 = funnel64(lo[k], lo[k + 1], lane), x1 = funnel64(hi[k], hi[k + 1], lane);
                unsigned long long d0 = x0 ^ a.sync_lo[0];
                unsigned long long d1 = x1 ^ a.sync_hi[0] ^ (~x0 & a.sync_lo[0]);
                int c1 = __popcll(~d1 & d0 & m0), c2 = __popcll(d1 & ~d0 & m0), c3 = __popcll(d1 & d0 & m0);
                if (n > 64) {
                    const unsigned long long y0 = funnel64(lo[k + 1], lo[k + 2], lane), y1 = funnel64(hi[k + 1], hi[k + 2], lane);
                    d0 = y0 ^ a.sync_lo[1];
                    d1 = y1 ^ a.sync_hi[1] ^ (~y0 & a.sync_lo[1]);
                    c1 += __popcll(~d1 & d0 & m1); c2 += __popcll(d1 & ~d0 & m1); c3 += __popcll(d1 & d0 & m1);
                }
                int best = n - c1 - c2 - c3, r = 0;                      /* the first rotation with the largest count */
                if (c1 > best) { best = c1; r = 1; }
                if (c2 > best) { best = c2; r = 2; }
                if (c3 > best) { best = c3; r = 3; }
                const unsigned long long mask = ballot64(gx + lane < P && gx + lane >= hx && best >= a.min_score);
                if (mask) {
                    const int l = __builtin_ctzll(mask);
                    pk = __builtin_amdgcn_readlane(best * 4 + r, l);
                    px = gx + l;
                }
            }
            if (px < 0) {
                s += DC_CHUNK;
                continue;
            }
            hx = px + n + N;
            moved = true;
            const int row0 = px + n - T;                                 /* >= 0: the body starts in the row */
            if (hx > X) {                                                /* collects into the next pushes */
                const int got = (int)nsym - row0;
                bad |= quantise_body(row + row0, got, pk & 3, g, pend, lane);
                pending = 1;
                have = got;
                if (lane == 0) { hd->ppos = base0 + px; hd->prot = pk & 3; hd->pscore = pk >> 2; }
                break;
            }
            if (count < a.per_stream) {                                  /* row0 + N <= nsym: the whole body lies in the row */
                int8_t *dst = a.stage + 2 * ((size_t)stream * a.per_stream + count) * (size_t)stage_pitch;
                bad |= quantise_body(row + row0, N, pk & 3, g, dst, lane);
                report(a, stream, count, base0 + px, pk & 3, pk >> 2, lane);
            }
            count++;
            s = hx >> 6;
        }
        if (moved) h = base0 + hx;
    }

    /* 3. the carried tail: the last min(len + nsym, nsync - 1) values of D, read before any lane writes */
    const long long len2 = len + nsym;
    const int T2 = X < n - 1 ? X : n - 1;
    unsigned tv[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int i = lane + 64 * q;
        const int j = X - T2 + i;
        tv[q] = i < T2 ? (j < T ? (unsigned)tail[j] : ring_at(row, j - T)) : 0u;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int i = lane + 64 * q;
        if (i < T2) tail[i] = (uint8_t)tv[q];
    }
    if (lane == 0) {
        hd->len = len2;
        hd->h = h;
        hd->pending = pending;
        hd->have = have;
        a.count[stream] = count;
    }
    if (__builtin_expect(bad, 0) && a.status) __hip_atomic_store(a.status, STATUS_SOFT_NONFINITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
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

/* rate 1/2: the staged row is [nsteps] pairs (stage_pitch = nbody = nsteps, even) */
template <bool LDS>
__global__ void __launch_bounds__(64)
deframe_coded_decode_kernel(DeframeCodedArgs a, int row0, unsigned long long *scratch)
{
    const int lane = threadIdx.x;
    const int e = row0 + (int)blockIdx.x;
    const int stream = e / a.per_stream, slot = e - stream * a.per_stream;
    if (slot >= a.count[stream]) return;                                 /* per_stream <= max_packets */
    const size_t r = (size_t)stream * a.max_packets + slot;
    const size_t nblk = ((size_t)a.nsteps + 63) >> 6;
    PacketSink sink = {a.bytes ? a.bytes + r * (size_t)(a.nbytes + 2) : nullptr, a.crc_adv, a.nbytes, 0u};
    const PairLoader ld = {a.stage + 2 * (size_t)e * (size_t)a.nsteps, a.flip};
    viterbi_row<LDS>(ld, a.nsteps, 0, LDS ? nullptr : scratch + (size_t)blockIdx.x * (nblk << 6), a.info ? a.info + 4 * r : nullptr, sink);
    unsigned share = sink.share;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) share ^= (unsigned)__shfl_xor((int)share, o, 64);
    if (lane == 0 && a.crc_ok) a.crc_ok[r] = (uint8_t)(((share & 0xFFFFu) ^ a.crc_init) == (share >> 16));
}

/* behind a pattern: the staged row holds the nbody transmitted dibits.  The same lines with the other loader, written out a second time
 * and not shared through a function: routed through one, the rate-1/2 kernels above come out with two more scalar registers than
 * DESIGN.md 4.4.7 records, and they are not to move */
template <bool LDS>
__global__ void __launch_bounds__(64)
deframe_coded_decode_punct_kernel(DeframeCodedArgs a, int row0, unsigned long long *scratch, DeframeCodedBody b)
{
    const int lane = threadIdx.x;
    const int e = row0 + (int)blockIdx.x;
    const int stream = e / a.per_stream, slot = e - stream * a.per_stream;
    if (slot >= a.count[stream]) return;                                 /* per_stream <= max_packets */
    const size_t r = (size_t)stream * a.max_packets + slot;
    const size_t nblk = ((size_t)a.nsteps + 63) >> 6;
    PacketSink sink = {a.bytes ? a.bytes + r * (size_t)(a.nbytes + 2) : nullptr, a.crc_adv, a.nbytes, 0u};
    const PunctLoader ld = {a.stage + 2 * (size_t)e * (size_t)b.stage_pitch, a.flip, b.punct};
    viterbi_row<LDS>(ld, a.nsteps, 0, LDS ? nullptr : scratch + (size_t)blockIdx.x * (nblk << 6), a.info ? a.info + 4 * r : nullptr, sink);
    unsigned share = sink.share;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) share ^= (unsigned)__shfl_xor((int)share, o, 64);
    if (lane == 0 && a.crc_ok) a.crc_ok[r] = (uint8_t)(((share & 0xFFFFu) ^ a.crc_init) == (share >> 16));
}

} // namespace

int launch_deframe_coded_hunt(const DeframeCodedArgs &a, const DeframeCodedBody &b, hipStream_t s)
{
    if (a.nstreams <= 0 || a.nsym <= 0 || a.per_stream < 1 || a.per_stream > a.max_packets || !a.costas || !a.gain || !a.stage || !a.count ||
        b.nbody < 1 || b.stage_pitch < b.nbody || (b.stage_pitch & 1))
        return (int)hipErrorInvalidValue;
    const dim3 grid((a.nstreams + DC_WAVES - 1) / DC_WAVES), block(64 * DC_WAVES);
    hipLaunchKernelGGL(deframe_coded_hunt_kernel, grid, block, 0, s, a, b.nbody, b.stage_pitch);
    return (int)hipGetLastError();
}

int launch_deframe_coded_decode(const DeframeCodedArgs &a, const DeframeCodedBody &b, int row0, int nrows, unsigned long long *scratch, bool lds,
                                hipStream_t s)
{
    if (row0 < 0 || nrows <= 0 || (long long)row0 + nrows > (long long)a.nstreams * a.per_stream || !a.stage || !a.count || !a.flip || !a.crc_adv)
        return (int)hipErrorInvalidValue;
    if (b.punctured ? b.punct.period < 1 || b.punct.period > 32 || b.punct.K < 1 || 2LL * b.nbody < punct_nsent(b.punct, a.nsteps) || b.stage_pitch < b.nbody
                    : b.nbody != a.nsteps || b.stage_pitch != a.nsteps)
        return (int)hipErrorInvalidValue;
    const size_t bytes = viterbi_scratch_bytes_per_row(a.nsteps);
    if (lds ? bytes > (size_t)VITERBI_LDS_MAX_BYTES : !scratch) return (int)hipErrorInvalidValue;
    if (b.punctured) {
        if (lds) hipLaunchKernelGGL(deframe_coded_decode_punct_kernel<true>, dim3(nrows), dim3(64), bytes, s, a, row0, scratch, b);
        else hipLaunchKernelGGL(deframe_coded_decode_punct_kernel<false>, dim3(nrows), dim3(64), 0, s, a, row0, scratch, b);
    } else if (lds) hipLaunchKernelGGL(deframe_coded_decode_kernel<true>, dim3(nrows), dim3(64), bytes, s, a, row0, scratch);
    else hipLaunchKernelGGL(deframe_coded_decode_kernel<false>, dim3(nrows), dim3(64), 0, s, a, row0, scratch);
    return (int)hipGetLastError();
}

} // namespace qpsk
