/*
 * viterbi_stream.hip -- the streaming Viterbi decoder with a sliding trace-back window (VITERBI STREAM in include/qpsk_hip.h, restated in
 * numpy by tests/test_viterbi_stream_cpu.py) and its transmit twin, the encoder that carries its register from call to call.
 *
 * viterbi_stream_kernel / viterbi_stream_punct_kernel (a push) and viterbi_stream_flush_kernel: ONE WAVE PER STREAM, lane = new state.
 *   forward     viterbi_row.h's chain, step for step: v_readlane of the wave-uniform pair, two ds_bpermute, the decision ORed into the lane's
 *               transposed 64-bit word, the pairs loaded one block ahead behind the same loaders (PairLoader / PunctLoader over the push's
 *               rows; the pattern's phase is 0 at a push's first step).  What is new is around the chain, once per 64 steps: the metrics are
 *               normalised (max(pm) subtracted) and the block's 64 decision words go into the stream's RING in global memory with one
 *               coalesced 512-byte vector store, beside four ballot words (sign and non-zero of s0 and s1) for the error count.
 *   alignment   the chain only ever runs over whole 64-step blocks that begin at a multiple of 64 steps since the reset: what a push leaves over
 *               (up to 63 soft pairs, depunctured, after the -128 rule) waits in the state as PENDING pairs and goes first in the next push.
 *               Decision points are multiples of 64, so this cannot be seen from outside; only the flush runs a partial block.
 *   decision    after the block that ends at T = k W: the best state, then the trace-back of viterbi_row.h over the min(T, D + W) / 64 blocks of
 *               the ring, newest first.  The D / 64 newest blocks are walked through only; the rest is emitted (lanes 0..7 store a byte each)
 *               and re-encoded for the error count one block behind the walk, as block_errors does it, but against the ballot words: the
 *               soft values themselves are long gone.  The register before the oldest block is the last emitted word, carried in the state.
 *   positions   a wave needs no absolute position: the host (api_vstream.cpp) keeps the 64-bit totals and hands each launch the ring slot of
 *               its first block, the blocks the ring holds and the blocks since the last decision point, all small.
 *
 * STATE per stream, state_stride bytes (vstream_state_stride): pm[64] int32 at 0, the pending pairs [64][2] int8 at 256, the last emitted
 * word at 384, then the ring: nring blocks of 64 decision words at 512, and nring blocks of 4 ballot words behind them.  Every word of it is
 * written by the lane that reads it back (lane l: pm[l], pair l, word l of a block; lanes 0..3: a block's ballots; lane 0: the last word), with
 * ordinary vector stores.  What a launch both writes and reads back -- the ring -- is read lane-parallel, never through a wave-uniform load,
 * which could be served from a scalar cache that the vector stores do not update.
 *
 * conv_encode_stream_kernel: conv_encode_punct_kernel without a tail, over a register that starts from d_state_in instead of 0.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "punct_table.h"
#include "viterbi_row.h"

namespace qpsk {

namespace {

constexpr int VS_PEND = 256, VS_LAST = 384, VS_RING = 512;

struct VStreamView {
    int *pm;                      /* [64] */
    unsigned short *pend;         /* [64] pairs, s0 in the low byte */
    unsigned long long *last;     /* the last 64 emitted bits, the newest in bit 63 */
    unsigned long long *dec;      /* [nring][64] */
    unsigned long long *bal;      /* [nring][4]: s0 < 0, s0 != 0, s1 < 0, s1 != 0 */
};

__device__ __forceinline__ VStreamView vstream_view(const VStreamArgs &a)
{
    uint8_t *base = a.state + (size_t)blockIdx.x * a.state_stride;
    return VStreamView{reinterpret_cast<int *>(base), reinterpret_cast<unsigned short *>(base + VS_PEND),
                       reinterpret_cast<unsigned long long *>(base + VS_LAST), reinterpret_cast<unsigned long long *>(base + VS_RING),
                       reinterpret_cast<unsigned long long *>(base + VS_RING + (size_t)a.nring * 512)};
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = max(v, __shfl_xor(v, h, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = min(v, __shfl_xor(v, h, 64));
    return v;
}
/* a wave-uniform 64-bit value out of lane k */
__device__ __forceinline__ unsigned long long lane_word(unsigned long long v, int k)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, k), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), k);
    return ((unsigned long long)hi << 32) | lo;
}

/* what a lane keeps for the chain (viterbi_row.h, forward) */
struct Chain {
    int sg0, sg1, from0, from1;
};
__device__ __forceinline__ Chain chain_make(int lane)
{
    Chain c = {parity((unsigned)lane & 0x79u) ? -1 : 1, parity((unsigned)lane & 0x5Bu) ? -1 : 1, (lane >> 1) << 2, ((lane >> 1) << 2) | 128};
    asm volatile("" : "+v"(c.sg0), "+v"(c.sg1));      /* opaque, as in viterbi_row: a 24-bit multiply and a multiply-add instead of selects */
    return c;
}

/* one step of the chain: bit j of acc takes the lane's decision */
__device__ __forceinline__ void forward_step(const Chain &c, int s0, int s1, int j, unsigned &acc, int &pm)
{
    const int b = __mul24(c.sg0, s0) + __mul24(c.sg1, s1);
    const int m0 = __builtin_amdgcn_ds_bpermute(c.from0, pm) + b;
    const int m1 = __builtin_amdgcn_ds_bpermute(c.from1, pm) - b;
    acc |= m1 > m0 ? 1u << j : 0u;       /* a tie keeps p0 */
    pm = max(m0, m1);
}

/* the 64 steps of one block, lane l holding the pair of the block's step l: viterbi_row's inner loops.  Returns the lane's decision word */
__device__ __forceinline__ unsigned long long forward_block(const Chain &c, int s0v, int s1v, int &pm)
{
    unsigned dh[2] = {0u, 0u};
#pragma unroll
    for (int half = 0; half < 2; half++) {
        unsigned acc = 0u;
#pragma unroll 8
        for (int j = 0; j < 32; j++)
            forward_step(c, __builtin_amdgcn_readlane(s0v, 32 * half + j), __builtin_amdgcn_readlane(s1v, 32 * half + j), j, acc, pm);
        dh[half] = acc;
    }
    return ((unsigned long long)dh[1] << 32) | dh[0];
}

/* the flush's partial block of n < 64 steps: the same steps, a plain loop -- it runs once per stream and flush */
__device__ __forceinline__ unsigned long long forward_partial(const Chain &c, int s0v, int s1v, int n, int &pm)
{
    unsigned dh[2] = {0u, 0u};
    for (int t = 0; t < n; t++) forward_step(c, __builtin_amdgcn_readlane(s0v, t), __builtin_amdgcn_readlane(s1v, t), t & 31, dh[t >> 5], pm);
    return ((unsigned long long)dh[1] << 32) | dh[0];
}

/* a block goes into ring slot `slot`: its decision words and its ballots */
__device__ __forceinline__ void ring_store(const VStreamView &v, int slot, int lane, unsigned long long w, int s0v, int s1v)
{
    v.dec[((size_t)slot << 6) + lane] = w;
    const unsigned long long neg0 = __ballot(s0v < 0), nz0 = __ballot(s0v != 0), neg1 = __ballot(s1v < 0), nz1 = __ballot(s1v != 0);
    if (lane < 4) v.bal[((size_t)slot << 2) + lane] = lane == 0 ? neg0 : lane == 1 ? nz0 : lane == 2 ? neg1 : nz1;
}

/* the state of the largest metric, ties to the lowest state; *spread = max(pm) - min(pm) */
__device__ __forceinline__ int best_state(int pm, int *spread)
{
    const int mx = wave_max(pm);
    *spread = mx - wave_min(pm);
    return __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(pm == mx)) - 1);
}

/* the channel errors and the non-zero soft values of one block against its ballots b (lanes 0..3), lane-parallel as block_errors: cur / prev =
 * the decoded bits of the block and of the one before it */
__device__ __forceinline__ void ballot_errors(unsigned long long b, int lane, unsigned long long cur, unsigned long long prev, int &errs, int &nz)
{
    const unsigned long long lo = (cur << 6) | (prev >> 58), hi = cur >> 58;
    const unsigned x = (unsigned)((lo >> lane) | ((hi << 1) << (63 - lane))) & 127u;
    const unsigned long long c0 = __ballot(parity(x & 0x4Fu) != 0), c1 = __ballot(parity(x & 0x6Du) != 0);
    const unsigned long long neg0 = lane_word(b, 0), nz0 = lane_word(b, 1), neg1 = lane_word(b, 2), nz1 = lane_word(b, 3);
    errs += __popcll(nz0 & (neg0 ^ c0)) + __popcll(nz1 & (neg1 ^ c1));
    nz += __popcll(nz0) + __popcll(nz1);
}

/* what a call reports (d_info) and where its bits go */
struct Emit {
    uint8_t *bits;      /* this stream's row of d_bits, or NULL */
    int outblk;         /* 64-bit blocks this call has emitted so far */
    int errs, nz, st, spread;
};

/* One decision: from state st, walk the ntrace newest blocks of the ring, the newest (n_newest <= 64 steps) in slot `slot`; the nskip newest are
 * walked through only, the others emitted in ascending order behind e.outblk and counted.  viterbi_row.h's trace-back, a block at a time */
template <bool PARTIAL>
__device__ __forceinline__ void decide(const VStreamView &v, int nring, int lane, int st, int spread, int slot, int ntrace, int nskip, int n_newest,
                                       unsigned long long &last, Emit &e)
{
    e.st = st;
    e.spread = spread;
    const int nemit = max(ntrace - nskip, 0);
    if (nemit == 0) return;      /* nothing is old enough yet: no walk */
    unsigned long long later = 0, later_bal = 0, newest = 0;
    for (int i = 0; i < ntrace; i++) {
        const unsigned long long w = v.dec[((size_t)slot << 6) + lane];
        const unsigned long long b = lane < 4 ? v.bal[((size_t)slot << 2) + lane] : 0ull;
        const int wlo = (int)(unsigned)w, whi = (int)(unsigned)(w >> 32);
        const int n = PARTIAL && i == 0 ? n_newest : 64;
        unsigned long long word = 0;
        if (PARTIAL && i == 0) {      /* the flush's newest block: a plain loop over its n_newest <= 64 steps */
            for (int t = n - 1; t >= 0; t--) {
                const unsigned d = ((unsigned)__builtin_amdgcn_readlane(t >> 5 ? whi : wlo, st) >> (t & 31)) & 1u;
                word |= (unsigned long long)(st & 1) << t;
                st = (st >> 1) | (int)(d << 5);
            }
        } else {
#pragma unroll
            for (int half = 1; half >= 0; half--) {
                const int wv = half ? whi : wlo;
                unsigned wh = 0u;
#pragma unroll 8
                for (int j = 31; j >= 0; j--) {
                    const unsigned d = ((unsigned)__builtin_amdgcn_readlane(wv, st) >> j) & 1u;      /* d[t][st]: bit j of state st's word */
                    wh |= (unsigned)(st & 1) << j;
                    st = (st >> 1) | (int)(d << 5);
                }
                word |= (unsigned long long)wh << (32 * half);
            }
        }
        if (i >= nskip) {
            const int ob = e.outblk + (ntrace - 1 - i);
            if (e.bits && lane < ((n + 7) >> 3)) e.bits[((size_t)ob << 3) + lane] = (uint8_t)(word >> (lane << 3));
            if (i > nskip) ballot_errors(later_bal, lane, later, word, e.errs, e.nz);
            else newest = word;
            later = word;
            later_bal = b;
        }
        slot = slot == 0 ? nring - 1 : slot - 1;
    }
    ballot_errors(later_bal, lane, later, last, e.errs, e.nz);      /* the oldest emitted block, behind the bits emitted before it */
    last = newest;      /* the last 64 emitted bits; behind a partial block (the flush's) nothing reads them again */
    e.outblk += nemit;
}

__device__ __forceinline__ void emit_info(const VStreamArgs &a, int lane, const Emit &e)
{
    if (a.info && lane < 4) a.info[4 * (size_t)blockIdx.x + lane] = lane == 0 ? e.errs : lane == 1 ? e.nz : lane == 2 ? e.st : e.spread;
}

/* a push: the pending pairs, then the a.n steps of this stream's row */
template <int KIND>
__device__ __forceinline__ void vstream_push(const VStreamArgs &a)
{
    const int lane = threadIdx.x;
    const VStreamView v = vstream_view(a);
    const auto ld = coded_loader<KIND>(a.soft + 2 * (size_t)blockIdx.x * a.pitch, nullptr, a.punct, IlvMul{});
    const Chain c = chain_make(lane);
    /* lane l: the pair at position 64 blk + l of (pending ++ push); (0, 0) beyond it.  Only block 0 reaches into the pending pairs */
    const auto load = [&](int blk, int &s0, int &s1) {
        const int t = (blk << 6) - a.pc + lane;
        s0 = s1 = 0;
        if (t < 0) {
            const unsigned w = v.pend[lane];
            s0 = (int)(int8_t)(w & 255u);
            s1 = (int)(int8_t)(w >> 8);
        } else {
            ld.load(t, a.n, 0, s0, s1);
        }
    };
    int pm = v.pm[lane];
    unsigned long long last = lane_word(lane == 0 ? *v.last : 0ull, 0);
    Emit e = {a.bits ? a.bits + (size_t)blockIdx.x * a.bits_pitch : nullptr, 0, 0, 0, -1, 0};
    const int nblk = (a.pc + a.n) >> 6;
    int slot = a.slot, have = a.have, wphase = a.wphase;
    int n0, n1;
    load(0, n0, n1);
    for (int blk = 0; blk < nblk; blk++) {
        const int s0v = n0, s1v = n1;
        load(blk + 1, n0, n1);      /* a block ahead; behind the last whole block it is what stays pending */
        pm -= wave_max(pm);
        const unsigned long long w = forward_block(c, s0v, s1v, pm);
        ring_store(v, slot, lane, w, s0v, s1v);
        have = min(have + 1, a.nring);
        if (++wphase == a.wblk) {
            wphase = 0;
            int spread;
            const int st = best_state(pm, &spread);
            decide<false>(v, a.nring, lane, st, spread, slot, have, a.dblk, 64, last, e);
        }
        slot = slot + 1 == a.nring ? 0 : slot + 1;
    }
    const int rem = (a.pc + a.n) & 63;
    if (lane < rem) v.pend[lane] = (unsigned short)(((unsigned)n0 & 255u) | (((unsigned)n1 & 255u) << 8));
    v.pm[lane] = pm;
    if (lane == 0) *v.last = last;
    emit_info(a, lane, e);
}

__global__ void __launch_bounds__(64) viterbi_stream_kernel(VStreamArgs a) { vstream_push<CODED_PLAIN>(a); }
__global__ void __launch_bounds__(64) viterbi_stream_punct_kernel(VStreamArgs a) { vstream_push<CODED_PUNCT>(a); }

/* the flush: the a.pc pending steps as a partial block, one decision over the a.have blocks not yet emitted (a.slot: the newest of them), and
 * the stream is as after a reset */
__global__ void __launch_bounds__(64) viterbi_stream_flush_kernel(VStreamArgs a)
{
    const int lane = threadIdx.x;
    const VStreamView v = vstream_view(a);
    int pm = v.pm[lane];
    unsigned long long last = lane_word(lane == 0 ? *v.last : 0ull, 0);
    Emit e = {a.bits ? a.bits + (size_t)blockIdx.x * a.bits_pitch : nullptr, 0, 0, 0, -1, 0};
    if (a.pc > 0) {
        int s0v = 0, s1v = 0;
        if (lane < a.pc) {
            const unsigned w = v.pend[lane];
            s0v = (int)(int8_t)(w & 255u);
            s1v = (int)(int8_t)(w >> 8);
        }
        pm -= wave_max(pm);
        const unsigned long long w = forward_partial(chain_make(lane), s0v, s1v, a.pc, pm);
        ring_store(v, a.slot, lane, w, s0v, s1v);
    }
    int spread;
    int st = best_state(pm, &spread);
    if (a.flags & VSTREAM_TERMINATED) st = 0;
    decide<true>(v, a.nring, lane, st, spread, a.slot, a.have, 0, a.pc > 0 ? a.pc : 64, last, e);
    v.pm[lane] = lane == 0 ? 0 : VITERBI_NEG;
    if (lane == 0) *v.last = 0ull;
    emit_info(a, lane, e);
}

/* a reset's state: the start metrics, nothing emitted yet */
__global__ void __launch_bounds__(64) viterbi_stream_init_kernel(VStreamArgs a)
{
    const int lane = threadIdx.x;
    const VStreamView v = vstream_view(a);
    v.pm[lane] = lane == 0 ? 0 : VITERBI_NEG;
    if (lane == 0) *v.last = 0ull;
}

/* the encoder's register of step t from a row of packed bits behind the six bits of `state` (bit k of it = the bit of step -1 - k) */
struct StreamRegister {
    const uint8_t *__restrict__ src;
    unsigned state;
    __device__ __forceinline__ unsigned operator()(int t) const
    {
        unsigned r = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const int p = t - k;
            r |= (p >= 0 ? ((unsigned)(src[p >> 3] >> (p & 7)) & 1u) : ((state >> (-1 - p)) & 1u)) << k;
        }
        return r;
    }
};

struct EncodeStreamArgs {
    const uint8_t *in;
    size_t nrows;
    int nbits;
    unsigned nsent, ntx;
    Puncture punct;
    PunctTable tab;
    const uint8_t *state_in;
    uint8_t *state_out, *out;
};

/* one thread per transmitted dibit; the thread of a row's first dibit also leaves the register behind the row */
__global__ void __launch_bounds__(256) conv_encode_stream_kernel(EncodeStreamArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nrows * (size_t)a.ntx) return;
    const size_t row = i / a.ntx;
    const unsigned d = (unsigned)(i - row * a.ntx);
    const StreamRegister reg = {a.in + row * (size_t)((a.nbits + 7) >> 3), a.state_in ? (unsigned)a.state_in[row] & 63u : 0u};
    a.out[i] = (uint8_t)coded_dibit(d, a.nsent, a.punct, a.tab, FlatMap{}, [&](int t, unsigned j) { return parity(reg(t) & (j ? 0x5Bu : 0x79u)); });
    if (d == 0 && a.state_out) a.state_out[row] = (uint8_t)(reg(a.nbits - 1) & 63u);
}

} // namespace

size_t vstream_state_stride(int nring) { return (size_t)VS_RING + (size_t)nring * (512 + 32); }

static bool vstream_args_fit(const VStreamArgs &a, int nstreams)
{
    return nstreams >= 1 && a.state && a.nring >= 2 && a.nring <= VSTREAM_MAX_SPAN / 64 && a.dblk >= 1 && a.wblk >= 1 && a.dblk + a.wblk == a.nring &&
           a.state_stride >= vstream_state_stride(a.nring) && a.slot >= 0 && a.slot < a.nring && a.have >= 0 && a.have <= a.nring && a.pc >= 0 &&
           a.pc < 64 && (a.bits || a.info);
}

int launch_vstream_init(const VStreamArgs &a, int nstreams, hipStream_t s)
{
    if (nstreams < 1 || !a.state || a.nring < 2 || a.state_stride < vstream_state_stride(a.nring)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(viterbi_stream_init_kernel, dim3(nstreams), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

int launch_vstream_push(const VStreamArgs &a, int nstreams, bool punctured, hipStream_t s)
{
    CodedLayout l;
    l.punct = a.punct;
    if (!vstream_args_fit(a, nstreams) || !a.soft || a.wphase < 0 || a.wphase >= a.wblk || !coded_layout_fits(l, a.n)) return (int)hipErrorInvalidValue;
    if (!punctured && !(a.punct.period == 1 && a.punct.K == 2)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(punctured ? viterbi_stream_punct_kernel : viterbi_stream_kernel, dim3(nstreams), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

int launch_vstream_flush(const VStreamArgs &a, int nstreams, hipStream_t s)
{
    if (!vstream_args_fit(a, nstreams)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(viterbi_stream_flush_kernel, dim3(nstreams), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

int launch_conv_encode_stream(const uint8_t *bits, int nrows, int nbits, const Puncture &p, const uint8_t *state_in, uint8_t *state_out,
                              uint8_t *dibits, hipStream_t s)
{
    CodedLayout l;
    l.punct = p;
    if (nrows <= 0 || !bits || !dibits || !coded_layout_fits(l, nbits) || nbits % p.period) return (int)hipErrorInvalidValue;
    const long long nsent = punct_nsent(p, nbits);
    if (nsent < 2 || (nsent & 1)) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)nrows * (size_t)(nsent / 2);
    if ((n + 255) / 256 > 0x7fffffffull) return (int)hipErrorInvalidValue;
    EncodeStreamArgs a = {bits, (size_t)nrows, nbits, (unsigned)nsent, (unsigned)(nsent / 2), p, {}, state_in, state_out, dibits};
    if (!punct_table_make(p, &a.tab)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_encode_stream_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
