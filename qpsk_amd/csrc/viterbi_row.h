/*
 * viterbi_row.h -- one row of the K = 7, rate-1/2 Viterbi decoder by ONE WAVE (lane = new state): the forward pass, the trace-back and
 * the channel error count of qpsk_viterbi_batch (include/qpsk_hip.h), shared by viterbi.hip (rows of a caller's batch) and
 * deframe_coded.hip (the staged soft rows of packets found in a stream).  viterbi.hip's header describes the passes.  The three layouts of
 * a row (kernels.h, CodedLayout) are the same passes behind a LOADER of the soft pairs: PairLoader at rate 1/2, and one loader behind a pattern
 * whose position map is the identity (punctured) or the stride's (interleaved).
 *
 * The caller's kernel runs workgroups of exactly one wave (64 threads) and hands the row over as plain pointers; what happens to the
 * decoded bits is the caller's too: the trace-back gives every block of 64 steps to a SINK,
 *     sink.block(blk, word, n, lane)     word = the decoded bits of steps 64 blk .. 64 blk + n - 1 (bit j = step 64 blk + j; wave-uniform),
 * blocks in DESCENDING order.  LDS = true keeps the decision words in the launch's dynamic LDS (8 bytes per step padded to 64 steps),
 * otherwise they wait in gdec ([steps padded to 64] words of global memory).
 */
#ifndef QPSK_VITERBI_ROW_H
#define QPSK_VITERBI_ROW_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace qpsk {

constexpr int VITERBI_NEG = -(1 << 30);      /* the start penalty of the 63 other states (qpsk_hip.h) */

__device__ __forceinline__ int parity(unsigned v) { return __popc(v) & 1; }

/* lane `lane`: the soft pair of step t0 + lane after the -128 rule and d_flip; (0, 0) -- an erasure -- beyond the row */
__device__ __forceinline__ void load_soft(const int8_t *__restrict__ row, const uint8_t *__restrict__ flip, int t0, int nsteps, int lane,
                                          int &s0, int &s1)
{
    const int t = t0 + lane;
    s0 = s1 = 0;
    if (t < nsteps) {
        const unsigned w = *reinterpret_cast<const unsigned short *>(row + 2 * (size_t)t);
        s0 = max((int)(int8_t)(w & 255u), -127);
        s1 = max((int)(int8_t)(w >> 8), -127);
        if (flip) {
            const unsigned f = flip[t];
            s0 = (f & 1u) ? -s0 : s0;
            s1 = (f & 2u) ? -s1 : s1;
        }
    }
}

/* LOADERS: where a step's soft pair lies is the only thing a punctured code changes, so the row's passes take it as a policy:
 *     ld.load(t0, nsteps, lane, s0, s1)     lane `lane`: the pair of step t0 + lane after the -128 rule and d_flip; (0, 0) beyond the row
 * always for 64 steps at once, lane-parallel and a block ahead of the steps that use them: nothing of a loader is in the per-step chain.
 *
 * PairLoader: rate 1/2, row = [nsteps][2] int8, flip [nsteps] or NULL */
struct PairLoader {
    const int8_t *__restrict__ row;
    const uint8_t *__restrict__ flip;
    __device__ __forceinline__ void load(int t0, int nsteps, int lane, int &s0, int &s1) const { load_soft(row, flip, t0, nsteps, lane, s0, s1); }
};

/* Behind a pattern (p: kernels.h) sent bit (t, j) is sent bit number idx(t, j) of the row: where step t's first sent bit lies and which of its
 * two coded bits are sent -- one division by the period and two popcounts.  idx(t, 1) = idx(t, 0) + b0.  k0 < 2^18; it is 64-bit because the flat
 * row is addressed with it as it is (IlvMul::at takes its low word) */
struct SentStep {
    size_t k0;
    unsigned b0, b1;
};
__device__ __forceinline__ SentStep sent_step(const Puncture &p, unsigned t)
{
    const unsigned q = t / (unsigned)p.period, r = t - q * (unsigned)p.period;
    const unsigned low = (1u << r) - 1u;
    const unsigned b0 = (p.keep0 >> r) & 1u, b1 = (p.keep1 >> r) & 1u;
    return SentStep{(size_t)q * (unsigned)p.K + __popc(p.keep0 & low) + __popc(p.keep1 & low), b0, b1};
}

/* SentLoader: row = the flat int8 of the TRANSMITTED dibits, flip [ntx] over those dibits or NULL; sent bit k lies at flat position map.at(k),
 * its flip bit at the same on-air position.  A lane works out its step's sent_step and the position of its first sent bit once per 64 steps
 * (map.ahead gives the second's) and does byte loads; an unsent bit is 0, the erasure the decoder needs no special case for.  idx < nsent for
 * every sent bit of a step below nsteps and the map is a bijection, so the pad bit of an odd nsent is never read.  Lane-parallel and a block
 * ahead like PairLoader.  The two maps (kernels.h):
 *     PunctLoader   FlatMap, qpsk_viterbi_punct_batch: sent bit k is flat bit k, a step's two sent bits are adjacent bytes
 *     IlvLoader     IlvMul, qpsk_viterbi_ilv_batch (INTERLEAVING in include/qpsk_hip.h): pi(k) = k s mod n, one modular product (32-bit, no
 *                   64-bit division) for the step's first sent bit and a conditional subtract for its second, the bytes now s apart */
template <class Map>
struct SentLoader {
    const int8_t *__restrict__ row;
    const uint8_t *__restrict__ flip;
    Puncture p;
    Map map;
    /* the soft value at flat position a after the -128 rule and d_flip */
    template <class Pos>
    __device__ __forceinline__ int value(Pos a) const
    {
        const int v = max((int)row[a], -127);
        return (flip && ((flip[a >> 1] >> (a & 1)) & 1u)) ? -v : v;
    }
    __device__ __forceinline__ void load(int t0, int nsteps, int lane, int &s0, int &s1) const
    {
        const int t = t0 + lane;
        s0 = s1 = 0;
        if (t < nsteps) {
            const SentStep e = sent_step(p, (unsigned)t);
            const auto a0 = map.at(e.k0), a1 = map.ahead(a0, e.b0);
            if (e.b0) s0 = value(a0);
            if (e.b1) s1 = value(a1);
        }
    }
};
using PunctLoader = SentLoader<FlatMap>;
using IlvLoader = SentLoader<IlvMul>;

/* the loader of a layout's kind (kernels.h, CodedKind) over one row; p and pi are looked at by the kinds that have them */
template <int KIND>
__device__ __forceinline__ auto coded_loader(const int8_t *row, const uint8_t *flip, const Puncture &p, const IlvMul &pi)
{
    if constexpr (KIND == CODED_PLAIN) return PairLoader{row, flip};
    else if constexpr (KIND == CODED_PUNCT) return PunctLoader{row, flip, p, FlatMap{}};
    else return IlvLoader{row, flip, p, pi};
}

/* the channel errors of block blk, lane-parallel: cur / prev = the decoded bits of blocks blk / blk - 1 (bit j = step 64 blk + j).
 * x = bits t-6 .. t of the row with bit t - 6 lowest, so the generators apply bit-reversed: 171 -> 0x4F, 133 -> 0x6D */
template <class Loader>
__device__ __forceinline__ int block_errors(const Loader &ld, int blk, int nsteps, int lane, unsigned long long cur, unsigned long long prev)
{
    const unsigned long long lo = (cur << 6) | (prev >> 58), hi = cur >> 58;
    const unsigned x = (unsigned)((lo >> lane) | ((hi << 1) << (63 - lane))) & 127u;
    int s0, s1;
    ld.load(blk << 6, nsteps, lane, s0, s1);
    return (int)(s0 != 0 && (s0 < 0) != (bool)parity(x & 0x4Fu)) + (int)(s1 != 0 && (s1 < 0) != (bool)parity(x & 0x6Du));
}

/* the sink of qpsk_viterbi_batch: d_bits, bit t in byte t >> 3 (lanes 0..7 each store their byte of the block: a vector store) */
struct BitsSink {
    uint8_t *bits;      /* this row's ceil(nsteps / 8) bytes, or NULL */
    __device__ __forceinline__ void block(int blk, unsigned long long word, int n, int lane) const
    {
        if (bits && lane < ((n + 7) >> 3)) bits[(blk << 3) + lane] = (uint8_t)(word >> (lane << 3));
    }
};

#ifdef QPSK_VITERBI_PROFILE
#define VIT_STAMP(t) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory")
#endif

/* ld: the row's loader (above); flags = VITERBI_*; info: this row's four words or NULL (then nothing is counted) */
template <bool LDS, class Loader, class Sink>
__device__ __forceinline__ void viterbi_row(const Loader &ld, int nsteps, int flags, unsigned long long *gdec, int32_t *info, Sink &sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long ldec[];      /* LDS route: [nblk * 64] decision words */
    const int lane = threadIdx.x;
    const int nblk = (nsteps + 63) >> 6;
#ifdef QPSK_VITERBI_PROFILE
    unsigned long long stamp0, stamp1, stamp2;
    VIT_STAMP(stamp0);
#endif

    /* ---- forward */
    int sg0 = parity((unsigned)lane & 0x79u) ? -1 : 1, sg1 = parity((unsigned)lane & 0x5Bu) ? -1 : 1;
    asm volatile("" : "+v"(sg0), "+v"(sg1));      /* opaque: keeps b at a 24-bit multiply and a multiply-add instead of selects on +-1 */
    const int from0 = (lane >> 1) << 2, from1 = from0 | 128;      /* byte addresses of lanes ns >> 1 and (ns >> 1) | 32 */
    int pm = ((flags & VITERBI_OPEN_START) || lane == 0) ? 0 : VITERBI_NEG;
    int n0, n1;
    ld.load(0, nsteps, lane, n0, n1);
    for (int blk = 0; blk < nblk; blk++) {
        const int s0v = n0, s1v = n1;
        if (blk + 1 < nblk) ld.load((blk + 1) << 6, nsteps, lane, n0, n1);      /* a block ahead: no step waits on memory */
        const int n = min(64, nsteps - (blk << 6));
        unsigned dh[2] = {0u, 0u};
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int nh = min(32, n - 32 * half);
            unsigned acc = 0u;
#pragma unroll 8
            for (int j = 0; j < nh; j++) {
                const int s0 = __builtin_amdgcn_readlane(s0v, 32 * half + j), s1 = __builtin_amdgcn_readlane(s1v, 32 * half + j);
                const int b = __mul24(sg0, s0) + __mul24(sg1, s1);
                const int m0 = __builtin_amdgcn_ds_bpermute(from0, pm) + b;
                const int m1 = __builtin_amdgcn_ds_bpermute(from1, pm) - b;
                acc |= m1 > m0 ? 1u << j : 0u;       /* a tie keeps p0 */
                pm = max(m0, m1);
            }
            dh[half] = acc;
        }
        const unsigned dlo = dh[0], dhi = dh[1];
        const unsigned long long w = ((unsigned long long)dhi << 32) | dlo;
        if (LDS) ldec[(blk << 6) + lane] = w;
        else gdec[(blk << 6) + lane] = w;
    }
#ifdef QPSK_VITERBI_PROFILE
    VIT_STAMP(stamp1);
    if (flags & VITERBI_PROFILE_FORWARD_ONLY) {      /* measurement: the decisions are in memory / LDS, the metrics go out so that nothing is dead */
        if (info && lane < 4) info[lane] = lane == 0 ? pm : lane == 1 ? (int)(stamp1 - stamp0) : 0;
        return;
    }
#endif

    /* ---- the end state */
    int st = 0;
    if (flags & VITERBI_OPEN_END) {
        int mx = pm;
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) mx = max(mx, __shfl_xor(mx, h, 64));
        st = __ffsll((long long)__ballot(pm == mx)) - 1;      /* ties to the lowest state */
    }
    st = __builtin_amdgcn_readfirstlane(st);
    const int end_state = st, end_metric = __builtin_amdgcn_readlane(pm, st);

    /* ---- trace-back over the whole row, the error count one block behind it */
    unsigned long long later = 0;      /* the decoded bits of block blk + 1 */
    int errs = 0;
    for (int blk = nblk - 1; blk >= 0; blk--) {
        const unsigned long long w = LDS ? ldec[(blk << 6) + lane] : gdec[(blk << 6) + lane];
        const int wlo = (int)(unsigned)w, whi = (int)(unsigned)(w >> 32);
        const int n = min(64, nsteps - (blk << 6));
        unsigned long long word = 0;
#pragma unroll
        for (int half = 1; half >= 0; half--) {
            const int nh = min(32, n - 32 * half), wv = half ? whi : wlo;
            unsigned wh = 0u;
#pragma unroll 8
            for (int j = nh - 1; j >= 0; j--) {
                const unsigned d = ((unsigned)__builtin_amdgcn_readlane(wv, st) >> j) & 1u;      /* d[t][st]: bit j of state st's word */
                wh |= (unsigned)(st & 1) << j;
                st = (st >> 1) | (int)(d << 5);
            }
            word |= (unsigned long long)wh << (32 * half);
        }
        sink.block(blk, word, n, lane);
        if (info && blk + 1 < nblk) errs += block_errors(ld, blk + 1, nsteps, lane, later, word);
        later = word;
    }
    if (info) {
        /* the six bits before the row are the state the trace-back arrived at (0 unless open start): state bit k = bit -1 - k */
        errs += block_errors(ld, 0, nsteps, lane, later, (unsigned long long)(__brev((unsigned)st) >> 26) << 58);
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) errs += __shfl_xor(errs, h, 64);
#ifdef QPSK_VITERBI_PROFILE
        VIT_STAMP(stamp2);
        if (flags & VITERBI_PROFILE_CYCLES) {      /* measurement: words 1, 2 = the cycles of the two passes */
            if (lane < 4) info[lane] = lane == 0 ? end_metric : lane == 1 ? (int)(stamp1 - stamp0) : lane == 2 ? (int)(stamp2 - stamp1) : errs;
            return;
        }
#endif
        if (lane < 4) info[lane] = lane == 0 ? end_metric : lane == 1 ? end_state : lane == 2 ? st : errs;
    }
}

} // namespace qpsk
#endif
