/*
 * viterbi.hip -- the K = 7, rate-1/2 convolutional code (generators 171 / 133 octal) on the int8 soft decisions of qpsk_soft_batch:
 * qpsk_conv_encode_batch and qpsk_viterbi_batch.  The definition is the contract in include/qpsk_hip.h, restated in numpy by
 * tests/test_viterbi_cpu.py (conv_encode_ref, viterbi_ref).
 *
 * NEW DESIGN: the reference has no FEC (parity unpinned by the reference).  Everything is integer arithmetic, so GPU
 * and numpy agree bit for bit by construction; what has to be kept is the tie rule (a tie keeps predecessor p0; the open end takes
 * the lowest state among equal metrics).
 *
 * viterbi_kernel: ONE WAVE PER ROW, lane = new state ns.
 *   forward     Both generators have bits 0 and 6 set, so the branch metric into register value ns | 64 is minus the one into ns: a lane
 *               keeps two signs (sg0, sg1) and computes b = sg0 s0 + sg1 s1, m0 = pm[ns >> 1] + b, m1 = pm[(ns >> 1) | 32] - b.  The
 *               two path metrics come from other lanes by ds_bpermute (cross-lane, no LDS memory).  (s0, s1) of a step is wave-uniform:
 *               lane l loads the pair of step 64 k + l (one 128-byte load per 64 steps, issued one block ahead, d_flip and the
 *               -128 -> -127 rule applied lane-parallel) and the step reads its pair with v_readlane.  The compare's result never
 *               leaves the vector unit: every lane ORs its own decision into bit (t & 63) of a 64-bit word it keeps (the decisions of
 *               64 steps, TRANSPOSED: lane ns holds d[64 k .. 64 k + 63][ns]), and every 64 steps the wave stores its 64 words with one
 *               coalesced 512-byte VECTOR store (global scratch), or ds_write (LDS route).  int32 metrics, no normalisation.
 *   trace-back  a chain of nsteps dependent steps on wave-uniform values: the words of 64 steps are read back lane-parallel, a step reads
 *               the word of lane st with v_readlane (st in a scalar register), and shift / and / or run on the scalar unit.  The 64
 *               decoded bits of a block are a scalar pair; lanes 0..7 each take their byte of it and store it (a vector store).
 *   error count re-encodes from the decoded bits, 64 steps per lane-parallel pass: lane l of block k needs bits 64 k + l - 6 .. 64 k + l,
 *               i.e. the decoded words of blocks k and k - 1; the trace-back meets them in that order, one block late.
 * The two routes differ only in where the decision words wait between the passes: viterbi_kernel (global scratch, [row][steps padded
 * to 64] words) and viterbi_lds_kernel (dynamic LDS, 8 bytes per padded step).
 *
 * The row's passes themselves live in viterbi_row.h, which deframe_coded.hip runs on the packets of a stream as well.
 *
 * conv_encode_kernel: one thread per coded dibit; a plain kernel so that a loopback stays on the device.
 *
 * PUNCTURED RATES (qpsk_viterbi_punct_batch, qpsk_conv_encode_punct_batch; PUNCTURING in include/qpsk_hip.h, restated by
 * tests/test_punct_cpu.py).  A punctured decode IS the decode of the zero-filled row, and a zero is an erasure the passes above need no
 * special case for, so viterbi_punct_kernel / viterbi_punct_lds_kernel are the same two kernels behind viterbi_row.h's PunctLoader: the
 * lane that loaded the pair of step 64 k + l now works out where the (up to) two sent bits of that step lie in the transmitted row -- one
 * division by the period and two popcounts per lane and 64 steps -- and loads them, and their flip bits, bytewise; unsent bits are 0.
 * That happens where the load sat, lane-parallel and a block ahead; the per-step chain is untouched.  conv_encode_punct_kernel: one
 * thread per transmitted dibit, its two sent bits mapped back to (step, generator) through a table of the period's K <= 64 sent bits.
 *
 * INTERLEAVING (qpsk_viterbi_ilv_batch, qpsk_conv_encode_ilv_batch; INTERLEAVING in include/qpsk_hip.h, restated by tests/test_ilv_cpu.py).
 * The coded bits of a row are spread over the row on air by pi(k) = k s mod n.  Both sides gather: viterbi_ilv_kernel /
 * viterbi_ilv_lds_kernel are the punctured kernels behind viterbi_row.h's IlvLoader, which reads sent bit k's soft value and flip bit at
 * pi(k); conv_encode_ilv_kernel is conv_encode_punct_kernel whose on-air bit a takes sent bit a s^-1 mod n.  No scatter, no atomics, no
 * pass of its own over memory, and nothing in the per-step chain.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "punct_table.h"
#include "viterbi_row.h"

namespace qpsk {

namespace {

struct VitArgs {
    const int8_t *soft;
    size_t pitch;                 /* dibits between rows: steps at rate 1/2, transmitted dibits behind a pattern */
    int nsteps, flags;
    const uint8_t *flip;
    unsigned long long *scratch;  /* [rows][nblk * 64] decision words (global route) */
    uint8_t *bits;
    int32_t *info;
    Puncture punct;               /* the punctured kernels only */
};

/* workgroup = wave = row blockIdx.x of the call (viterbi_row.h); PUNCT: the row is what was transmitted and PunctLoader finds the steps in it */
template <bool LDS, bool PUNCT>
__device__ __forceinline__ void viterbi_batch_row(const VitArgs &a)
{
    const size_t row = blockIdx.x;
    const size_t nblk = ((size_t)a.nsteps + 63) >> 6;
    BitsSink sink = {a.bits ? a.bits + row * (((size_t)a.nsteps + 7) >> 3) : nullptr};
    unsigned long long *gdec = LDS ? nullptr : a.scratch + row * (nblk << 6);
    int32_t *info = a.info ? a.info + 4 * row : nullptr;
    if (PUNCT) {
        const PunctLoader ld = {a.soft + 2 * row * a.pitch, a.flip, a.punct};
        viterbi_row<LDS>(ld, a.nsteps, a.flags, gdec, info, sink);
    } else {
        const PairLoader ld = {a.soft + 2 * row * a.pitch, a.flip};
        viterbi_row<LDS>(ld, a.nsteps, a.flags, gdec, info, sink);
    }
}

__global__ void __launch_bounds__(64) viterbi_kernel(VitArgs a) { viterbi_batch_row<false, false>(a); }
__global__ void __launch_bounds__(64) viterbi_lds_kernel(VitArgs a) { viterbi_batch_row<true, false>(a); }
__global__ void __launch_bounds__(64) viterbi_punct_kernel(VitArgs a) { viterbi_batch_row<false, true>(a); }
__global__ void __launch_bounds__(64) viterbi_punct_lds_kernel(VitArgs a) { viterbi_batch_row<true, true>(a); }

/* the same row behind IlvLoader; the stride is an argument of these two kernels alone */
template <bool LDS>
__device__ __forceinline__ void viterbi_ilv_row(const VitArgs &a, const IlvMul &pi)
{
    const size_t row = blockIdx.x;
    const size_t nblk = ((size_t)a.nsteps + 63) >> 6;
    BitsSink sink = {a.bits ? a.bits + row * (((size_t)a.nsteps + 7) >> 3) : nullptr};
    unsigned long long *gdec = LDS ? nullptr : a.scratch + row * (nblk << 6);
    int32_t *info = a.info ? a.info + 4 * row : nullptr;
    const IlvLoader ld = {a.soft + 2 * row * a.pitch, a.flip, a.punct, pi};
    viterbi_row<LDS>(ld, a.nsteps, a.flags, gdec, info, sink);
}

__global__ void __launch_bounds__(64) viterbi_ilv_kernel(VitArgs a, IlvMul pi) { viterbi_ilv_row<false>(a, pi); }
__global__ void __launch_bounds__(64) viterbi_ilv_lds_kernel(VitArgs a, IlvMul pi) { viterbi_ilv_row<true>(a, pi); }

/* one thread per coded dibit: register r of step t = bits t-6 .. t (bit t in bit 0), zeros before the row and in the tail */
__global__ void __launch_bounds__(256)
conv_encode_kernel(const uint8_t *__restrict__ in, size_t nrows, int nbits, int nsteps, uint8_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * (size_t)nsteps) return;
    const size_t row = i / (size_t)nsteps;
    const int t = (int)(i - row * (size_t)nsteps);
    const uint8_t *src = in + row * (size_t)((nbits + 7) >> 3);
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const int p = t - k;
        if (p >= 0 && p < nbits) r |= ((unsigned)(src[p >> 3] >> (p & 7)) & 1u) << k;
    }
    out[i] = (uint8_t)(parity(r & 0x79u) | (parity(r & 0x5Bu) << 1));
}

/* one thread per transmitted dibit: sent bits 2 d and 2 d + 1 of the row, each mapped back to (t, j) through the table (punct_table.h) and encoded as
 * conv_encode_kernel does; a sent bit at or beyond nsent -- the pad bit of an odd nsent -- is 0 */
__global__ void __launch_bounds__(256)
conv_encode_punct_kernel(const uint8_t *__restrict__ in, size_t nrows, int nbits, unsigned nsent, unsigned ntx, int period, int K, PunctTable tab,
                         uint8_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * (size_t)ntx) return;
    const size_t row = i / ntx;
    const unsigned d = (unsigned)(i - row * ntx);
    const uint8_t *src = in + row * (size_t)((nbits + 7) >> 3);
    unsigned dibit = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const unsigned k = 2 * d + h;
        if (k >= nsent) continue;
        int t;
        const unsigned j = punct_sent_step(k, period, K, tab, &t);
        unsigned r = 0;
#pragma unroll
        for (int b = 0; b < 7; b++) {
            const int p = t - b;
            if (p >= 0 && p < nbits) r |= ((unsigned)(src[p >> 3] >> (p & 7)) & 1u) << b;
        }
        dibit |= (unsigned)parity(r & (j ? 0x5Bu : 0x79u)) << h;
    }
    out[i] = (uint8_t)dibit;
}

/* conv_encode_punct_kernel behind the permutation: on-air bits 2 d and 2 d + 1 take sent bits (2 d) s^-1 mod n and that + s^-1 (mod n); a sent
 * bit number at or beyond nsent is the pad of an odd nsent, 0 */
__global__ void __launch_bounds__(256)
conv_encode_ilv_kernel(const uint8_t *__restrict__ in, size_t nrows, int nbits, unsigned nsent, unsigned ntx, int period, int K, PunctTable tab,
                       IlvMul inv, uint8_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * (size_t)ntx) return;
    const size_t row = i / ntx;
    const unsigned d = (unsigned)(i - row * ntx);
    const uint8_t *src = in + row * (size_t)((nbits + 7) >> 3);
    unsigned dibit = 0, k = inv.at(2 * d);
#pragma unroll
    for (int h = 0; h < 2; h++, k = inv.next(k)) {
        if (k >= nsent) continue;
        int t;
        const unsigned j = punct_sent_step(k, period, K, tab, &t);
        unsigned r = 0;
#pragma unroll
        for (int b = 0; b < 7; b++) {
            const int p = t - b;
            if (p >= 0 && p < nbits) r |= ((unsigned)(src[p >> 3] >> (p & 7)) & 1u) << b;
        }
        dibit |= (unsigned)parity(r & (j ? 0x5Bu : 0x79u)) << h;
    }
    out[i] = (uint8_t)dibit;
}

} // namespace

size_t viterbi_scratch_bytes_per_row(int nsteps) { return sizeof(unsigned long long) * (((size_t)nsteps + 63) & ~(size_t)63); }

int launch_viterbi(const int8_t *soft, size_t pitch, int nrows, int nsteps, const Puncture *punct, const uint8_t *flip, int flags,
                   unsigned long long *scratch, bool lds, uint8_t *bits, int32_t *info, hipStream_t s)
{
    if (nrows <= 0 || nsteps <= 0 || nsteps > VITERBI_MAX_STEPS || !soft || (!bits && !info)) return (int)hipErrorInvalidValue;
    if (punct && (punct->period < 1 || punct->period > 32 || punct->K < 1)) return (int)hipErrorInvalidValue;
    const size_t bytes = viterbi_scratch_bytes_per_row(nsteps);
    if (lds ? bytes > (size_t)VITERBI_LDS_MAX_BYTES : !scratch) return (int)hipErrorInvalidValue;
    const VitArgs a = {soft, pitch, nsteps, flags, flip, scratch, bits, info, punct ? *punct : Puncture{1, 1u, 1u, 2}};
    if (lds) hipLaunchKernelGGL(punct ? viterbi_punct_lds_kernel : viterbi_lds_kernel, dim3(nrows), dim3(64), bytes, s, a);
    else hipLaunchKernelGGL(punct ? viterbi_punct_kernel : viterbi_kernel, dim3(nrows), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

/* n = 2 ntx of the pattern, 1 <= s < max(n, 2); that s is coprime to n and sinv its inverse is the caller's (api.cpp, ilv_make) */
static bool ilv_fits(const Interleave &v, long long ntx)
{
    return ntx >= 1 && ntx <= (long long)VITERBI_MAX_STEPS && v.n == 2u * (unsigned)ntx && v.s >= 1 && v.s < v.n && v.sinv >= 1 && v.sinv < v.n;
}

int launch_viterbi_ilv(const int8_t *soft, size_t pitch, int nrows, int nsteps, const Puncture &punct, const Interleave &ilv, const uint8_t *flip,
                       int flags, unsigned long long *scratch, bool lds, uint8_t *bits, int32_t *info, hipStream_t s)
{
    if (nrows <= 0 || nsteps <= 0 || nsteps > VITERBI_MAX_STEPS || !soft || (!bits && !info)) return (int)hipErrorInvalidValue;
    if (punct.period < 1 || punct.period > 32 || punct.K < 1 || !ilv_fits(ilv, (punct_nsent(punct, nsteps) + 1) / 2)) return (int)hipErrorInvalidValue;
    const size_t bytes = viterbi_scratch_bytes_per_row(nsteps);
    if (lds ? bytes > (size_t)VITERBI_LDS_MAX_BYTES : !scratch) return (int)hipErrorInvalidValue;
    const VitArgs a = {soft, pitch, nsteps, flags, flip, scratch, bits, info, punct};
    const IlvMul pi = ilv_mul(ilv.n, ilv.s);
    if (lds) hipLaunchKernelGGL(viterbi_ilv_lds_kernel, dim3(nrows), dim3(64), bytes, s, a, pi);
    else hipLaunchKernelGGL(viterbi_ilv_kernel, dim3(nrows), dim3(64), 0, s, a, pi);
    return (int)hipGetLastError();
}

int launch_conv_encode(const uint8_t *bits, int nrows, int nbits, int nsteps, uint8_t *dibits, hipStream_t s)
{
    if (nrows <= 0 || nbits <= 0 || nsteps < nbits || !bits || !dibits) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)nrows * (size_t)nsteps;
    if ((n + 255) / 256 > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bits, (size_t)nrows, nbits, nsteps, dibits);
    return (int)hipGetLastError();
}

int launch_conv_encode_punct(const uint8_t *bits, int nrows, int nbits, int nsteps, const Puncture &p, uint8_t *dibits, hipStream_t s)
{
    if (nrows <= 0 || nbits <= 0 || nsteps < nbits || !bits || !dibits || p.period < 1 || p.period > 32 || p.K < 1 || p.K > 64)
        return (int)hipErrorInvalidValue;
    const long long nsent = punct_nsent(p, nsteps), ntx = (nsent + 1) / 2;
    if (ntx < 1) return (int)hipErrorInvalidValue;
    PunctTable tab;
    if (!punct_table_make(p, &tab)) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)nrows * (size_t)ntx;
    if ((n + 255) / 256 > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_encode_punct_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bits, (size_t)nrows, nbits, (unsigned)nsent,
                       (unsigned)ntx, p.period, p.K, tab, dibits);
    return (int)hipGetLastError();
}

int launch_conv_encode_ilv(const uint8_t *bits, int nrows, int nbits, int nsteps, const Puncture &p, const Interleave &ilv, uint8_t *dibits,
                           hipStream_t s)
{
    if (nrows <= 0 || nbits <= 0 || nsteps < nbits || !bits || !dibits || p.period < 1 || p.period > 32 || p.K < 1 || p.K > 64)
        return (int)hipErrorInvalidValue;
    const long long nsent = punct_nsent(p, nsteps), ntx = (nsent + 1) / 2;
    if (!ilv_fits(ilv, ntx)) return (int)hipErrorInvalidValue;
    PunctTable tab;
    if (!punct_table_make(p, &tab)) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)nrows * (size_t)ntx;
    if ((n + 255) / 256 > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_encode_ilv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bits, (size_t)nrows, nbits, (unsigned)nsent,
                       (unsigned)ntx, p.period, p.K, tab, ilv_mul(ilv.n, ilv.sinv), dibits);
    return (int)hipGetLastError();
}

} // namespace qpsk
