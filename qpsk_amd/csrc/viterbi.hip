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
 * conv_encode_kernel: one thread per coded dibit; a plain kernel so that a loopback stays on the device.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace qpsk {

namespace {

constexpr int NEG = -(1 << 30);      /* the start penalty of the 63 other states (qpsk_hip.h) */

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

/* the channel errors of block blk, lane-parallel: cur / prev = the decoded bits of blocks blk / blk - 1 (bit j = step 64 blk + j).
 * x = bits t-6 .. t of the row with bit t - 6 lowest, so the generators apply bit-reversed: 171 -> 0x4F, 133 -> 0x6D */
__device__ __forceinline__ int block_errors(const int8_t *__restrict__ row, const uint8_t *__restrict__ flip, int blk, int nsteps, int lane,
                                            unsigned long long cur, unsigned long long prev)
{
    const unsigned long long lo = (cur << 6) | (prev >> 58), hi = cur >> 58;
    const unsigned x = (unsigned)((lo >> lane) | ((hi << 1) << (63 - lane))) & 127u;
    int s0, s1;
    load_soft(row, flip, blk << 6, nsteps, lane, s0, s1);
    return (int)(s0 != 0 && (s0 < 0) != (bool)parity(x & 0x4Fu)) + (int)(s1 != 0 && (s1 < 0) != (bool)parity(x & 0x6Du));
}

struct VitArgs {
    const int8_t *soft;
    size_t pitch;                 /* steps between rows */
    int nsteps, flags;
    const uint8_t *flip;
    unsigned long long *scratch;  /* [rows][nblk * 64] decision words (global route) */
    uint8_t *bits;
    int32_t *info;
};

#ifdef QPSK_VITERBI_PROFILE
#define VIT_STAMP(t) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory")
#endif

template <bool LDS>
__device__ __forceinline__ void viterbi_row(const VitArgs &a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long ldec[];      /* LDS route: [nblk * 64] decision words */
    const int lane = threadIdx.x, row = blockIdx.x;
    const int nsteps = a.nsteps, nblk = (nsteps + 63) >> 6;
    const int8_t *soft = a.soft + 2 * (size_t)row * a.pitch;
    unsigned long long *gdec = a.scratch + (size_t)row * ((size_t)nblk << 6);
#ifdef QPSK_VITERBI_PROFILE
    unsigned long long stamp0, stamp1, stamp2;
    VIT_STAMP(stamp0);
#endif

    /* ---- forward */
    int sg0 = parity((unsigned)lane & 0x79u) ? -1 : 1, sg1 = parity((unsigned)lane & 0x5Bu) ? -1 : 1;
    asm volatile("" : "+v"(sg0), "+v"(sg1));      /* opaque: keeps b at a 24-bit multiply and a multiply-add instead of selects on +-1 */
    const int from0 = (lane >> 1) << 2, from1 = from0 | 128;      /* byte addresses of lanes ns >> 1 and (ns >> 1) | 32 */
    int pm = ((a.flags & VITERBI_OPEN_START) || lane == 0) ? 0 : NEG;
    int n0, n1;
    load_soft(soft, a.flip, 0, nsteps, lane, n0, n1);
    for (int blk = 0; blk < nblk; blk++) {
        const int s0v = n0, s1v = n1;
        if (blk + 1 < nblk) load_soft(soft, a.flip, (blk + 1) << 6, nsteps, lane, n0, n1);      /* a block ahead: no step waits on memory */
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
    if (a.flags & VITERBI_PROFILE_FORWARD_ONLY) {      /* measurement: the decisions are in memory / LDS, the metrics go out so that nothing is dead */
        if (a.info && lane < 4) a.info[4 * (size_t)row + lane] = lane == 0 ? pm : lane == 1 ? (int)(stamp1 - stamp0) : 0;
        return;
    }
#endif

    /* ---- the end state */
    int st = 0;
    if (a.flags & VITERBI_OPEN_END) {
        int mx = pm;
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) mx = max(mx, __shfl_xor(mx, h, 64));
        st = __ffsll((long long)__ballot(pm == mx)) - 1;      /* ties to the lowest state */
    }
    st = __builtin_amdgcn_readfirstlane(st);
    const int end_state = st, end_metric = __builtin_amdgcn_readlane(pm, st);

    /* ---- trace-back over the whole row, the error count one block behind it */
    const size_t nbytes = ((size_t)nsteps + 7) >> 3;
    uint8_t *bits = a.bits ? a.bits + (size_t)row * nbytes : nullptr;
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
        if (bits && lane < ((n + 7) >> 3)) bits[(blk << 3) + lane] = (uint8_t)(word >> (lane << 3));
        if (a.info && blk + 1 < nblk) errs += block_errors(soft, a.flip, blk + 1, nsteps, lane, later, word);
        later = word;
    }
    if (a.info) {
        /* the six bits before the row are the state the trace-back arrived at (0 unless open start): state bit k = bit -1 - k */
        errs += block_errors(soft, a.flip, 0, nsteps, lane, later, (unsigned long long)(__brev((unsigned)st) >> 26) << 58);
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) errs += __shfl_xor(errs, h, 64);
#ifdef QPSK_VITERBI_PROFILE
        VIT_STAMP(stamp2);
        if (a.flags & VITERBI_PROFILE_CYCLES) {      /* measurement: words 1, 2 = the cycles of the two passes */
            if (lane < 4) a.info[4 * (size_t)row + lane] = lane == 0 ? end_metric : lane == 1 ? (int)(stamp1 - stamp0) : lane == 2 ? (int)(stamp2 - stamp1) : errs;
            return;
        }
#endif
        if (lane < 4) a.info[4 * (size_t)row + lane] = lane == 0 ? end_metric : lane == 1 ? end_state : lane == 2 ? st : errs;
    }
}

__global__ void __launch_bounds__(64) viterbi_kernel(VitArgs a) { viterbi_row<false>(a); }
__global__ void __launch_bounds__(64) viterbi_lds_kernel(VitArgs a) { viterbi_row<true>(a); }

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

} // namespace

size_t viterbi_scratch_bytes_per_row(int nsteps) { return sizeof(unsigned long long) * (((size_t)nsteps + 63) & ~(size_t)63); }

int launch_viterbi(const int8_t *soft, size_t pitch, int nrows, int nsteps, const uint8_t *flip, int flags, unsigned long long *scratch,
                   bool lds, uint8_t *bits, int32_t *info, hipStream_t s)
{
    if (nrows <= 0 || nsteps <= 0 || nsteps > VITERBI_MAX_STEPS || !soft || (!bits && !info)) return (int)hipErrorInvalidValue;
    const size_t bytes = viterbi_scratch_bytes_per_row(nsteps);
    if (lds ? bytes > (size_t)VITERBI_LDS_MAX_BYTES : !scratch) return (int)hipErrorInvalidValue;
    const VitArgs a = {soft, pitch, nsteps, flags, flip, scratch, bits, info};
    if (lds) hipLaunchKernelGGL(viterbi_lds_kernel, dim3(nrows), dim3(64), bytes, s, a);
    else hipLaunchKernelGGL(viterbi_kernel, dim3(nrows), dim3(64), 0, s, a);
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

} // namespace qpsk
