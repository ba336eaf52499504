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
 * THE LAYERS.  Where the coded bits of a row lie on air is a CodedLayout (kernels.h): plain rate 1/2; behind a puncturing pattern
 * (qpsk_*_punct_batch; PUNCTURING in include/qpsk_hip.h, restated by tests/test_punct_cpu.py); behind a pattern and an interleaver's stride
 * (qpsk_*_ilv_batch; INTERLEAVING, tests/test_ilv_cpu.py).  Each is the one before behind one more map, and the code is written that way,
 * as the numpy restatements are: one launch_viterbi and one launch_conv_encode take the layout, and its kind picks the kernel.
 *   decode   A punctured decode IS the decode of the zero-filled row, and a zero is an erasure the passes above need no special case for, so
 *            all six kernels are viterbi_batch_row behind the loader of their kind (viterbi_row.h, coded_loader).  Behind a pattern the lane
 *            that loaded the pair of step 64 k + l works out where the (up to) two sent bits of that step lie in the transmitted row -- one
 *            division by the period and two popcounts per lane and 64 steps -- and loads them, and their flip bits, bytewise; unsent bits
 *            are 0.  Behind a stride as well, sent bit k and its flip bit are read at pi(k) = k s mod n: the same loader over another
 *            position map.  That happens where the load sat, lane-parallel and a block ahead; the per-step chain is untouched.
 *   encode   conv_encode_punct_kernel / conv_encode_ilv_kernel: one thread per transmitted dibit, punct_table.h's coded_dibit -- the dibit's
 *            two sent bits (themselves, or sent bits a s^-1 mod n of on-air bits a) mapped back to (step, generator) through a table of the
 *            period's K <= 64 sent bits -- over the same register-from-the-packed-row functor conv_encode_kernel uses.
 * Both sides gather: no scatter, no atomics, no pass of its own over memory, and nothing in the per-step chain.
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
    Puncture punct;               /* the layout's pattern */
};

/* workgroup = wave = row blockIdx.x of the call (viterbi_row.h) behind the loader of the layout's kind; pi: the interleaved kernels' own argument */
template <bool LDS, int KIND>
__device__ __forceinline__ void viterbi_batch_row(const VitArgs &a, const IlvMul &pi)
{
    const size_t row = blockIdx.x;
    const size_t nblk = ((size_t)a.nsteps + 63) >> 6;
    BitsSink sink = {a.bits ? a.bits + row * (((size_t)a.nsteps + 7) >> 3) : nullptr};
    unsigned long long *gdec = LDS ? nullptr : a.scratch + row * (nblk << 6);
    int32_t *info = a.info ? a.info + 4 * row : nullptr;
    const auto ld = coded_loader<KIND>(a.soft + 2 * row * a.pitch, a.flip, a.punct, pi);
    viterbi_row<LDS>(ld, a.nsteps, a.flags, gdec, info, sink);
}

/* the six names stay one kernel each, so that a profile reads as the tables of DESIGN.md do.  IlvMul{} (n = 0) is a placeholder the plain and
 * punctured loaders never look at (coded_loader): it must stay unused there */
__global__ void __launch_bounds__(64) viterbi_kernel(VitArgs a) { viterbi_batch_row<false, CODED_PLAIN>(a, IlvMul{}); }
__global__ void __launch_bounds__(64) viterbi_lds_kernel(VitArgs a) { viterbi_batch_row<true, CODED_PLAIN>(a, IlvMul{}); }
__global__ void __launch_bounds__(64) viterbi_punct_kernel(VitArgs a) { viterbi_batch_row<false, CODED_PUNCT>(a, IlvMul{}); }
__global__ void __launch_bounds__(64) viterbi_punct_lds_kernel(VitArgs a) { viterbi_batch_row<true, CODED_PUNCT>(a, IlvMul{}); }
__global__ void __launch_bounds__(64) viterbi_ilv_kernel(VitArgs a, IlvMul pi) { viterbi_batch_row<false, CODED_ILV>(a, pi); }
__global__ void __launch_bounds__(64) viterbi_ilv_lds_kernel(VitArgs a, IlvMul pi) { viterbi_batch_row<true, CODED_ILV>(a, pi); }

/* the encoder's register of step t from a row of packed bits: bits t-6 .. t (bit t in bit 0), zeros before the row and in the tail */
struct RowRegister {
    const uint8_t *__restrict__ src;
    int nbits;
    __device__ __forceinline__ unsigned operator()(int t) const
    {
        unsigned r = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const int p = t - k;
            if (p >= 0 && p < nbits) r |= ((unsigned)(src[p >> 3] >> (p & 7)) & 1u) << k;
        }
        return r;
    }
};

/* one thread per coded dibit */
__global__ void __launch_bounds__(256)
conv_encode_kernel(const uint8_t *__restrict__ in, size_t nrows, int nbits, int nsteps, uint8_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * (size_t)nsteps) return;
    const size_t row = i / (size_t)nsteps;
    const RowRegister reg = {in + row * (size_t)((nbits + 7) >> 3), nbits};
    const unsigned r = reg((int)(i - row * (size_t)nsteps));
    out[i] = (uint8_t)(parity(r & 0x79u) | (parity(r & 0x5Bu) << 1));
}

/* behind a pattern: one thread per transmitted dibit, punct_table.h's walk from the dibit to its (up to) two coded bits, each encoded as
 * conv_encode_kernel does */
struct EncodeArgs {
    const uint8_t *in;
    size_t nrows;
    int nbits;
    unsigned nsent, ntx;
    Puncture punct;
    PunctTable tab;
    uint8_t *out;
};

template <class Map>
__device__ __forceinline__ void conv_encode_sent(const EncodeArgs &a, const Map &map)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nrows * (size_t)a.ntx) return;
    const size_t row = i / a.ntx;
    const RowRegister reg = {a.in + row * (size_t)((a.nbits + 7) >> 3), a.nbits};
    a.out[i] = (uint8_t)coded_dibit((unsigned)(i - row * a.ntx), a.nsent, a.punct, a.tab, map,
                                    [&](int t, unsigned j) { return parity(reg(t) & (j ? 0x5Bu : 0x79u)); });
}

__global__ void __launch_bounds__(256) conv_encode_punct_kernel(EncodeArgs a) { conv_encode_sent(a, FlatMap{}); }
__global__ void __launch_bounds__(256) conv_encode_ilv_kernel(EncodeArgs a, IlvMul inv) { conv_encode_sent(a, inv); }

} // namespace

size_t viterbi_scratch_bytes_per_row(int nsteps) { return sizeof(unsigned long long) * (((size_t)nsteps + 63) & ~(size_t)63); }

int launch_viterbi(const int8_t *soft, size_t pitch, int nrows, int nsteps, const CodedLayout &l, const uint8_t *flip, int flags,
                   unsigned long long *scratch, bool lds, uint8_t *bits, int32_t *info, hipStream_t s)
{
    if (nrows <= 0 || !soft || (!bits && !info) || !coded_layout_fits(l, nsteps)) return (int)hipErrorInvalidValue;
    const size_t bytes = viterbi_scratch_bytes_per_row(nsteps);
    if (lds ? bytes > (size_t)VITERBI_LDS_MAX_BYTES : !scratch) return (int)hipErrorInvalidValue;
    const VitArgs a = {soft, pitch, nsteps, flags, flip, scratch, bits, info, l.punct};
    const dim3 grid(nrows), block(64);
    const size_t shared = lds ? bytes : 0;
    if (l.kind == CODED_ILV)
        hipLaunchKernelGGL(lds ? viterbi_ilv_lds_kernel : viterbi_ilv_kernel, grid, block, shared, s, a, ilv_mul(l.ilv.n, l.ilv.s));
    else if (l.kind == CODED_PUNCT)
        hipLaunchKernelGGL(lds ? viterbi_punct_lds_kernel : viterbi_punct_kernel, grid, block, shared, s, a);
    else
        hipLaunchKernelGGL(lds ? viterbi_lds_kernel : viterbi_kernel, grid, block, shared, s, a);
    return (int)hipGetLastError();
}

int launch_conv_encode(const uint8_t *bits, int nrows, int nbits, int nsteps, const CodedLayout &l, uint8_t *dibits, hipStream_t s)
{
    if (nrows <= 0 || nbits <= 0 || nsteps < nbits || !bits || !dibits || !coded_layout_fits(l, nsteps)) return (int)hipErrorInvalidValue;
    const long long nsent = coded_nsent(l, nsteps), ntx = coded_ndibits(l, nsteps);
    if (ntx < 1) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)nrows * (size_t)ntx;
    if ((n + 255) / 256 > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (l.kind == CODED_PLAIN) {
        hipLaunchKernelGGL(conv_encode_kernel, grid, block, 0, s, bits, (size_t)nrows, nbits, nsteps, dibits);
        return (int)hipGetLastError();
    }
    EncodeArgs a = {bits, (size_t)nrows, nbits, (unsigned)nsent, (unsigned)ntx, l.punct, {}, dibits};
    if (!punct_table_make(l.punct, &a.tab)) return (int)hipErrorInvalidValue;
    if (l.kind == CODED_ILV) hipLaunchKernelGGL(conv_encode_ilv_kernel, grid, block, 0, s, a, ilv_mul(l.ilv.n, l.ilv.sinv));
    else hipLaunchKernelGGL(conv_encode_punct_kernel, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
