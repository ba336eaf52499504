/*
 * soft.hip -- soft decisions and per-row signal quality from costas_frame[] (qpsk_soft_batch; the definition is the contract in
 * include/qpsk_hip.h, restated in numpy by tests/test_soft_cpu.py::soft_ref).
 *
 * NEW DESIGN: the reference has no counterpart (parity unpinned by the reference).  What makes GPU and numpy agree bit
 * for bit is that the ORDER of the fp64 sums is part of the definition: 256 partial sums P[l], l = (i - skip) mod 256, each taking its
 * terms in increasing i, then the tree P[l] += P[l + h], h = 128 .. 1.
 *
 * One workgroup of 256 threads per row in every kernel.  Thread t loads the symbols i = t, t + 256, ... (8-byte loads, a wave reads 512
 * contiguous bytes), so it owns the partial l = (t - skip) & 255 and meets its terms in increasing i.  The tree: the partials go to LDS
 * at their l; lane l < 64 of wave 0 takes (P[l] + P[l+128]) + (P[l+64] + P[l+192]) -- the steps h = 128 and h = 64 -- and the steps
 * h = 32 .. 1 are shuffles (v += shfl_down(v, h): lane l < h reads lane l + h, the lanes above compute values nobody reads).
 *
 *   soft_onepass_kernel   nsym <= SOFT_ONE_PASS_MAX, sums and soft output both wanted: the row is staged in LDS while it is summed
 *                         (8 nsym bytes), lane 0 turns the sums into the quality figures and the gain (or takes the caller's), the gain is
 *                         broadcast through LDS and the int8 pairs are written from the staged row: every row is read from memory ONCE
 *   soft_sums_kernel      sums only (no soft output wanted, or the first pass of a longer row): quality, sums, and the gain into a
 *                         scratch array
 *   soft_apply_kernel     soft output from a gain per row that is already in memory (the second pass of a longer row, or the caller's
 *                         d_gain_in with no quality output: then nothing is summed at all); reads the payload only
 *
 * Soft output: two output symbols (4 bytes) per lane and store -- a wave writes 256 contiguous bytes; a row whose output starts on an
 * odd 2-byte boundary (odd nout) has its first symbol peeled, an odd remainder is a tail symbol (the caller has checked that the array itself
 * is 2-byte aligned).  A lag that would leave the row is never used as an address: that row's output is zeros and the status word
 * receives STATUS_SOFT_BAD_LAG.  Non-finite samples: the sums turn non-finite (fp64 cannot overflow on 2^21 finite floats), the payload
 * is looked at where it is loaded; either stores STATUS_SOFT_NONFINITE.  Vector stores only.
 */
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "kernels.h"
#include "soft_quant.h"

namespace qpsk {

namespace {

constexpr int WG = 256;            /* threads per workgroup = partial sums of the definition */
constexpr int UNROLL = 8;          /* loads in flight per thread while summing */
constexpr int APPLY_PAIRS = 4;     /* soft_apply_kernel: pairs of output symbols per thread (2048 symbols per workgroup) */

struct Sums {
    double s1, s2, s4, sq;
};

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= DBL_MAX; }

/* one symbol's terms (qpsk_hip.h): t1 = |a| + |b|, t2 = p, t4 = p p, tq = Re z^4, fp64 on the widened floats, nothing fused */
__device__ __forceinline__ void add_terms(Sums &P, float2 z)
{
    const double a = (double)z.x, b = (double)z.y;
    const double aa = a * a, bb = b * b;
    const double p = aa + bb;
    const double sr = aa - bb;
    const double si = 2.0 * (a * b);
    P.s1 += fabs(a) + fabs(b);
    P.s2 += p;
    P.s4 += p * p;
    P.sq += sr * sr - si * si;
}

/* thread tid's partial over the symbols i = tid (mod 256), skip <= i < nsym, in increasing i; STAGE: every symbol of the row also
 * goes to stage[i] (LDS), the ones before skip included */
template <bool STAGE>
__device__ __forceinline__ Sums sum_row(const float2 *__restrict__ row, int nsym, int skip, int tid, float2 *stage)
{
    Sums P = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = STAGE ? 0 : (skip / WG) * WG; i0 < nsym; i0 += WG * UNROLL) {
        float2 z[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int i = i0 + WG * u + tid;
            z[u] = i < nsym ? row[i] : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int i = i0 + WG * u + tid;
            if (i < nsym) {
                if (STAGE) stage[i] = z[u];
                if (i >= skip) add_terms(P, z[u]);
            }
        }
    }
    return P;
}

/* the tree over the 256 partials; the sums are valid in thread 0.  red: [4][WG] doubles of LDS.  Ends without a barrier */
__device__ __forceinline__ Sums fold(const Sums &P, int l, int tid, double *red)
{
    red[0 * WG + l] = P.s1;
    red[1 * WG + l] = P.s2;
    red[2 * WG + l] = P.s4;
    red[3 * WG + l] = P.sq;
    __syncthreads();
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid < 64) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double *r = red + q * WG + tid;
            v[q] = (r[0] + r[128]) + (r[64] + r[192]);
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) v[q] += __shfl_down(v[q], h, 64);
        }
    }
    return Sums{v[0], v[1], v[2], v[3]};
}

__device__ __forceinline__ float gain_of(double num, double den)      /* (float)min(num / den, FLT_MAX), den > 0 */
{
    double g = num / den;
    if (g > (double)FLT_MAX) g = (double)FLT_MAX;
    return (float)g;
}

/* thread 0: the sums of one row -> the quality figures, the sums themselves and the gain (qpsk_hip.h) */
__device__ __forceinline__ float finish_row(const Sums &S, int m, int mode, float scale, float *quality, double *sums, int *status)
{
    const double dm = (double)m;
    const double M2 = S.s2 / dm, M4 = S.s4 / dm;
    const double D = 2.0 * M2 * M2 - M4;
    const double Ps = D > 0.0 ? sqrt(D) : 0.0;
    const double Pn = M2 - Ps;
    const double amp = S.s1 / (2.0 * dm);
    if (quality) {
        quality[0] = (float)amp;
        quality[1] = Pn > 0.0 ? (float)(Ps / Pn) : 0.0f;
        quality[2] = S.s4 > 0.0 ? (float)(-S.sq / S.s4) : 0.0f;
        quality[3] = (float)((Pn > 0.0 ? Pn : 0.0) / 2.0);
    }
    if (sums) {
        sums[0] = S.s1;
        sums[1] = S.s2;
        sums[2] = S.s4;
        sums[3] = S.sq;
    }
    if (__builtin_expect(!finite_d(S.s2), 0) && status)
        __hip_atomic_store(status, STATUS_SOFT_NONFINITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (mode == SOFT_MODE_LLR && Pn > 0.0) return gain_of(2.0 * sqrt(Ps / 2.0) / (Pn / 2.0), (double)scale);
    const double target = mode == SOFT_MODE_LLR ? 127.0 : (double)scale;
    return amp > 0.0 ? gain_of(target, amp) : 0.0f;
}

/*
 * The soft output of one row, pairs [p0, p1) of it by this workgroup's threads (pair p = output symbols head + 2 p, head + 2 p + 1; the
 * peeled head symbol and the tail symbol by thread 0 of the workgroup with p0 == 0).  src: the row (LDS or memory), already advanced
 * to the payload's first symbol, or NULL for a row whose lag was refused (zeros).  Returns whether a non-finite sample was loaded.
 */
__device__ __forceinline__ bool write_soft(const float2 *src, int8_t *out, int nout, int r, float g, int p0, int p1, int tid)
{
    bool bad = false;
    const int head = nout > 0 ? (int)(((uintptr_t)out >> 1) & 1) : 0;
    const int npairs = (nout - head) >> 1;
    for (int p = p0 + tid; p < min(p1, npairs); p += WG) {
        const int o = head + 2 * p;
        unsigned w = 0u;
        if (src) w = soft_pair(src[o], r, g, bad) | (soft_pair(src[o + 1], r, g, bad) << 16);
        *reinterpret_cast<unsigned *>(out + 2 * (size_t)o) = w;
    }
    if (p0 == 0 && tid == 0) {
        if (head) *reinterpret_cast<unsigned short *>(out) = (unsigned short)(src ? soft_pair(src[0], r, g, bad) : 0u);
        if ((nout - head) & 1)
            *reinterpret_cast<unsigned short *>(out + 2 * (size_t)(nout - 1)) = (unsigned short)(src ? soft_pair(src[nout - 1], r, g, bad) : 0u);
    }
    return bad;
}

/* the payload's first symbol in row `row`, or -1 for a lag that would leave the row (flagged, never an address) */
__device__ __forceinline__ int payload_base(const int32_t *lag, int row, int first, int nout, int nsym, int *status)
{
    const long long L = lag ? (long long)lag[row] : 0;
    if (L < 0 || L + first + nout > nsym) {
        if (status) __hip_atomic_store(status, STATUS_SOFT_BAD_LAG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return -1;
    }
    return (int)L + first;
}

__global__ void __launch_bounds__(WG)
soft_onepass_kernel(const float2 *__restrict__ x, size_t pitch, int nsym, int skip, int mode, float scale, const float *__restrict__ gain_in,
                    const int32_t *__restrict__ lag, const int32_t *__restrict__ rot, int first, int nout, int8_t *__restrict__ soft, float *__restrict__ quality,
                    double *__restrict__ sums, int *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double red[4 * WG];
    __shared__ float gain;
    float2 *stage = reinterpret_cast<float2 *>(smem);      /* [nsym] */
    const int tid = threadIdx.x, row = blockIdx.x;
    const Sums P = sum_row<true>(x + (size_t)row * pitch, nsym, skip, tid, stage);
    const Sums S = fold(P, (tid - skip) & (WG - 1), tid, red);
    bool bad = false;
    if (tid == 0) {
        const float g = finish_row(S, nsym - skip, mode, scale, quality ? quality + 4 * (size_t)row : nullptr,
                                   sums ? sums + 4 * (size_t)row : nullptr, status);
        gain = gain_in ? gain_in[row] : g;      /* the caller's own gain replaces the row's */
        bad = !finite_f(gain);
    }
    __syncthreads();      /* the gain, and every thread's part of the staged row */
    const int base = payload_base(lag, row, first, nout, nsym, status);
    const int r = rot ? rot[row] & 3 : 0;
    bad |= write_soft(base >= 0 ? stage + base : nullptr, soft + 2 * (size_t)row * (size_t)nout, nout, r, gain, 0, (nout + 1) / 2, tid);
    if (__builtin_expect(bad, 0) && status) __hip_atomic_store(status, STATUS_SOFT_NONFINITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(WG)
soft_sums_kernel(const float2 *__restrict__ x, size_t pitch, int nsym, int skip, int mode, float scale, float *__restrict__ gain_out,
                 float *__restrict__ quality, double *__restrict__ sums, int *status)
{
    __shared__ double red[4 * WG];
    const int tid = threadIdx.x, row = blockIdx.x;
    const Sums P = sum_row<false>(x + (size_t)row * pitch, nsym, skip, tid, nullptr);
    const Sums S = fold(P, (tid - skip) & (WG - 1), tid, red);
    if (tid == 0) {
        const float g = finish_row(S, nsym - skip, mode, scale, quality ? quality + 4 * (size_t)row : nullptr,
                                   sums ? sums + 4 * (size_t)row : nullptr, status);
        if (gain_out) gain_out[row] = g;
    }
}

/* workgroup b: chunk b % nchunks of row b / nchunks */
__global__ void __launch_bounds__(WG)
soft_apply_kernel(const float2 *__restrict__ x, size_t pitch, int nsym, int nchunks, const float *__restrict__ gain, int check_gain,
                  const int32_t *__restrict__ lag, const int32_t *__restrict__ rot, int first, int nout, int8_t *__restrict__ soft, int *status)
{
    const int tid = threadIdx.x;
    const int row = (int)(blockIdx.x / (unsigned)nchunks), chunk = (int)(blockIdx.x % (unsigned)nchunks);
    const float g = gain[row];
    const int base = payload_base(lag, row, first, nout, nsym, status);
    const int r = rot ? rot[row] & 3 : 0;
    const int p0 = chunk * (WG * APPLY_PAIRS);
    bool bad = write_soft(base >= 0 ? x + (size_t)row * pitch + base : nullptr, soft + 2 * (size_t)row * (size_t)nout, nout, r, g, p0,
                          p0 + WG * APPLY_PAIRS, tid);
    if (check_gain) bad |= !finite_f(g);      /* the caller's own gain */
    if (__builtin_expect(bad, 0) && status) __hip_atomic_store(status, STATUS_SOFT_NONFINITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

} // namespace

int soft_one_pass_max(void) { return SOFT_ONE_PASS_MAX; }

int launch_soft_onepass(const float *x, size_t pitch, int nrows, int nsym, int skip, int mode, float scale, const float *gain_in,
                        const int32_t *lag, const int32_t *rot, int first, int nout, int8_t *soft, float *quality, double *sums, int *status, hipStream_t s)
{
    if (nrows <= 0 || nsym <= 0 || nsym > SOFT_ONE_PASS_MAX || !soft) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(soft_onepass_kernel, dim3(nrows), dim3(WG), sizeof(float2) * (size_t)nsym, s, reinterpret_cast<const float2 *>(x), pitch,
                       nsym, skip, mode, scale, gain_in, lag, rot, first, nout, soft, quality, sums, status);
    return (int)hipGetLastError();
}

int launch_soft_sums(const float *x, size_t pitch, int nrows, int nsym, int skip, int mode, float scale, float *gain_out, float *quality,
                     double *sums, int *status, hipStream_t s)
{
    if (nrows <= 0 || nsym <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(soft_sums_kernel, dim3(nrows), dim3(WG), 0, s, reinterpret_cast<const float2 *>(x), pitch, nsym, skip, mode, scale,
                       gain_out, quality, sums, status);
    return (int)hipGetLastError();
}

int launch_soft_apply(const float *x, size_t pitch, int nrows, int nsym, const float *gain, bool check_gain, const int32_t *lag,
                      const int32_t *rot, int first, int nout, int8_t *soft, int *status, hipStream_t s)
{
    if (nrows <= 0 || nsym <= 0 || !soft || !gain) return (int)hipErrorInvalidValue;
    const int per = 2 * WG * APPLY_PAIRS;                       /* output symbols per workgroup */
    const int nchunks = nout > 0 ? (nout + per - 1) / per : 1;  /* the pairs of a peeled row still fit: (nout - 1) / 2 <= per / 2 * nchunks */
    const long long blocks = (long long)nrows * nchunks;
    if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(soft_apply_kernel, dim3((unsigned)blocks), dim3(WG), 0, s, reinterpret_cast<const float2 *>(x), pitch, nsym, nchunks, gain,
                       check_gain ? 1 : 0, lag, rot, first, nout, soft, status);
    return (int)hipGetLastError();
}

} // namespace qpsk
