/*
 * carrier_est.hip -- coarse carrier estimate from the fourth-power spectral line (qpsk_carrier_est_batch).
 *
 * NEW DESIGN: the reference has no carrier estimate of its own (README.md: "there also needs to be a frequency error adjustment";
 * its answer is the Costas loop alone).  What is pinned to the reference is the filter (rrc_fir.c:17-30) and the transform
 * (fft.c:110-120, forward, scaled 1/n); the steps between and after them are this library's own (parity unpinned by the reference,
 * DESIGN.md), checked against the oracle restatement tests/test_carrier_est_cpu.py::oracle_carrier_est.  Per frame x:
 *
 *   y[0 .. start+n-1] = rrc_fir() of x[0 .. start+n-1], fresh delay line                        (rrc_fir.c:17-30)
 *   z[m]  = y[start+m]^4 in fp64, unfused: s = (a a - b b, 2 (a b)), z = (s.re s.re - s.im s.im, 2 (s.re s.im))
 *   X     = fftn(z, n)                                                                          (fft.c:110-120)
 *   S     = { k : |k| < n / (2 CYCLES), min_freq <= w(k) <= max_freq },  w(k) = (float)(TAU (k CYCLES) / (4 n))
 *   k*    = the k in S with the largest |X[k mod n]|^2 (fp64, unfused); ties: smaller |k|, then smaller k
 *   outputs w(k*), the seed (0, w(k*)), k*, X[k*]
 *
 * QPSK modulation is removed by the fourth power and a carrier offset df leaves a line at 4 df; |w| < pi/4 keeps the symbol-rate
 * sidebands of y^4 (at 4 df +- RS) out of S for every |df| < RS / 8.
 *
 * ONE WORKGROUP PER FRAME, W = min(4, n / 512) waves:
 *   - the filter is the generated full-rate stream of timing_fft.hip (fir_full8s_asm.h with the taps in SGPRs for a symmetric filter,
 *     fir_full8_asm.h with the taps in LDS otherwise): one pass = 512 consecutive outputs of one wave, from a window of 638 samples
 *     staged sample by sample (any start, alignment or pitch; samples before 0 are the fresh delay line's zeros, samples past
 *     start + n - 1 are never read).  Wave w takes passes w, w + W, ...;
 *   - each lane turns its 8 outputs into y^4 in fp64 registers and writes them bit-reversed into the frame's n-point array in LDS
 *     (fft.c:99-101 + the recursion's even/odd order, as fft_kernel does);
 *   - the butterflies are fft_lds_stages() (fft_lds.h), the scaling fft.c:117-119's division by n;
 *   - the argmax runs over S only (a contiguous range of k: w(k) is monotone), a wave reduction with shuffles and one across waves.
 * LDS: 16 n bytes for the array + 6.3 KB per wave for its window (n = 8192, W = 4: 154 KB of gfx950's 160 KB).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qpsk_device.h"
#include "costas_asm.h"      /* lds_addr() */
#include "fir_full8_asm.h"
#include "fir_full8s_asm.h"
#include "timing_fft_wave.h" /* the stream's window image (slot_of, R, PADS, WSLOTS), wave_sync() */
#include "fft_lds.h"
#include "kernels.h"

namespace qpsk {

namespace cest {
constexpr int PASS = 512;            /* outputs per wave pass of the stream */
constexpr int WPOS = PASS + HIST;    /* window positions of one pass: position q = sample (first output) - HIST + q */
}

/* (p, k) is a better maximum than (bp, bk): larger power; equal power: smaller |k|, then smaller k.  A NaN power never wins */
__device__ __forceinline__ bool est_better(double p, int k, double bp, int bk)
{
    if (p > bp) return true;
    if (p == bp) {
        const int ak = k < 0 ? -k : k, abk = bk < 0 ? -bk : bk;
        return ak < abk || (ak == abk && k < bk);
    }
    return false;
}

template <int W, bool SYM>
__global__ void __launch_bounds__(64 * W)
carrier_est_kernel(const float *__restrict__ x, size_t pitch, int nframes, int start, int n, int log2n, int cycles, int klo,
                   int khi, int kdef, const float *__restrict__ taps_g, const double2 *__restrict__ tw, float2 *seed, float *freq,
                   int32_t *bin, double2 *line, int *status)
{
    using namespace cest;
    using tfft::R;
    using tfft::PADS;
    using tfft::WSLOTS;
    using tfft::slot_of;
    using tfft::wave_sync;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ __attribute__((aligned(16))) float taps[SYM ? 4 : 128];
    __shared__ double red_p[W];
    __shared__ int red_k[W];
    double2 *vv = reinterpret_cast<double2 *>(smem);                                  /* [n] the transform, bit-reversed in */
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2 *win = reinterpret_cast<float2 *>(smem + (size_t)n * sizeof(double2)) + wave * WSLOTS;
    const int f = blockIdx.x;
    if (f >= nframes) return;
    if (!SYM) {
        for (int i = tid; i < 128; i += 64 * W) taps[i] = i < NTAPS ? taps_g[i] : 0.0f;      /* all 128 entries whatever W */
        __syncthreads();
    }
    const float *src = x + 2 * (size_t)f * pitch;
    const int last = start + n - 1;                                                   /* the last sample the estimate depends on */
    const unsigned rd_addr = lds_addr(win + (R + PADS) * lane);
    const unsigned tap_addr = lds_addr(taps);
    const int npass = (n + PASS - 1) / PASS;
    bool bad = false;
    for (int p = wave; p < npass; p += W) {
        /* the window of outputs start + 512 p .. + 511: zeros before sample 0 (fresh delay line) and past `last` (never used) */
        const int base = start + PASS * p - HIST;
#pragma unroll
        for (int j = 0; j < (WPOS + 63) / 64; j++) {
            const int q = lane + 64 * j;
            if (q < WPOS) {
                const int s = base + q;
                float re = 0.0f, im = 0.0f;
                if (s >= 0 && s <= last) {
                    re = src[2 * (size_t)s];
                    im = src[2 * (size_t)s + 1];
                    bad |= !(fabsf(re) <= 3.402823466e+38f) || !(fabsf(im) <= 3.402823466e+38f);
                }
                win[slot_of(q)] = make_float2(re, im);
            }
        }
        wave_sync();
        v2f a0, a1, a2, a3, a4, a5, a6, a7;
        if constexpr (SYM) fir_full8s_asm(rd_addr, taps_g, a0, a1, a2, a3, a4, a5, a6, a7);
        else fir_full8_asm(rd_addr, tap_addr, a0, a1, a2, a3, a4, a5, a6, a7);   /* both end with every LDS read returned */
        wave_sync();                                                                   /* the next pass's staging overwrites the window */
        const v2f acc[R] = {a0, a1, a2, a3, a4, a5, a6, a7};
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int m = PASS * p + R * lane + r;                                    /* z[m] = y[start + m]^4 */
            const float2 y = fir_gain(make_float2(acc[r].x, acc[r].y));              /* rrc_fir.c:28 */
            const double a = (double)y.x, b = (double)y.y;
            const double sr = a * a - b * b;
            const double si = 2.0 * (a * b);
            const double zr = sr * sr - si * si;
            const double zi = 2.0 * (sr * si);
            if (m < n) vv[__brev((unsigned)m) >> (32 - log2n)] = make_double2(zr, zi);
        }
    }
    if (__builtin_expect(bad, 0) && status)
        __hip_atomic_store(status, STATUS_EST_NONFINITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    fft_lds_stages(vv, tw, n, log2n, tid, 64 * W, -1.0);                              /* fft.c:38-64, forward; ends with a barrier */

    /* argmax over S = [klo, khi] of |X[k mod n]|^2, X = the array / n (fft.c:117-119) */
    const double dn = (double)n;
    double bp = -1.0;                                                                 /* below every power: kdef (in S) only if all are NaN */
    int bk = kdef;
    for (int k = klo + tid; k <= khi; k += 64 * W) {
        const double2 v = vv[k & (n - 1)];
        const double xr = v.x / dn, xi = v.y / dn;
        const double pw = xr * xr + xi * xi;
        if (est_better(pw, k, bp, bk)) { bp = pw; bk = k; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double op = __shfl_xor(bp, d);
        const int ok = __shfl_xor(bk, d);
        if (est_better(op, ok, bp, bk)) { bp = op; bk = ok; }
    }
    if (W > 1) {
        if (lane == 0) { red_p[wave] = bp; red_k[wave] = bk; }
        __syncthreads();
    }
    if (tid == 0) {
        for (int w = 1; w < W; w++)
            if (est_better(red_p[w], red_k[w], bp, bk)) { bp = red_p[w]; bk = red_k[w]; }
        const double2 v = vv[bk & (n - 1)];
        const float om = (float)(TAU * (double)(bk * cycles) / (double)(4 * n));
        if (seed) seed[f] = make_float2(0.0f, om);
        if (freq) freq[f] = om;
        if (bin) bin[f] = bk;
        if (line) line[f] = make_double2(v.x / dn, v.y / dn);
    }
}

template <int W>
static size_t carrier_est_lds(int n) { return (size_t)n * sizeof(double2) + (size_t)W * tfft::WSLOTS * sizeof(float2); }

int prepare_carrier_est(void)
{
    const void *k[] = {
        reinterpret_cast<const void *>(carrier_est_kernel<1, true>), reinterpret_cast<const void *>(carrier_est_kernel<2, true>),
        reinterpret_cast<const void *>(carrier_est_kernel<4, true>), reinterpret_cast<const void *>(carrier_est_kernel<1, false>),
        reinterpret_cast<const void *>(carrier_est_kernel<2, false>), reinterpret_cast<const void *>(carrier_est_kernel<4, false>),
    };
    for (const void *p : k) {
        const hipError_t e = hipFuncSetAttribute(p, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS_BYTES - 1024);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

int launch_carrier_est(const float *x, size_t pitch, int nframes, int start, int n, int cycles, int klo, int khi, int kdef,
                       const float *taps, const double *tw, float *seed, float *freq, int32_t *bin, double *line, int *status,
                       bool symmetric, hipStream_t s)
{
    if (n < 64 || n > 8192 || (n & (n - 1)) || nframes <= 0) return (int)hipErrorInvalidValue;
    int log2n = 0;
    while ((1 << log2n) < n) log2n++;
    const int npass = (n + cest::PASS - 1) / cest::PASS;
    const double2 *tw2 = reinterpret_cast<const double2 *>(tw);
    auto go = [&](auto kern, size_t lds, int W) {
        hipLaunchKernelGGL(kern, dim3(nframes), dim3(64 * W), lds, s, x, pitch, nframes, start, n, log2n, cycles, klo, khi, kdef, taps,
                           tw2, reinterpret_cast<float2 *>(seed), freq, bin, reinterpret_cast<double2 *>(line), status);
    };
    if (symmetric) {
        if (npass >= 4) go(carrier_est_kernel<4, true>, carrier_est_lds<4>(n), 4);
        else if (npass == 2) go(carrier_est_kernel<2, true>, carrier_est_lds<2>(n), 2);
        else go(carrier_est_kernel<1, true>, carrier_est_lds<1>(n), 1);
    } else {
        if (npass >= 4) go(carrier_est_kernel<4, false>, carrier_est_lds<4>(n), 4);
        else if (npass == 2) go(carrier_est_kernel<2, false>, carrier_est_lds<2>(n), 2);
        else go(carrier_est_kernel<1, false>, carrier_est_lds<1>(n), 1);
    }
    return (int)hipGetLastError();
}

} // namespace qpsk
