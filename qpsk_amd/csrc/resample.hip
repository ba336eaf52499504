/*
 * resample.hip -- the batched polyphase rational resampler (RESAMPLER in include/qpsk_hip.h, restated in numpy by tests/test_resample_cpu.py):
 * nstreams rows in at one rate, the same rows out at L / D of it.  Per stream s = the history (the last P consumed samples) followed by the
 * push; sample index i counts from the push's first sample, so the history is i = -P .. -1.
 *
 * resample_push_kernel<PT, STAGED>: a workgroup of 256 threads takes one stream and a tile of RESAMPLE_TILE = 256 consecutive outputs, one
 * output per lane.  The L P taps are copied into LDS as they lie (h[q L + b]: lanes adjacent in n differ by D mod L in b).  Output n of the
 * push: tt = r + L + n D (positive, below 2^31: the host checks), i = tt / L - 1, b = tt mod L, unsigned 32-bit with the wave-uniform
 * divisor L; then acc = fl(h[b] s[i]), acc = acc + fl(h[q L + b] s[i - q]), q = 1 .. P - 1, real and imaginary part apart.
 *   STAGED: the tile's window s[i0 .. i_last], i0 = i(first output) - (P - 1), at most resample_window(L, D, P) samples, is loaded once,
 *     coalesced, into LDS behind the taps; every output reads its P samples there.
 *   direct: the window would not fit (strong decimation: adjacent outputs share few inputs or none), every lane loads its P samples from
 *     global memory or the history.
 *   PT = P > 0: the taps loop is unrolled (8 and 16); PT = 0: any P.
 * No address outside the buffers is formed: i <= K - 1 = nin - 1 for the push's last output (the host has refused any other nin), i - q >= -P,
 * and lanes beyond nout do nothing after the barrier.
 *
 * Behind the push, polyphase_history_kernel (polyphase.hip) moves the history on, n = P per stream; a push with K = 0 launches none and
 * swaps nothing.  The tap loop is not polyphase.h's: an output has its own branch b and no neighbour in time to share a window with.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace qpsk {

namespace {

struct ResampleArgs {
    const float2 *in;         /* [nstreams] rows of nin, in_pitch apart; never read when nin = 0 */
    const float2 *hist;       /* [nstreams][P] */
    const float *proto;       /* [L P] */
    float2 *out;              /* [nstreams] rows of nout, out_pitch apart */
    size_t in_pitch, out_pitch;
    int nout, L, D, P;
    unsigned tt;              /* r + L of the push: 0 < tt < D + L */
    unsigned tiles;           /* per stream */
};

template <int PT, bool STAGED>
__global__ void __launch_bounds__(RESAMPLE_TILE) resample_push_kernel(ResampleArgs a)
{
    extern __shared__ float resample_lds[];
    float *taps = resample_lds;
    const int tid = threadIdx.x;
    const int P = PT > 0 ? PT : a.P;
    const int ntaps = a.L * P;
    const unsigned L = (unsigned)a.L, D = (unsigned)a.D;
    const unsigned tile = blockIdx.x % a.tiles;
    const size_t stream = blockIdx.x / a.tiles;
    const int n0 = (int)tile * RESAMPLE_TILE;
    const int left = a.nout - n0, cnt = left < RESAMPLE_TILE ? left : RESAMPLE_TILE;
    const float2 *in = a.in + stream * a.in_pitch;
    const float2 *hist = a.hist + stream * (size_t)P;
    const unsigned tt0 = a.tt + (unsigned)n0 * D;
    const int i0 = (int)(tt0 / L) - P;      /* the window's first sample: i(output n0) - (P - 1) */

    for (int j = tid; j < ntaps; j += RESAMPLE_TILE) taps[j] = a.proto[j];
    float2 *win = reinterpret_cast<float2 *>(taps + ((ntaps + 1) & ~1));
    if constexpr (STAGED) {
        const unsigned ttl = tt0 + (unsigned)(cnt - 1) * D;
        const int W = (int)(ttl / L) - 1 - i0 + 1;
        for (int j = tid; j < W; j += RESAMPLE_TILE) {
            const int idx = i0 + j;
            win[j] = idx < 0 ? hist[P + idx] : in[idx];
        }
    }
    __syncthreads();
    if (tid >= cnt) return;

    const unsigned tt = tt0 + (unsigned)tid * D;
    const unsigned i1 = tt / L, b = tt - i1 * L;
    const int i = (int)i1 - 1;
    auto sample = [&](int q) -> float2 {
        const int idx = i - q;
        if constexpr (STAGED) return win[idx - i0];
        else return idx < 0 ? hist[P + idx] : in[idx];
    };
    const float2 x0 = sample(0);
    const float h0 = taps[b];
    float accr = h0 * x0.x, acci = h0 * x0.y;
    if constexpr (PT > 0) {
        float2 x[PT];
        float h[PT];
#pragma unroll
        for (int q = 1; q < PT; q++) {
            x[q] = sample(q);
            h[q] = taps[(unsigned)q * L + b];
        }
#pragma unroll
        for (int q = 1; q < PT; q++) {
            accr = accr + h[q] * x[q].x;
            acci = acci + h[q] * x[q].y;
        }
    } else {
#pragma unroll 4
        for (int q = 1; q < P; q++) {
            const float2 xq = sample(q);
            const float hq = taps[(unsigned)q * L + b];
            accr = accr + hq * xq.x;
            acci = acci + hq * xq.y;
        }
    }
    a.out[stream * a.out_pitch + (size_t)(n0 + tid)] = make_float2(accr, acci);
}

template <int PT, bool STAGED>
void launch_push(const ResampleArgs &a, unsigned blocks, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL((resample_push_kernel<PT, STAGED>), dim3(blocks), dim3(RESAMPLE_TILE), lds, s, a);
}

template <int PT, bool STAGED>
hipError_t prepare_push()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(resample_push_kernel<PT, STAGED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(RESAMPLE_MAX_L * RESAMPLE_MAX_P * sizeof(float) + (STAGED ? RESAMPLE_WIN_MAX * sizeof(float2) : 0)));
}

} // namespace

int prepare_resample()
{
    hipError_t e = prepare_push<0, true>();
    if (e == hipSuccess) e = prepare_push<8, true>();
    if (e == hipSuccess) e = prepare_push<16, true>();
    if (e == hipSuccess) e = prepare_push<0, false>();
    if (e == hipSuccess) e = prepare_push<8, false>();
    if (e == hipSuccess) e = prepare_push<16, false>();
    return (int)e;
}

int launch_resample_push(const float2 *in, size_t in_pitch, int nin, const float2 *hist, const float *proto, int nstreams, int L, int D, int P, int r,
                         int nout, float2 *out, size_t out_pitch, hipStream_t s)
{
    if (!hist || !proto || !out || nstreams < 1 || nstreams > RESAMPLE_MAX_STREAMS || L < 1 || L > RESAMPLE_MAX_L || D < 1 ||
        D > RESAMPLE_MAX_D || P < 1 || P > RESAMPLE_MAX_P || (r != 0 && r < D - L) || r >= D || nout < 1 || nout > RESAMPLE_MAX_OUT ||
        (long long)nout * D + L >= (1ll << 31) || out_pitch < (size_t)nout)
        return (int)hipErrorInvalidValue;
    /* the one nin the position allows: the kernel's reads end at K - 1 */
    const long long last = (long long)r + (long long)(nout - 1) * D;
    const long long K = (last >= 0 ? last / L : -((-last + L - 1) / L)) + 1;
    if (nin != K || (nin > 0 && (!in || in_pitch < (size_t)nin))) return (int)hipErrorInvalidValue;
    const long long tiles = ((long long)nout + RESAMPLE_TILE - 1) / RESAMPLE_TILE;
    if (tiles * nstreams > 0x7fffffffll) return (int)hipErrorInvalidValue;
    const bool staged = resample_staged(L, D, P);
    const size_t lds = resample_lds_bytes(L, D, P, staged);
    if (lds > (size_t)MAX_LDS_BYTES) return (int)hipErrorInvalidValue;
    const ResampleArgs a = {in ? in : hist, hist, proto, out, in_pitch, out_pitch, nout, L, D, P, (unsigned)(r + L), (unsigned)tiles};
    const unsigned blocks = (unsigned)(tiles * nstreams);
    if (staged) {
        if (P == 8) launch_push<8, true>(a, blocks, lds, s);
        else if (P == 16) launch_push<16, true>(a, blocks, lds, s);
        else launch_push<0, true>(a, blocks, lds, s);
    } else {
        if (P == 8) launch_push<8, false>(a, blocks, lds, s);
        else if (P == 16) launch_push<16, false>(a, blocks, lds, s);
        else launch_push<0, false>(a, blocks, lds, s);
    }
    return (int)hipGetLastError();
}

} // namespace qpsk
