/*
 * synth.hip -- the polyphase synthesis bank (SYNTHESIS BANK in include/qpsk_hip.h, restated in numpy by tests/test_synth_cpu.py), the
 * channeliser's transmit twin: nsel channel rows in, one wideband complex stream out.  Two launches through a scratch buffer V [T][M] of
 * transformed vectors; polyphase_history_kernel (polyphase.hip) behind them keeps the last P - 1 of those.
 *
 * synth_transform_kernel<NT>: channel_push_kernel's geometry (channel_tile(M) times per workgroup of channel_threads(M) threads) and its LDS
 * image of TB rows of M complex values, element e at e + (e >> 5):
 *   1. the image is zeroed (+0.0: a channel nobody names); behind a barrier the transposed load: TB consecutive times of a selected row are
 *      8 TB contiguous bytes, lanes adjacent in time; row i goes to element bitrev(chan[i]) of every row of the image.  The channels are
 *      distinct, so no two lanes write one element.  Times at or beyond T read the push's last time and are never stored; no address
 *      outside the buffers is formed for them.
 *   2. the transform: channel_fft.h's passes, the ones channel_push_kernel runs.
 *   3. the rows go out in natural order: the tile is TB M contiguous values of V, lanes adjacent in r.
 *
 * synth_filter_kernel<PT>: a lane owns branch r for a run of SYNTH_RUN consecutive times; lanes adjacent in r, so the loads of V and of the
 * taps and the stores of x coalesce.  The run is polyphase.h's (PT = P > 0: taps and window in registers, 8 loads in flight; PT = 0: any
 * P); rows before the push come from the history, rows from 0 on from V, selected without a branch.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channel_fft.h"
#include "kernels.h"
#include "polyphase.h"

namespace qpsk {

namespace {

struct SynthTransformArgs {
    const float2 *in;         /* [nsel] rows, pitch elements apart */
    const float2 *tw;         /* [M / 2] */
    const int32_t *chan;      /* [nsel], distinct */
    float2 *V;                /* [T][M] */
    size_t pitch;
    int T, M, log2m, nsel, tb;
};

template <int NT>
__global__ void __launch_bounds__(NT) synth_transform_kernel(SynthTransformArgs a)
{
    extern __shared__ float2 synth_lds[];
    float2 *v = synth_lds;
    const int tid = threadIdx.x, M = a.M, log2m = a.log2m;
    const int row_pitch = M + (M >> 5) + 1;
    const long long m0 = (long long)blockIdx.x * a.tb;

    /* ---- 1. zeros, then the transposed load */
    for (int e = tid; e < a.tb * row_pitch; e += NT) v[e] = make_float2(0.f, 0.f);
    __syncthreads();
    {
        const int log2tb = __ffs(a.tb) - 1;
        const long long items = (long long)a.nsel << log2tb;
        for (long long item = tid; item < items; item += NT) {
            const int r = (int)(item & (a.tb - 1));
            const long long i = item >> log2tb;
            long long m = m0 + r;
            m = m < a.T ? m : (long long)a.T - 1;
            const int at = channel_phys((int)(__brev((unsigned)a.chan[i]) >> (32 - log2m)));
            v[r * row_pitch + at] = a.in[(size_t)i * a.pitch + (size_t)m];
        }
    }
    __syncthreads();

    /* ---- 2. the transform of every row (channel_fft.h) */
    channel_transform_rows<NT>(v, a.tw, tid, M, log2m, a.tb, row_pitch);

    /* ---- 3. the rows in natural order */
    {
        const long long left = (long long)a.T - m0;
        const int rows = left < a.tb ? (int)left : a.tb;
        float2 *tile = a.V + (size_t)m0 * M;
        for (int item = tid; item < (rows << log2m); item += NT)
            tile[item] = v[(item >> log2m) * row_pitch + channel_phys(item & (M - 1))];
    }
}

struct SynthFilterArgs {
    const float2 *V;          /* [T][M] */
    const float2 *hist;       /* [P - 1][M]: the vectors of times -(P - 1) .. -1 */
    const float *proto;       /* [P][M] */
    float2 *x;                /* [T M] */
    int T, M, log2m, P;
    long long items;          /* runs x M */
};

template <int PT>
__global__ void __launch_bounds__(256) synth_filter_kernel(SynthFilterArgs a)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= a.items) return;
    const int M = a.M, r = (int)(gid & (M - 1));
    const long long m0 = (gid >> a.log2m) * SYNTH_RUN;
    polyphase_branch_run<PT, 8>(
        a.proto, r, M, a.P, 0, SYNTH_RUN, [&](long long t) { return polyphase_at(a.V, a.hist, m0 + t, a.T, a.P, M, r); },
        [&](int t, float2 y) {
            if (m0 + t < a.T) a.x[(size_t)(m0 + t) * M + r] = y;
        });
}

template <int NT>
hipError_t prepare_transform()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(synth_transform_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)channel_lds_bytes(CHANNEL_MAX_M, channel_tile(CHANNEL_MAX_M)));
}

} // namespace

int prepare_synth()
{
    hipError_t e = prepare_transform<256>();
    if (e == hipSuccess) e = prepare_transform<1024>();
    return (int)e;
}

int launch_synth_transform(const float2 *in, size_t pitch, int T, int M, const float2 *tw, const int32_t *chan, int nsel, float2 *V, hipStream_t s)
{
    const int log2m = channel_log2(M);
    if (!in || !tw || !chan || !V || T < 1 || log2m < 0 || nsel < 1 || nsel > M || pitch < (size_t)T || (long long)T * M > SYNTH_MAX_SAMPLES)
        return (int)hipErrorInvalidValue;
    const int tb = channel_tile(M), nt = channel_threads(M);
    if (channel_lds_bytes(M, tb) > (size_t)MAX_LDS_BYTES) return (int)hipErrorInvalidValue;
    const SynthTransformArgs a = {in, tw, chan, V, pitch, T, M, log2m, nsel, tb};
    const unsigned blocks = (unsigned)(((long long)T + tb - 1) / tb);
    if (nt == 256) hipLaunchKernelGGL(synth_transform_kernel<256>, dim3(blocks), dim3(256), channel_lds_bytes(M, tb), s, a);
    else hipLaunchKernelGGL(synth_transform_kernel<1024>, dim3(blocks), dim3(1024), channel_lds_bytes(M, tb), s, a);
    return (int)hipGetLastError();
}

int launch_synth_filter(const float2 *V, const float2 *hist, int T, int M, int P, const float *proto, float2 *x, hipStream_t s)
{
    const int log2m = channel_log2(M);
    if (!V || !proto || !x || T < 1 || log2m < 0 || P < 1 || P > CHANNEL_MAX_P || (P > 1 && !hist) || (long long)T * M > SYNTH_MAX_SAMPLES)
        return (int)hipErrorInvalidValue;
    const long long items = (((long long)T + SYNTH_RUN - 1) / SYNTH_RUN) << log2m;
    const SynthFilterArgs a = {V, hist, proto, x, T, M, log2m, P, items};
    const dim3 blocks((unsigned)((items + 255) / 256)), threads(256);
    if (P == 8) hipLaunchKernelGGL(synth_filter_kernel<8>, blocks, threads, 0, s, a);
    else if (P == 16) hipLaunchKernelGGL(synth_filter_kernel<16>, blocks, threads, 0, s, a);
    else hipLaunchKernelGGL(synth_filter_kernel<0>, blocks, threads, 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
