/*
 * channel.hip -- the polyphase channeliser (CHANNELISER in include/qpsk_hip.h, restated in numpy by tests/test_channel_cpu.py): one wideband
 * complex stream in, M channel rows out, as qpsk_streams_rx_cplx takes them.  s = the history ((P - 1) M samples) followed by the push.
 *
 * channel_push_kernel<PT, NT>: a workgroup of NT threads takes a tile of TB consecutive output times (TB = channel_tile(M), kernels.h) and
 * runs three phases over one LDS image of TB rows of M complex values:
 *   1. branch sums.  The NT threads are G = NT / min(M, NT) groups of min(M, NT) lanes; a group takes R = TB / G consecutive times, a lane
 *      the branches p = lane, lane + NT, ...  Lanes adjacent in p read adjacent samples (reversed), and adjacent taps.  A branch's run of R
 *      times is polyphase.h's (PT = P > 0: taps and window in registers; PT = 0: any P).  u_m[p] goes to row m, element bitrev(p).
 *   2. the transform (channel_fft.h, shared with synth.hip): fft_lds.h's butterflies, inverse sign, fp32.  Two stages per pass over the
 *      LDS: a thread holds the four values i0 + {0, 1, 2, 3} half of stages s and s + 1 and performs the four butterflies of the
 *      definition on them, the operands and the order of every operation as there; an odd log2 M runs stage 1 alone first.
 *   3. the transposed store: TB consecutive times of a selected channel are 8 TB contiguous bytes of its row.
 * Element e of a row lies at e + (e >> 5), rows M + (M >> 5) + 1 elements apart: the strided accesses of the early stages and of the store's
 * column reads spread over the banks.  Times at or beyond T are computed on the push's last block and not stored; no address outside the
 * buffers is formed for them.  Behind the push, polyphase_history_kernel (polyphase.hip) moves the history on.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channel_fft.h"
#include "kernels.h"
#include "polyphase.h"

namespace qpsk {

namespace {

struct ChannelArgs {
    const float2 *x;          /* [T M] */
    const float2 *hist;       /* [(P - 1) M]: the blocks -(P - 1) .. -1 */
    const float *proto;       /* [P M] */
    const float2 *tw;         /* [M / 2] */
    const int32_t *chan;      /* [nsel] */
    float2 *out;              /* [nsel] rows, pitch elements apart */
    size_t pitch;
    int T, M, log2m, P, nsel;
    int tb, run, lanes;       /* the tile, R, min(M, NT) */
};

template <int PT, int NT>
__global__ void __launch_bounds__(NT) channel_push_kernel(ChannelArgs a)
{
    extern __shared__ float2 channel_lds[];
    float2 *v = channel_lds;
    const int tid = threadIdx.x, M = a.M, log2m = a.log2m;
    const int row_pitch = M + (M >> 5) + 1;
    const long long m0 = (long long)blockIdx.x * a.tb;
    constexpr int RUN_UNROLL = NT == 256 ? 8 : 4;      /* new samples a lane has in flight: a run is 32 times at most at 256 threads, 16 at 1024 */

    /* ---- 1. branch sums */
    {
        const int lane = tid & (a.lanes - 1), grp = tid / a.lanes;
        const int r0 = grp * a.run;
        for (int p = lane; p < M; p += NT) {
            const int at = channel_phys((int)(__brev((unsigned)p) >> (32 - log2m)));
            polyphase_branch_run<PT, RUN_UNROLL>(
                a.proto, p, M, a.P, r0, a.run, [&](long long r) { return polyphase_at(a.x, a.hist, m0 + r, a.T, a.P, M, M - 1 - p); },
                [&](int r, float2 u) { v[r * row_pitch + at] = u; });
        }
    }
    __syncthreads();

    /* ---- 2. the transform of every row (channel_fft.h) */
    channel_transform_rows<NT>(v, a.tw, tid, M, log2m, a.tb, row_pitch);

    /* ---- 3. the transposed store */
    {
        const int log2tb = __ffs(a.tb) - 1;
        const long long left = (long long)a.T - m0;
        const int rows = left < a.tb ? (int)left : a.tb;
        const long long items = (long long)a.nsel << log2tb;
        for (long long item = tid; item < items; item += NT) {
            const int r = (int)(item & (a.tb - 1));
            const long long i = item >> log2tb;
            if (r < rows) a.out[(size_t)i * a.pitch + (size_t)(m0 + r)] = v[r * row_pitch + channel_phys(a.chan[i])];
        }
    }
}

template <int PT, int NT>
void launch_push(const ChannelArgs &a, unsigned blocks, hipStream_t s)
{
    hipLaunchKernelGGL((channel_push_kernel<PT, NT>), dim3(blocks), dim3(NT), channel_lds_bytes(a.M, a.tb), s, a);
}

template <int PT, int NT>
hipError_t prepare_push()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(channel_push_kernel<PT, NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)channel_lds_bytes(CHANNEL_MAX_M, channel_tile(CHANNEL_MAX_M)));
}

} // namespace

int prepare_channel()
{
    hipError_t e = prepare_push<0, 256>();
    if (e == hipSuccess) e = prepare_push<8, 256>();
    if (e == hipSuccess) e = prepare_push<16, 256>();
    if (e == hipSuccess) e = prepare_push<0, 1024>();
    if (e == hipSuccess) e = prepare_push<8, 1024>();
    return (int)e;
}

int launch_channel_push(const float2 *x, int T, int M, int P, const float *proto, const float2 *tw, const float2 *hist, const int32_t *chan, int nsel,
                        float2 *out, size_t pitch, hipStream_t s)
{
    const int log2m = channel_log2(M);
    if (!x || !proto || !tw || !chan || !out || T < 1 || log2m < 0 || P < 1 || P > CHANNEL_MAX_P || (P > 1 && !hist) || nsel < 1 ||
        pitch < (size_t)T || (long long)T * M > CHANNEL_MAX_SAMPLES)
        return (int)hipErrorInvalidValue;
    const int tb = channel_tile(M), nt = channel_threads(M);
    const int lanes = M < nt ? M : nt, run = tb / (nt / lanes);
    if (run < 1 || channel_lds_bytes(M, tb) > (size_t)MAX_LDS_BYTES) return (int)hipErrorInvalidValue;
    const ChannelArgs a = {x, hist, proto, tw, chan, out, pitch, T, M, log2m, P, nsel, tb, run, lanes};
    const unsigned blocks = (unsigned)(((long long)T + tb - 1) / tb);
    if (nt == 256) {
        if (P == 8) launch_push<8, 256>(a, blocks, s);
        else if (P == 16) launch_push<16, 256>(a, blocks, s);
        else launch_push<0, 256>(a, blocks, s);
    } else {
        if (P == 8) launch_push<8, 1024>(a, blocks, s);      /* P = 16 would spill under the 128 registers of 1024 threads */
        else launch_push<0, 1024>(a, blocks, s);
    }
    return (int)hipGetLastError();
}

} // namespace qpsk
