/*
 * polyphase.hip -- the history the three polyphase stages (channel.hip, synth.hip, resample.hip) carry from push to push.
 *
 * polyphase_history_kernel: per row the last n of (history [n], push [K]) into the OTHER history buffer (the host swaps the two), so that no
 * launch reads what it writes, and a push of K < n values shifts the history.  The banks have one row of n = (P - 1) M values and K = T M;
 * the resampler a row of n = P per stream.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace qpsk {

namespace {

/* a workgroup is 4 rows of 64 lanes: the resampler's rows are short (n = P), the banks' one row is long */
__global__ void __launch_bounds__(256) polyphase_history_kernel(const float2 *__restrict__ hist, const float2 *__restrict__ in, size_t in_pitch, size_t K,
                                                                size_t n, size_t rows, float2 *__restrict__ next)
{
    const size_t row = (size_t)blockIdx.x * 4 + threadIdx.y;
    if (row >= rows) return;
    for (size_t i = (size_t)blockIdx.y * 64 + threadIdx.x; i < n; i += (size_t)gridDim.y * 64) {
        const size_t at = i + K;      /* in (hist, in) */
        next[row * n + i] = at < n ? hist[row * n + at] : in[row * in_pitch + (at - n)];
    }
}

} // namespace

int launch_polyphase_history(const float2 *hist, const float2 *in, size_t in_pitch, size_t K, int rows, size_t n, float2 *next, hipStream_t s)
{
    if (!hist || !in || !next || K < 1 || in_pitch < K || rows < 1 || n < 1 || n > SIZE_MAX / 16 / (size_t)rows) return (int)hipErrorInvalidValue;
    const size_t want = (n + 63) / 64;
    hipLaunchKernelGGL(polyphase_history_kernel, dim3((unsigned)((rows + 3) / 4), (unsigned)(want < 4096 ? want : 4096)), dim3(64, 4), 0, s, hist, in,
                       in_pitch, K, n, (size_t)rows, next);
    return (int)hipGetLastError();
}

} // namespace qpsk
