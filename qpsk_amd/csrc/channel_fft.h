/*
 * channel_fft.h -- the transform passes of the two filter banks (CHANNELISER and SYNTHESIS BANK in include/qpsk_hip.h), written once:
 * channel_push_kernel (channel.hip) and synth_transform_kernel (synth.hip) run them over the same LDS image of TB rows of M complex values.
 * Element e of a row lies at channel_phys(e) = e + (e >> 5), rows row_pitch = M + (M >> 5) + 1 elements apart.  The butterflies are
 * fft_lds.h's with the inverse sign, fp32, the operands and the order of every operation as the header's definition states them.
 */
#ifndef QPSK_CHANNEL_FFT_H
#define QPSK_CHANNEL_FFT_H

#include <hip/hip_runtime.h>

namespace qpsk {

__device__ __forceinline__ int channel_phys(int e) { return e + (e >> 5); }

__device__ __forceinline__ void channel_butterfly(const float2 w, const float2 e, const float2 o, float2 &lo, float2 &hi)
{
    const float zr = w.x * o.x - w.y * o.y;
    const float zi = w.x * o.y + w.y * o.x;
    lo = make_float2(e.x + zr, e.y + zi);
    hi = make_float2(e.x - zr, e.y - zi);
}

/* stages 1 .. log2 M on the tb rows of v, which hold the input in bit-reversed order and the output in natural order.  Two stages per
 * pass over the LDS: a thread holds the four values i0 + {0, 1, 2, 3} half of stages s and s + 1 and performs the four butterflies of the
 * definition on them; an odd log2 M runs stage 1 alone first.  Every thread of the workgroup calls it behind a barrier; a barrier ends
 * every pass, the last one included */
template <int NT>
__device__ __forceinline__ void channel_transform_rows(float2 *v, const float2 *tw, int tid, int M, int log2m, int tb, int row_pitch)
{
    int s = 1;
    if (log2m & 1) {      /* stage 1 alone: half = 1, k = 0 */
        const float2 w = tw[0];
        const int per_row = M >> 1;
        for (int item = tid; item < tb * per_row; item += NT) {
            float2 *row = v + (item >> (log2m - 1)) * row_pitch;
            const int lo = channel_phys(2 * (item & (per_row - 1))), hi = channel_phys(2 * (item & (per_row - 1)) + 1);
            float2 c0, c1;
            channel_butterfly(w, row[lo], row[hi], c0, c1);
            row[lo] = c0;
            row[hi] = c1;
        }
        __syncthreads();
        s = 2;
    }
    for (; s < log2m; s += 2) {      /* stages s and s + 1 */
        const int half = 1 << (s - 1), per_row = M >> 2;
        for (int item = tid; item < tb * per_row; item += NT) {
            float2 *row = v + (item >> (log2m - 2)) * row_pitch;
            const int j = item & (per_row - 1);
            const int k = j & (half - 1);
            const int i0 = ((j >> (s - 1)) << (s + 1)) + k;
            const int e0 = channel_phys(i0), e1 = channel_phys(i0 + half), e2 = channel_phys(i0 + 2 * half), e3 = channel_phys(i0 + 3 * half);
            const float2 w1 = tw[k * (M >> s)];
            const float2 w2a = tw[k * (M >> (s + 1))], w2b = tw[(k + half) * (M >> (s + 1))];
            float2 b0, b1, b2, b3, c0, c1, c2, c3;
            channel_butterfly(w1, row[e0], row[e1], b0, b1);
            channel_butterfly(w1, row[e2], row[e3], b2, b3);
            channel_butterfly(w2a, b0, b2, c0, c2);
            channel_butterfly(w2b, b1, b3, c1, c3);
            row[e0] = c0;
            row[e1] = c1;
            row[e2] = c2;
            row[e3] = c3;
        }
        __syncthreads();
    }
}

} // namespace qpsk

#endif
