/* soft_quant.h -- the quantiser of qpsk_soft_batch (include/qpsk_hip.h: q(x), (u, v) = z (-j)^r), shared by soft.hip and the coded
 * deframer (deframe_coded.hip) */
#ifndef QPSK_SOFT_QUANT_H
#define QPSK_SOFT_QUANT_H

#include <hip/hip_runtime.h>
#include <float.h>

namespace qpsk {

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }

__device__ __forceinline__ unsigned q8(float x, float g)
{
    const float v = fminf(127.0f, fmaxf(-127.0f, rintf(x * g)));
    return (unsigned)(int)v & 255u;
}

/* z (-j)^r as the two int8 of one output symbol, bit 0's in the low byte */
__device__ __forceinline__ unsigned soft_pair(float2 z, int r, float g, bool &bad)
{
    bad |= !finite_f(z.x) || !finite_f(z.y);
    /* (a, b), (b, -a), (-a, -b), (-b, a): one swap and two sign bits, so a wave-uniform r costs one select mask, not three */
    const bool swap = r & 1;
    const unsigned nu = (r & 2) ? 0x80000000u : 0u, nv = ((r + 1) & 2) ? 0x80000000u : 0u;
    const float u = __uint_as_float(__float_as_uint(swap ? z.y : z.x) ^ nu);
    const float v = __uint_as_float(__float_as_uint(swap ? z.x : z.y) ^ nv);
    return q8(u, g) | (q8(v, g) << 8);
}

} // namespace qpsk
#endif
