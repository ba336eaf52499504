/*
 * polyphase.h -- what the polyphase filter banks' kernels share (channel.hip, synth.hip; device only): a branch's sequence across the
 * history and the push, and the run of one branch's filter over consecutive times.  A branch is one of the M sequences the blocks of M
 * values fall into; its filter is y(t) = fl(h0 s(t)) + fl(h1 s(t - 1)) + ... + fl(h(P-1) s(t - P + 1)), summed in that order, real and
 * imaginary part apart.  The history the banks carry between pushes moves on with polyphase_history_kernel (polyphase.hip).
 */
#ifndef QPSK_POLYPHASE_H
#define QPSK_POLYPHASE_H

#include <hip/hip_runtime.h>

namespace qpsk {

/* element e of block t of the push `cur` [T][M]; t < 0: of the history `hist` [P - 1][M], the blocks -(P - 1) .. -1.  No branch, so that a
 * lane's loads go out together: a block at or beyond T (a time whose output is never stored) reads the push's last block instead, and no
 * address outside the buffers is formed */
__device__ __forceinline__ float2 polyphase_at(const float2 *cur, const float2 *hist, long long t, int T, int P, int M, int e)
{
    t = t < T ? t : (long long)T - 1;
    const float2 *block = t >= 0 ? cur + (size_t)t * M : hist + (size_t)(t + P - 1) * M;
    return block[e];
}

/* One lane filters one branch over the times t0 .. t0 + count - 1 of its run: s(t) = fetch(t), t >= t0 - (P - 1), fetch taking a 64-bit
 * time (the window's offsets are subtracted behind the widening, so that they fold into the caller's 64-bit base); the branch's taps are
 * taps[q tap_stride + first]; emit(t, y(t)) takes the results in order.  PT = P > 0: the P taps and the last P - 1 values stay in
 * registers, a time loads one new value and shifts the window (a run re-reads (count + P - 1) / count of its input), UNROLL new values in
 * flight.  PT = 0, any P: every product loads its tap and its value, nothing is kept */
template <int PT, int UNROLL, class Fetch, class Emit>
__device__ __forceinline__ void polyphase_branch_run(const float *taps, int first, int tap_stride, int P, int t0, int count, Fetch fetch, Emit emit)
{
    if constexpr (PT > 0) {
        float h[PT];
        float2 w[PT > 1 ? PT - 1 : 1];      /* w[j] = s(t - 1 - j) */
#pragma unroll
        for (int q = 0; q < PT; q++) h[q] = taps[(size_t)q * tap_stride + first];
#pragma unroll
        for (int j = 0; j < PT - 1; j++) w[j] = fetch((long long)t0 - 1 - j);
#pragma unroll UNROLL
        for (int t = t0; t < t0 + count; t++) {
            const float2 s0 = fetch(t);
            float accr = h[0] * s0.x, acci = h[0] * s0.y;
#pragma unroll
            for (int q = 1; q < PT; q++) {
                accr = accr + h[q] * w[q - 1].x;
                acci = acci + h[q] * w[q - 1].y;
            }
            emit(t, make_float2(accr, acci));
#pragma unroll
            for (int j = PT - 2; j > 0; j--) w[j] = w[j - 1];
            if (PT > 1) w[0] = s0;
        }
    } else {
        for (int t = t0; t < t0 + count; t++) {
            const float2 s0 = fetch(t);
            const float h0 = taps[first];
            float accr = h0 * s0.x, acci = h0 * s0.y;
#pragma unroll 4
            for (int q = 1; q < P; q++) {
                const float2 sq = fetch((long long)t - q);
                const float hq = taps[(size_t)q * tap_stride + first];
                accr = accr + hq * sq.x;
                acci = acci + hq * sq.y;
            }
            emit(t, make_float2(accr, acci));
        }
    }
}

} // namespace qpsk

#endif
