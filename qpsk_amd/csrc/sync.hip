/*
 * sync.hip -- what turns the receiver's decisions into a payload (include/qpsk_hip.h, qpsk_rx_batch_data / qpsk_sync_batch):
 *
 *   sync_search_kernel       per frame, the lag and the quarter-turn rotation at which a caller's sync word matches the data
 *                            decisions best, then the payload behind it de-rotated into the transmitter's dibits
 *   data_from_costas_kernel  the data rule (qpsk_device.h, data_rule) over a costas_frame[] dump: qpsk_rx_batch_data on the routes
 *                            rx_lean_kernel does not serve
 *
 * ring(x) = {0, 1, 3, 2}[x] = x ^ (x >> 1) is a dibit's place on the circle in quarter turns (qpsk.c:58-63: 1, j, -1, -j for
 * dibits 0, 1, 3, 2); it is its own inverse.  A data decision rotated by r quarter turns against the transmitter reads
 * ring(ring(sent) + r), so a sync dibit s matches the received dibit x under rotation r exactly when
 * r = (ring(x) - ring(s)) & 3: one pass over the word counts all four rotations of a lag at once.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "qpsk_device.h"

namespace qpsk {

namespace {

constexpr int SYNC_WAVES = 4;     /* frames per workgroup: one wave each */

struct SyncWord {
    uint8_t ring[SYNC_MAX_WORD];  /* ring(sync[i]), i < nsync */
};

/*
 * One wave per frame.  Lane l takes lags lag_min + l, + 64, ...: per lag one pass over the word with the four rotations' counts packed
 * in the bytes of one register (a count is at most 128).  The best (score, lag, rotation) of the lane is ONE 64-bit key -- score in
 * the high word, ~(4 lag + r) in the low word -- so the wave's maximum of the keys is the largest score, then the smallest lag, then
 * the smallest rotation.  Then the payload: nout dibits from lag* + nsync on, de-rotated, byte per lane (coalesced).
 */
__global__ void __launch_bounds__(64 * SYNC_WAVES)
sync_search_kernel(const uint8_t *__restrict__ data, int nframes, int nsym, SyncWord w, int nsync, int lag_min, int lag_max, int nout,
                   uint8_t *__restrict__ out, int32_t *__restrict__ lag_out, int32_t *__restrict__ rot_out, int32_t *__restrict__ score_out)
{
    __shared__ uint8_t sw[SYNC_MAX_WORD];
    for (int i = threadIdx.x; i < nsync; i += blockDim.x) sw[i] = w.ring[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * SYNC_WAVES + (int)(threadIdx.x >> 6);
    if (f >= nframes) return;
    const uint8_t *row = data + (size_t)f * (size_t)nsym;
    unsigned long long best = 0;
    for (int L = lag_min + lane; L <= lag_max; L += 64) {
        unsigned cnt = 0;
        const uint8_t *p = row + L;
        for (int i = 0; i < nsync; i++) {
            const unsigned d = (ring_of(p[i] & 3u) - sw[i]) & 3u;
            cnt += 1u << (8 * d);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const unsigned long long key = ((unsigned long long)((cnt >> (8 * r)) & 255u) << 32) | (unsigned)~(4u * (unsigned)L + (unsigned)r);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    const unsigned low = ~(unsigned)best;
    const int L = (int)(low >> 2), r = (int)(low & 3u);
    if (lane == 0) {
        if (lag_out) lag_out[f] = L;
        if (rot_out) rot_out[f] = r;
        if (score_out) score_out[f] = (int32_t)(best >> 32);
    }
    if (out) {
        const uint8_t *p = row + L + nsync;
        uint8_t *o = out + (size_t)f * (size_t)nout;
        for (int i = lane; i < nout; i += 64) o[i] = (uint8_t)ring_of((ring_of(p[i] & 3u) - (unsigned)r) & 3u);
    }
}

__global__ void __launch_bounds__(256)
data_from_costas_kernel(const float2 *__restrict__ z, uint8_t *__restrict__ data, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        data[i] = (uint8_t)data_rule(z[i]);
}

} // namespace

int launch_sync_search(const uint8_t *data, int nframes, int nsym, const uint8_t *h_sync, int nsync, int lag_min, int lag_max, int nout,
                       uint8_t *out, int32_t *lag, int32_t *rot, int32_t *score, hipStream_t s)
{
    SyncWord w{};
    for (int i = 0; i < nsync; i++) w.ring[i] = (uint8_t)ring_of(h_sync[i] & 3u);
    hipLaunchKernelGGL(sync_search_kernel, dim3((nframes + SYNC_WAVES - 1) / SYNC_WAVES), dim3(64 * SYNC_WAVES), 0, s, data, nframes, nsym, w,
                       nsync, lag_min, lag_max, nout, out, lag, rot, score);
    return (int)hipGetLastError();
}

int launch_data_from_costas(const float2 *costas, uint8_t *data, size_t n, hipStream_t s)
{
    size_t blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(data_from_costas_kernel, dim3((unsigned)blocks), dim3(256), 0, s, costas, data, n);
    return (int)hipGetLastError();
}

} // namespace qpsk
