/*
 * deframe.hip -- packets out of continuous streams of data decisions (include/qpsk_hip.h, qpsk_deframer_push):
 *
 *   deframe_kernel   one wave per stream: deframe_hunt.h's hunt (the sequence D, the window X, the scoring and the walk are described
 *                    there) over data rows or costas_frame[] rows, each completed packet de-rotated, descrambled, packed to bytes and
 *                    checked against its CRC-16; an incomplete packet's payload waits in the pending buffer as ring values
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "qpsk_device.h"
#include "deframe_bits.h"
#include "deframe_hunt.h"

namespace qpsk {

namespace {

template <bool COSTAS>
__device__ __forceinline__ unsigned ring_at(const void *row, long long i)
{
    if (COSTAS) return qpsk::ring_at(reinterpret_cast<const float2 *>(row), i);      /* deframe_hunt.h's */
    return ring_of(reinterpret_cast<const uint8_t *>(row)[i] & 3u);
}

/*
 * One completed packet, by the whole wave.  Payload dibit i < have comes from the pending buffer, i >= have from the row at
 * row0 + i - have.  Lane l builds bytes [l c, (l+1) c) (c = the args' bytes per lane) and runs crc16() over those below nbytes from
 * register 0 (lane 0: 0xFFFF); the register times x^(8 k), k = the data bytes behind the lane's chunk, is the lane's share of the
 * packet's CRC (crc16 is linear in the register and the data), and an xor over the wave sums the shares.
 */
template <bool COSTAS>
__device__ void emit_packet(const DeframeArgs &a, int stream, int slot, long long pos, int rot, int score, const uint8_t *pend, int have,
                            const void *row, long long row0)
{
    const int lane = threadIdx.x & 63;
    const int nb = a.nbytes + 2;
    const int c = a.bytes_per_lane;
    const int k0 = lane * c;
    uint8_t *out = a.bytes ? a.bytes + ((size_t)stream * a.max_packets + slot) * (size_t)nb : nullptr;
    unsigned crc = lane == 0 ? 0xFFFFu : 0u, rx = 0;
    for (int k = k0; k < k0 + c && k < nb; k++) {
        unsigned b = 0;
        for (int j = 0; j < 4; j++) {
            const int i = 4 * k + j;
            const unsigned v = i < have ? (unsigned)pend[i] : ring_at<COSTAS>(row, row0 + (i - have));
            b |= ring_of((v - (unsigned)rot) & 3u) << (2 * j);
        }
        b ^= a.keystream[k];
        if (out) out[k] = (uint8_t)b;
        if (k < a.nbytes) {
            unsigned x = ((crc >> 8) ^ b) & 0xFFu;
            x ^= x >> 4;
            crc = ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFFu;
        } else {
            rx |= k == a.nbytes ? b << 8 : b;
        }
    }
    unsigned share = crc_mulmod(crc, a.crc_adv[lane]) | (rx << 16);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) share ^= (unsigned)__shfl_xor((int)share, o, 64);
    const size_t r = (size_t)stream * a.max_packets + slot;
    report(a, r, pos, rot, score, lane);
    if (lane == 0 && a.crc_ok) a.crc_ok[r] = (uint8_t)((share & 0xFFFFu) == (share >> 16));
}

/* the hunt's policy: packets as bytes, the pending payload as ring values */
template <bool COSTAS>
struct BytePackets {
    const DeframeArgs &a;
    int stream;
    const void *row;
    uint8_t *pend;
    __device__ __forceinline__ unsigned ring(long long i) const { return ring_at<COSTAS>(row, i); }
    __device__ __forceinline__ void complete(int slot, long long pos, int rot, int score, int have, int row0) const
    {
        emit_packet<COSTAS>(a, stream, slot, pos, rot, score, pend, have, row, row0);
    }
    __device__ __forceinline__ void collect(int have, int row0, int cnt, int /* rot: the packet is turned when it is built */) const
    {
        for (int i = threadIdx.x & 63; i < cnt; i += 64) pend[have + i] = (uint8_t)ring(row0 + i);
    }
};

template <bool COSTAS>
__global__ void __launch_bounds__(64 * HUNT_WAVES)
deframe_kernel(DeframeArgs a)
{
    const int stream = blockIdx.x * HUNT_WAVES + (int)(threadIdx.x >> 6);
    if (stream >= a.nstreams) return;
    const void *row = COSTAS ? (const void *)(a.costas + (size_t)stream * (size_t)a.nsym) : (const void *)(a.data + (size_t)stream * (size_t)a.nsym);
    uint8_t *st = a.state + (size_t)stream * a.state_stride;
    BytePackets<COSTAS> p = {a, stream, row, st + DEFRAME_PEND_OFFSET};
    deframe_hunt(a, stream, 4 * (a.nbytes + 2), a.max_packets, st, p);
}

} // namespace

int launch_deframe(const DeframeArgs &a, hipStream_t s)
{
    const dim3 grid((a.nstreams + HUNT_WAVES - 1) / HUNT_WAVES), block(64 * HUNT_WAVES);
    if (a.costas)
        hipLaunchKernelGGL(deframe_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(deframe_kernel<false>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
