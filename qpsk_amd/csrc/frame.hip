/*
 * frame.hip -- qpsk_frame_batch (include/qpsk_hip.h, FRAMER): payloads in, rows of on-air dibits out -- the packets the three deframers
 * receive, placed in idle-filled rows, in ONE launch.  The definition is a composition of pinned ones (crc16, the scrambler's keystream,
 * qpsk_conv_encode_punct_batch), restated in numpy by tests/test_frame_cpu.py (frame_ref).  Integers only: no tolerance anywhere.
 *
 * frame_kernel<CODED>: ONE WAVE PER PACKET, FRAME_WAVES packets per workgroup; a wave past the last packet does nothing between the
 * barriers.  Per wave:
 *   stage   the payload goes into the wave's LDS slice, lane-parallel and coalesced (byte loads: the payload pointer and pitch are
 *           arbitrary).  A zero byte lies in front of the packet and one behind it, so that the coded body's register needs no bounds:
 *           the bits before the row and the six tail bits are read as what they are, zeros.
 *   crc     deframe_kernel's way, backwards: lane l runs crc16()'s byte recurrence from register 0 over its chunk of c = ceil(nbytes / 64)
 *           bytes; that register times x^(8 k) mod the polynomial, k = the bytes behind the chunk, is the lane's share (crc16 is linear in
 *           the register and the data); the init value's share is 0xFFFF x^(8 nbytes); an xor over the wave sums them.  The 64 factors and
 *           the init share are built by the host per call and travel in the kernel arguments.  Lane 0 appends the CRC to the staged
 *           packet, big-endian, and stores d_crc.
 *   columns the wave owns the columns [c0, c1) of its row: the idle columns in front of its packet (the lead for the row's first packet,
 *           the gap otherwise), the packet, and for the row's last packet the columns behind it up to row_len -- the waves of a row
 *           tile it, nothing is written twice and nothing needs a second launch.  dibit_at(c) is the definition read column by column:
 *           idle ks[c]; the sync word from the kernel arguments; body dibit i = ks[i] ^ E[i].  E[i] uncoded: two bits of the packet.
 *           Coded: punct_table.h's coded_dibit, the walk conv_encode_punct_kernel / conv_encode_ilv_kernel take from an on-air dibit to
 *           its sent bits and their (step t, generator); here a coded bit comes from the staged packet.  The register of step t is packet
 *           bits t - 6 .. t, seven consecutive bits of the staged bytes: two LDS byte reads and a shift give them with bit t - 6 lowest,
 *           i.e. the register mirrored, so the generators are mirrored instead (171 -> 0x4F, 133 -> 0x6D; viterbi_row.h's re-encoder
 *           does the same).  The pad bit of an odd nsent stays 0 before the xor.
 *   stores  byte-wise up to the first 4-byte aligned ADDRESS of the range (d_out, row_len and the start column are arbitrary), then one
 *           dword of four dibits per lane, 256 contiguous bytes per wave instruction, then a byte-wise tail.
 * frame_ilv_kernel (qpsk_frame_batch_ilv, INTERLEAVING in include/qpsk_hip.h): the coded kernel over the other position map -- on-air bit
 * 2 i + h of the body takes sent bit (2 i + h) s^-1 mod n, or 0 when that is at or beyond nsent (the pad's place) -- and everything else,
 * the stores included, as it is.  One body, frame_packet<CODED, ILV>, behind both kernel names, and one launch_frame that takes the body's
 * CodedLayout (kernels.h) and picks the kernel by its kind.
 * No atomics, no scratch, no inter-wave traffic beyond the two barriers that order a wave's own LDS writes before its reads.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "deframe_bits.h"
#include "punct_table.h"

namespace qpsk {

namespace {

constexpr int FRAME_WAVES = 4;
/* a wave's LDS slice: [0] zero, the packet (payload and CRC, up to FRAME_MAX_BYTES + 2 bytes) from [1], a zero byte behind it */
constexpr int FRAME_SLICE = (1 + FRAME_MAX_BYTES + 2 + 1 + 15) & ~15;

/* what travels by value: the sync word's dibits, the lanes' CRC factors x^(8 k_l) with the init value's share 0xFFFF x^(8 nbytes) at [64], the
 * sent bits of a puncturing period */
struct FrameTables {
    uint8_t sync[SYNC_MAX_WORD];
    uint16_t crc_adv[66];
    PunctTable punct;
};

template <bool CODED, bool ILV>
__device__ __forceinline__ unsigned body_dibit(const FrameArgs &a, const FrameTables &t, const IlvMul &inv, const uint8_t *slice, int i)
{
    if (!CODED) return ((unsigned)slice[1 + (i >> 2)] >> (2 * (i & 3))) & 3u;
    /* coded bit j of step `step` from the staged packet: the register mirrored, so the generators are */
    const auto bit = [&](int step, unsigned j) {
        const int at = step + 2;                /* packet bit step - 6 in the slice: one zero byte in front */
        const unsigned two = (unsigned)slice[at >> 3] | (unsigned)slice[(at >> 3) + 1] << 8;
        const unsigned w = (two >> (at & 7)) & 127u;
        return (unsigned)(__popc(w & (j ? 0x6Du : 0x4Fu)) & 1);
    };
    if (ILV) return coded_dibit((unsigned)i, a.nsent, a.punct, t.punct, inv, bit);
    return coded_dibit((unsigned)i, a.nsent, a.punct, t.punct, FlatMap{}, bit);
}

template <bool CODED, bool ILV>
__device__ __forceinline__ void frame_packet(const FrameArgs &a, const FrameTables &t, const IlvMul &inv)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[FRAME_WAVES][FRAME_SLICE];
    const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
    const unsigned upk = blockIdx.x * (unsigned)FRAME_WAVES + (unsigned)wave;
    const bool live = upk < (unsigned)a.npackets;      /* wave-uniform; the barriers below are met by every wave */
    const int pk = (int)upk;
    uint8_t *slice = lds[wave];
    if (live) {
        const uint8_t *src = a.payload + (size_t)pk * a.pitch;
        for (int k = lane; k < a.nbytes; k += 64) slice[1 + k] = src[k];
        if (lane == 0) {
            slice[0] = 0;
            slice[a.nbytes + 3] = 0;
        }
    }
    __syncthreads();
    if (live) {
        unsigned reg = 0;
        const int k0 = lane * a.bytes_per_lane;
        for (int k = k0; k < k0 + a.bytes_per_lane && k < a.nbytes; k++) {
            unsigned x = ((reg >> 8) ^ slice[1 + k]) & 0xFFu;
            x ^= x >> 4;
            reg = ((reg << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFFu;
        }
        unsigned crc = crc_mulmod(reg, t.crc_adv[lane]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) crc ^= (unsigned)__shfl_xor((int)crc, o, 64);
        crc ^= t.crc_adv[64];
        if (lane == 0) {
            slice[1 + a.nbytes] = (uint8_t)(crc >> 8);
            slice[2 + a.nbytes] = (uint8_t)(crc & 255u);
            if (a.crc) a.crc[pk] = (uint16_t)crc;
        }
    }
    __syncthreads();
    if (!live) return;

    const int row = pk / a.per_row, j = pk - row * a.per_row;
    const int P = a.nsync + a.nbody;
    const int start = a.lead + j * (P + a.gap);
    const int c0 = j == 0 ? 0 : start - a.gap;
    const int c1 = j == a.per_row - 1 ? a.row_len : start + P;
    uint8_t *out = a.out + (size_t)row * (size_t)a.row_len;
    const auto dibit_at = [&](int c) -> unsigned {
        const int i = c - start;
        if (i < 0 || i >= P) return a.ks[c];
        if (i < a.nsync) return t.sync[i];
        return (unsigned)a.ks[i - a.nsync] ^ body_dibit<CODED, ILV>(a, t, inv, slice, i - a.nsync);
    };
    int head = (int)((4u - (unsigned)((uintptr_t)(out + c0) & 3u)) & 3u);
    if (head > c1 - c0) head = c1 - c0;
    if (lane < head) out[c0 + lane] = (uint8_t)dibit_at(c0 + lane);
    const int cb = c0 + head, nd = (c1 - cb) >> 2;
    for (int d = lane; d < nd; d += 64) {
        const int c = cb + 4 * d;
        const unsigned v = dibit_at(c) | dibit_at(c + 1) << 8 | dibit_at(c + 2) << 16 | dibit_at(c + 3) << 24;
        *reinterpret_cast<unsigned *>(out + c) = v;
    }
    const int ct = cb + 4 * nd;
    if (lane < c1 - ct) out[ct + lane] = (uint8_t)dibit_at(ct + lane);
}

template <bool CODED>
__global__ void __launch_bounds__(64 * FRAME_WAVES)
frame_kernel(FrameArgs a, FrameTables t)
{
    frame_packet<CODED, false>(a, t, IlvMul{});
}

__global__ void __launch_bounds__(64 * FRAME_WAVES)
frame_ilv_kernel(FrameArgs a, FrameTables t, IlvMul inv)
{
    frame_packet<true, true>(a, t, inv);
}

} // namespace

int launch_frame(const FrameArgs &args, const CodedLayout &l, const uint8_t *h_sync, const uint16_t *h_crc_adv, hipStream_t s)
{
    FrameArgs a = args;
    if (!a.payload || !a.out || !a.ks || !h_sync || !h_crc_adv || a.npackets < 1 || a.per_row < 1 || a.nbytes < 1 || a.nbytes > FRAME_MAX_BYTES ||
        a.nsync < 1 || a.nsync > SYNC_MAX_WORD || a.nbody < 1 || a.lead < 0 || a.gap < 0 || a.bytes_per_lane * 64 < a.nbytes)
        return (int)hipErrorInvalidValue;
    if ((long long)a.lead + (long long)a.per_row * (a.nsync + a.nbody) + (long long)(a.per_row - 1) * a.gap > (long long)a.row_len)
        return (int)hipErrorInvalidValue;
    FrameTables t = {};
    for (int i = 0; i < a.nsync; i++) t.sync[i] = (uint8_t)(h_sync[i] & 3u);
    for (int i = 0; i < 65; i++) t.crc_adv[i] = h_crc_adv[i];
    const dim3 grid(((unsigned)a.npackets + FRAME_WAVES - 1) / FRAME_WAVES), block(64 * FRAME_WAVES);
    if (!a.coded) {
        hipLaunchKernelGGL(frame_kernel<false>, grid, block, 0, s, a, t);
        return (int)hipGetLastError();
    }
    const int nsteps = 8 * (a.nbytes + 2) + 6;
    if (l.kind == CODED_PLAIN || !coded_layout_fits(l, nsteps) || a.nbody != coded_ndibits(l, nsteps) || !punct_table_make(l.punct, &t.punct))
        return (int)hipErrorInvalidValue;
    a.nsent = (unsigned)coded_nsent(l, nsteps);
    a.punct = l.punct;
    if (l.kind == CODED_ILV) hipLaunchKernelGGL(frame_ilv_kernel, grid, block, 0, s, a, t, ilv_mul(l.ilv.n, l.ilv.sinv));
    else hipLaunchKernelGGL(frame_kernel<true>, grid, block, 0, s, a, t);
    return (int)hipGetLastError();
}

} // namespace qpsk
