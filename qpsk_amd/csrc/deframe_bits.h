/* deframe_bits.h -- the bit-plane and CRC helpers the deframer kernels share (deframe_hunt.h, deframe.hip, deframe_coded.hip) */
#ifndef QPSK_DEFRAME_BITS_H
#define QPSK_DEFRAME_BITS_H

#include <hip/hip_runtime.h>

namespace qpsk {

__device__ __forceinline__ unsigned long long funnel64(unsigned long long lo, unsigned long long hi, int l)
{
    return l ? (lo >> l) | (hi << (64 - l)) : lo;
}

__device__ __forceinline__ unsigned long long ballot64(bool b) { return (unsigned long long)__ballot(b); }

/* multiply a CRC register by m(x) modulo the CRC-16 polynomial x^16 + x^12 + x^5 + 1 */
__device__ __forceinline__ unsigned crc_mulmod(unsigned a, unsigned m)
{
    unsigned r = 0;
    for (int i = 15; i >= 0; i--) {
        r = ((r << 1) ^ ((r & 0x8000u) ? 0x1021u : 0u)) & 0xFFFFu;
        if ((m >> i) & 1u) r ^= a;
    }
    return r;
}

/* crc16()'s register after one byte b from register 0: b(x) x^16 modulo the polynomial */
__device__ __forceinline__ unsigned crc_byte(unsigned b)
{
    unsigned x = b & 0xFFu;
    x ^= x >> 4;
    return ((x << 12) ^ (x << 5) ^ x) & 0xFFFFu;
}

} // namespace qpsk
#endif
