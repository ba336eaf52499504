/* punct_table.h -- the encoders' side of a row's layout (kernels.h, CodedLayout): on-air dibit d -> its two sent bits -> (trellis step, generator)
 * -> the coded bit.  One walk, coded_dibit, for conv_encode_punct_kernel / conv_encode_ilv_kernel (viterbi.hip) and the framer's coded bodies
 * (frame.hip); what differs between them is where the encoder's register comes from, and that is the caller's functor */
#ifndef QPSK_PUNCT_TABLE_H
#define QPSK_PUNCT_TABLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace qpsk {

/* sent bit m of a period -> its step within the period (bits 0..4) and which coded bit it is (bit 5): built by the host, passed by value */
struct PunctTable {
    uint8_t e[64];
};

/* false: the pattern's K is not the number of its mask bits (the caller made the Puncture by hand) */
inline bool punct_table_make(const Puncture &p, PunctTable *tab)
{
    *tab = PunctTable{};
    int m = 0;
    for (int r = 0; r < p.period; r++)
        for (int j = 0; j < 2; j++)
            if (((j ? p.keep1 : p.keep0) >> r) & 1u) {
                if (m == 64) return false;
                tab->e[m++] = (uint8_t)(r | (j << 5));
            }
    return m == p.K;
}

/* sent bit k of a row: *t = its trellis step; returns which coded bit of that step it is (0: c0, generator 171; 1: c1, generator 133) */
__device__ __forceinline__ unsigned punct_sent_step(unsigned k, int period, int K, const PunctTable &tab, int *t)
{
    const unsigned q = k / (unsigned)K, e = tab.e[k - q * (unsigned)K];
    *t = (int)(q * (unsigned)period + (e & 31u));
    return (e >> 5) & 1u;
}

/* on-air dibit d of a row of nsent sent bits: on-air bits 2 d and 2 d + 1 take sent bits map.at(2 d) and map.next of it -- FlatMap: themselves; the
 * encoders' IlvMul of s^-1: (2 d) s^-1 mod n and that + s^-1 (mod n).  A number at or beyond nsent is the pad of an odd nsent and stays 0.
 * bit(t, j) = coded bit j of step t (0: c0, generator 171; 1: c1, generator 133), 0 or 1 */
template <class Map, class Bit>
__device__ __forceinline__ unsigned coded_dibit(unsigned d, unsigned nsent, const Puncture &p, const PunctTable &tab, const Map &map, const Bit &bit)
{
    unsigned dibit = 0, k = map.at(2u * d);
#pragma unroll
    for (int h = 0; h < 2; h++, k = map.next(k)) {
        if (k >= nsent) continue;
        int t;
        const unsigned j = punct_sent_step(k, p.period, p.K, tab, &t);
        dibit |= (unsigned)bit(t, j) << h;
    }
    return dibit;
}

} // namespace qpsk
#endif
