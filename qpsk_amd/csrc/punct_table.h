/* punct_table.h -- the encoder's side of PUNCTURING (include/qpsk_hip.h): sent bit k of a row -> (trellis step, generator).  One mapping for
 * conv_encode_punct_kernel (viterbi.hip) and frame_kernel (frame.hip) */
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

} // namespace qpsk
#endif
