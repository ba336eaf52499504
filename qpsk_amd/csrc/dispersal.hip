/*
 * dispersal.hip -- DVB's energy dispersal (DVB TRANSPORT in include/qpsk_hip.h, restated in numpy by tests/test_dvb_cpu.py): byte q of a row of
 * group index k is xored with table[k][q], the table being the inverted-sync mask (q = 0) and the keystream bytes PR[k len + q - 1] (q >= 1), built
 * on the host once per (len, group, flags).
 *
 * dispersal_kernel: a pure stream, every byte read once and written once.  A workgroup takes DISPERSAL_ROWS consecutive rows; their dwords,
 * ceil(len / 4) a row, are laid thread after thread, DISPERSAL_ITEMS to a thread, so a wave's accesses are consecutive apart from the gaps a
 * pitch leaves.  An item's row is item / dwords-a-row by a multiplication with a reciprocal the host rounded up (exact below 2048 items for a
 * divisor up to 64: launch_dispersal); no thread divides.  DWORD = true where both buffers and both pitches are multiples of 4: a thread first
 * loads its whole dwords, all of them before the first store, then xors each with one dword of the table and stores it; the last len & 3 bytes
 * of a row, and every byte where DWORD = false, go byte by byte, so that no byte between two rows is ever read or written.  The table (at most
 * 16 * 256 bytes, rows dword aligned) is read from memory through the caches: every workgroup reads the same few kilobytes, and staging them in
 * the LDS would cost each workgroup a fill and a barrier for 6 KiB of rows.  A row whose index is not below `group` is copied: its index is never
 * used as an address.  In place (out == in with equal pitches) a thread overwrites only what it has read itself.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace qpsk {

namespace {

constexpr int DISPERSAL_ROWS = 32;       /* rows a workgroup takes */
constexpr int DISPERSAL_ITEMS = 8;       /* dwords a thread takes: DISPERSAL_ROWS * 64 dwords a row at most, over 256 threads */

struct DispersalArgs {
    const uint8_t *in, *table, *wflags;
    uint8_t *out;
    size_t in_pitch, out_pitch, nrows;
    int len, group, first, per_row, table_pitch;
    unsigned recip;      /* ceil(2^20 / per_row) */
};

template <bool DWORD>
__global__ void __launch_bounds__(256) dispersal_kernel(DispersalArgs a)
{
    const size_t row0 = (size_t)blockIdx.x * DISPERSAL_ROWS;
    const size_t left = a.nrows - row0;
    const unsigned nitems = (unsigned)(left < (size_t)DISPERSAL_ROWS ? left : (size_t)DISPERSAL_ROWS) * (unsigned)a.per_row;
    const unsigned index0 = (unsigned)((row0 + (unsigned)a.first) % (unsigned)a.group);      /* the first row's, without d_flags: wave-uniform */
    unsigned word[DISPERSAL_ITEMS];
#pragma unroll
    for (int k = 0; k < DISPERSAL_ITEMS; k++) {
        const unsigned item = threadIdx.x + 256u * k;
        word[k] = 0;
        if (DWORD && item < nitems) {
            const unsigned r = (item * a.recip) >> 20;
            const int q = 4 * (int)(item - r * (unsigned)a.per_row);
            if (q + 4 <= a.len) word[k] = *reinterpret_cast<const unsigned *>(a.in + (row0 + r) * a.in_pitch + q);
        }
    }
#pragma unroll
    for (int k = 0; k < DISPERSAL_ITEMS; k++) {
        const unsigned item = threadIdx.x + 256u * k;
        if (item >= nitems) continue;
        const unsigned r = (item * a.recip) >> 20;
        const int q = 4 * (int)(item - r * (unsigned)a.per_row);
        const size_t row = row0 + r;
        const int idx = a.wflags ? a.wflags[row] >> 4 : (int)((index0 + r) % (unsigned)a.group);
        const bool live = idx < a.group;
        const uint8_t *t = a.table + (live ? idx * a.table_pitch : 0) + q;
        uint8_t *dst = a.out + row * a.out_pitch + q;
        if (DWORD && q + 4 <= a.len) {
            *reinterpret_cast<unsigned *>(dst) = live ? word[k] ^ *reinterpret_cast<const unsigned *>(t) : word[k];
            continue;
        }
        const uint8_t *src = a.in + row * a.in_pitch + q;
        const int nb = min(4, a.len - q);
        uint8_t v[4];
        for (int j = 0; j < nb; j++) v[j] = src[j];      /* read first: in place, dst is src */
        for (int j = 0; j < nb; j++) dst[j] = live ? (uint8_t)(v[j] ^ t[j]) : v[j];
    }
}

} // namespace

int launch_dispersal(const uint8_t *in, size_t in_pitch, int nrows, int len, int group, const uint8_t *table, const uint8_t *wflags, int first,
                     uint8_t *out, size_t out_pitch, hipStream_t s)
{
    if (!in || !out || !table || nrows < 1 || len < 2 || len > 255 || group < 1 || group > DISPERSAL_MAX_GROUP || in_pitch < (size_t)len ||
        out_pitch < (size_t)len || first < 0 || first >= group || (wflags && first))
        return (int)hipErrorInvalidValue;
    const int per_row = (len + 3) / 4;
    /* item / per_row == (item * recip) >> 20 for item < 2048, per_row <= 64: recip exceeds 2^20 / per_row by less than 1, so the product
     * exceeds item / per_row by less than 2048 / 2^20 = 1 / 512, which the fraction of item / per_row (at most 63 / 64) has room for; and
     * 2047 * 2^20 fits 32 bits */
    static_assert(DISPERSAL_ROWS * 64 <= 2048 && DISPERSAL_ROWS * 64 <= 256 * DISPERSAL_ITEMS, "the reciprocal's range, and every dword of a workgroup's rows has a thread");
    const DispersalArgs a = {in, table, wflags, out, in_pitch, out_pitch, (size_t)nrows, len, group, first, per_row, dispersal_table_pitch(len),
                             ((1u << 20) + (unsigned)per_row - 1u) / (unsigned)per_row};
    const unsigned blocks = (unsigned)(((size_t)nrows + DISPERSAL_ROWS - 1) / DISPERSAL_ROWS);
    const bool dword = !(((uintptr_t)in | (uintptr_t)out | (uintptr_t)in_pitch | (uintptr_t)out_pitch) & 3);
    if (dword) hipLaunchKernelGGL(dispersal_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dispersal_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
