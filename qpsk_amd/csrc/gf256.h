/*
 * gf256.h -- GF(256) modulo 0x11D, alpha = 2, for the Reed-Solomon units (rs.hip, rs_cross.hip): the exp / log tables, built at compile
 * time, as a host constant (H_GF) and as a __constant__ instance that a workgroup copies into its LDS, and the multiplies over the LDS
 * copy.  Everything has internal linkage: each unit that includes this carries its own 768 bytes in its code object (without relocatable
 * device code two units cannot share one device symbol).
 */
#ifndef QPSK_GF256_H
#define QPSK_GF256_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpsk {

namespace {

struct GfTables {
    uint8_t exp[512];      /* alpha^i for i < 510 (the period twice: log a + log b needs no reduction) */
    uint8_t log[256];      /* log[0] is never used as a logarithm */
};

constexpr GfTables gf_make()
{
    GfTables t{};
    unsigned x = 1;
    for (int i = 0; i < 255; i++) {
        t.exp[i] = (uint8_t)x;
        t.exp[i + 255] = (uint8_t)x;
        t.log[x] = (uint8_t)i;
        x <<= 1;
        if (x & 0x100u) x ^= 0x11Du;
    }
    return t;
}

constexpr GfTables H_GF = gf_make();
__constant__ GfTables c_gf = gf_make();

static_assert(sizeof(GfTables) == 768, "192 dwords");

/* the tables into a workgroup's LDS copy: the thread takes dwords first, first + step, ...; the caller's barrier follows */
__device__ __forceinline__ void gf_load(GfTables &lds, unsigned first, unsigned step)
{
    const unsigned *src = reinterpret_cast<const unsigned *>(&c_gf);
    unsigned *dst = reinterpret_cast<unsigned *>(&lds);
    for (unsigned i = first; i < 192u; i += step) dst[i] = src[i];
}

__device__ __forceinline__ unsigned gmul(const GfTables &g, unsigned a, unsigned b)
{
    const unsigned v = g.exp[(unsigned)g.log[a] + (unsigned)g.log[b]];
    return (a && b) ? v : 0u;
}

/* a alpha^l, l < 255 */
__device__ __forceinline__ unsigned gmul_log(const GfTables &g, unsigned a, unsigned l)
{
    const unsigned v = g.exp[(unsigned)g.log[a] + l];
    return a ? v : 0u;
}

} // namespace

} // namespace qpsk

#endif
