/*
 * rs.hip -- qpsk_rs_generator, qpsk_rs_encode_batch, qpsk_rs_decode_batch (include/qpsk_hip.h, REED-SOLOMON): the byte-oriented outer code
 * behind the K = 7 inner code.  GF(256) as gf256.h builds it, alpha = 2, generator roots alpha^0 .. alpha^(nroots - 1).  The definition is restated
 * in numpy by tests/test_rs_cpu.py (rs_encode_ref, rs_decode_ref -- Euclid and a linear solve, not the algorithm below -- pinned to a
 * codebook decoder).  Integers only: no tolerance anywhere.
 *
 * ONE WAVE PER CODEWORD, RS_WAVES codewords per workgroup; this is why nroots <= 64.  The workgroup copies the field's exp / log tables
 * (gf256.h: 768 bytes, built at compile time) into LDS and meets ONE barrier, before any wave can leave; behind it a wave works on its own LDS slice
 * only, in order, and takes whichever exit its row needs (clean, corrected, failed) without waiting for its neighbours.
 *
 * rs_decode_kernel, per wave:
 *   stage      the row goes into the slice RIGHT-ALIGNED in 4 q bytes, q = ceil(n / 4), zeros in front -- the shortened code's missing
 *              leading bytes, which change no syndrome.  Lane l keeps bytes l, l + 64, l + 128, l + 192 and their erasure flags in registers.
 *   syndromes  lane i runs Horner for S_i = r(alpha^i).  A serial chain of 4 q table lookups would be all latency, so the 4 q bytes are cut
 *              into four runs of q whose chains interleave, and S_i = h0 a^(3q) ^ h1 a^(2q) ^ h2 a^q ^ h3 with a = alpha^i.  Every lane reads
 *              the same staged byte (an LDS broadcast).
 *   exits      f > nroots: failed.  All syndromes zero and f <= nroots: r is the codeword with e = 0 -- the common case.
 *   locator    Lambda starts as the erasure locator prod (1 + X_j x), X_j = alpha^(n - 1 - j), one erased position after the other (the
 *              positions come from wave ballots); then Berlekamp-Massey for r = f + 1 .. nroots with B = Lambda as its start.  Lambda_0 = 1
 *              always and only x B is ever used, so lane l holds Lambda_(l + 1) and (x B)_(l + 1): 65 coefficients in 64 lanes (deg Lambda
 *              = 64 happens, with 64 erasures).  The discrepancy is a wave xor-reduction.
 *   Chien      over the n stored positions only, lane-parallel: Horner of Lambda at X_j^-1.  A root in the shortened region is never
 *              counted, so the count then misses deg Lambda: failed.
 *   Forney     Omega = S Lambda mod x^nroots (lane i builds Omega_i); value = X_j Omega(X_j^-1) / Lambda'(X_j^-1).  The factor X_j is there
 *              because the first root is alpha^0 (with alpha^1 it cancels).
 *   verdict    THE DEFINITION'S: the corrected word is written to the slice and its syndromes are computed again; the row is decoded iff
 *              they are all zero, every root gave a value, the root count is deg Lambda, and 2 e + f <= nroots with e counted as the
 *              definition counts it (unflagged places whose byte changed).  A word that passes IS the output (it is unique); when the
 *              output exists Berlekamp-Massey finds its locator.  So nothing rests on the checks in between: they only end a hopeless row
 *              early.  Otherwise the row leaves as it came and its status is -1.
 * rs_encode_kernel: the division's shift register, lane l holding parity byte l; per data byte the feedback (a broadcast of lane 0) times
 * the lane's generator coefficient, whose logarithm travels in the kernel arguments.
 * No atomics, no scratch, no status word: a failed decode is a row's result, not an error.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf256.h"
#include "kernels.h"
#include "wave_sync.h"

namespace qpsk {

namespace {

constexpr int RS_WAVES = 4;

struct RsSlice {
    uint8_t row[256];      /* the word, right-aligned in 4 q bytes */
    uint8_t syn[64];
    uint8_t lam[68];       /* Lambda_0 .. Lambda_64 */
    uint8_t om[64];
};

struct RsLds {
    GfTables gf;           /* first: tests/rs_port.py models the offsets */
    RsSlice w[RS_WAVES];
};

__device__ __forceinline__ unsigned wave_xor(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v ^= (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

/* the word in row[0 .. 4 q) at alpha^i: four interleaved Horner chains */
__device__ __forceinline__ unsigned syndrome(const GfTables &g, const uint8_t *row, int q, unsigned i)
{
    unsigned h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    for (int t = 0; t < q; t++) {
        h0 = gmul_log(g, h0, i) ^ row[t];
        h1 = gmul_log(g, h1, i) ^ row[q + t];
        h2 = gmul_log(g, h2, i) ^ row[2 * q + t];
        h3 = gmul_log(g, h3, i) ^ row[3 * q + t];
    }
    const unsigned s = (i * (unsigned)q) % 255u;
    return gmul_log(g, h0, (3u * s) % 255u) ^ gmul_log(g, h1, (2u * s) % 255u) ^ gmul_log(g, h2, s) ^ h3;
}

struct RsDecodeArgs {
    const uint8_t *in;
    size_t in_pitch;
    const uint8_t *erase;      /* [nrows][n] or NULL */
    uint8_t *out;              /* or NULL */
    size_t out_pitch;
    int32_t *info;             /* [nrows][4] or NULL */
    int nrows, n, nroots;
};

__global__ void __launch_bounds__(64 * RS_WAVES)
rs_decode_kernel(RsDecodeArgs a)
{
    __shared__ __attribute__((aligned(16))) RsLds L;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const unsigned urow = blockIdx.x * (unsigned)RS_WAVES + (unsigned)wave;
    const bool live = urow < (unsigned)a.nrows;      /* wave-uniform */
    const int n = a.n, nroots = a.nroots;
    const int q = (n + 3) >> 2, pad = 4 * q - n;
    RsSlice &w = L.w[wave];
    const GfTables &g = L.gf;
    unsigned rb[4] = {0, 0, 0, 0};
    bool fl[4] = {false, false, false, false};

    gf_load(L.gf, threadIdx.x, 64u * RS_WAVES);
    if (live) {
        const uint8_t *src = a.in + (size_t)urow * a.in_pitch;
        const uint8_t *er = a.erase ? a.erase + (size_t)urow * (size_t)n : nullptr;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = lane + 64 * c;
            if (j < n) {
                rb[c] = src[j];
                fl[c] = er && er[j] != 0;
                w.row[pad + j] = (uint8_t)rb[c];
            }
        }
        if (lane < pad) w.row[lane] = 0;
    }
    __syncthreads();      /* the only workgroup barrier: every exit lies behind it */
    if (!live) return;

    uint8_t *dst = a.out ? a.out + (size_t)urow * a.out_pitch : nullptr;
    int32_t *info = a.info ? a.info + 4 * (size_t)urow : nullptr;
    int f = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) f += __popcll((unsigned long long)__ballot(fl[c]));

    unsigned S = syndrome(g, w.row, q, (unsigned)lane);
    if (lane >= nroots) S = 0;
    const int clean = __ballot(S != 0) == 0 ? 1 : 0;

    const auto leave = [&](const unsigned *bytes, int changed, int e) {
        if (dst) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int j = lane + 64 * c;
                if (j < n) dst[j] = (uint8_t)bytes[c];
            }
        }
        if (info && lane == 0) {
            info[0] = changed;
            info[1] = f;
            info[2] = e;
            info[3] = clean;
        }
    };
    if (f > nroots) return leave(rb, -1, -1);
    if (clean) return leave(rb, 0, 0);

    w.syn[lane] = (uint8_t)S;
    wave_sync();

    /* Lambda = the erasure locator; lane l holds Lambda_(l + 1) */
    unsigned lam = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        unsigned long long m = (unsigned long long)__ballot(fl[c]);
        while (m) {
            const int j = 64 * c + (__ffsll((long long)m) - 1);
            m &= m - 1;
            unsigned prev = (unsigned)__shfl_up((int)lam, 1, 64);
            if (lane == 0) prev = 1;
            lam ^= gmul_log(g, prev, (unsigned)(n - 1 - j));
        }
    }
    /* Berlekamp-Massey; xb = x B, lane l holds (x B)_(l + 1) */
    unsigned xb = (unsigned)__shfl_up((int)lam, 1, 64);
    if (lane == 0) xb = 1;
    int len = f;
    for (int r = f + 1; r <= nroots; r++) {
        const int at = r - 2 - lane;
        const unsigned term = at >= 0 ? gmul(g, lam, w.syn[at >= 0 ? at : 0]) : 0u;
        const unsigned d = (unsigned)__builtin_amdgcn_readfirstlane((int)(wave_xor(term) ^ w.syn[r - 1]));
        unsigned shifted = (unsigned)__shfl_up((int)xb, 1, 64);
        if (lane == 0) shifted = 0;
        if (d == 0) {
            xb = shifted;
            continue;
        }
        const unsigned next = lam ^ gmul(g, d, xb);
        if (2 * len <= r + f - 1) {
            len = r + f - len;
            const unsigned dinv = g.exp[255u - (unsigned)g.log[d]];
            unsigned up = (unsigned)__shfl_up((int)lam, 1, 64);
            if (lane == 0) up = 1;
            xb = gmul(g, up, dinv);
        } else
            xb = shifted;
        lam = next;
    }
    const unsigned long long nz = (unsigned long long)__ballot(lam != 0);
    if (nz == 0) return leave(rb, -1, -1);      /* non-zero syndromes and nothing to correct */
    const int deg = 64 - __clzll((long long)nz);
    w.lam[lane + 1] = (uint8_t)lam;
    if (lane == 0) w.lam[0] = 1;
    wave_sync();

    /* Omega_i = sum_k S_(i - k) Lambda_k */
    {
        unsigned om = 0;
        for (int k = 0; k <= deg && k < 64; k++) {
            const int at = lane - k;
            const unsigned t = gmul(g, w.syn[at >= 0 ? at : 0], w.lam[k]);
            om ^= at >= 0 ? t : 0u;
        }
        w.om[lane] = (uint8_t)(lane < nroots ? om : 0u);
    }
    wave_sync();

    unsigned cb[4];
    int roots = 0, changed = 0, e = 0;
    bool bad = false;
    const int top = (deg & 1) ? deg : deg - 1;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        cb[c] = rb[c];
        if (64 * c >= n) continue;      /* wave-uniform */
        const int j = lane + 64 * c;
        const bool valid = j < n;
        const unsigned lx = valid ? (unsigned)(n - 1 - j) : 0u;      /* log X_j */
        const unsigned ly = (255u - lx) % 255u;                      /* log X_j^-1 */
        unsigned v = 0;
        for (int i = deg; i >= 0; i--) v = gmul_log(g, v, ly) ^ w.lam[i];
        const bool root = valid && v == 0;
        const unsigned long long rm = (unsigned long long)__ballot(root);
        roots += __popcll(rm);
        if (rm == 0) continue;
        unsigned o = 0, dd = 0;
        const int otop = deg - 1 < nroots - 1 ? deg - 1 : nroots - 1;
        for (int i = otop; i >= 0; i--) o = gmul_log(g, o, ly) ^ w.om[i];
        const unsigned ly2 = (2u * ly) % 255u;
        for (int i = top; i >= 1; i -= 2) dd = gmul_log(g, dd, ly2) ^ w.lam[i];
        const unsigned num = gmul_log(g, o, lx);
        const unsigned quot = g.exp[(unsigned)g.log[num] + 255u - (unsigned)g.log[dd]];
        const unsigned val = (root && num && dd) ? quot : 0u;
        bad = bad || (root && dd == 0);
        cb[c] = rb[c] ^ val;
        changed += __popcll((unsigned long long)__ballot(val != 0));
        e += __popcll((unsigned long long)__ballot(val != 0 && !fl[c]));
    }
    if (__ballot(bad) != 0 || roots != deg || 2 * e + f > nroots) return leave(rb, -1, -1);

    /* the verdict: the corrected word's own syndromes */
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int j = lane + 64 * c;
        if (j < n) w.row[pad + j] = (uint8_t)cb[c];
    }
    wave_sync();
    unsigned S2 = syndrome(g, w.row, q, (unsigned)lane);
    if (lane >= nroots) S2 = 0;
    if (__ballot(S2 != 0) != 0) return leave(rb, -1, -1);
    leave(cb, changed, e);
}

struct RsEncodeArgs {
    const uint8_t *data;
    size_t data_pitch;
    uint8_t *out;
    size_t out_pitch;
    int nrows, k, nroots;
    uint8_t glog[64];          /* log of the coefficient of x^(nroots - 1 - l) of g, for lane l < nroots */
    uint8_t gnz[64];           /* 1 where that coefficient is not zero */
};

__global__ void __launch_bounds__(64 * RS_WAVES)
rs_encode_kernel(RsEncodeArgs a)
{
    __shared__ __attribute__((aligned(16))) RsLds L;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const unsigned urow = blockIdx.x * (unsigned)RS_WAVES + (unsigned)wave;
    const bool live = urow < (unsigned)a.nrows;
    const int k = a.k, nroots = a.nroots;
    RsSlice &w = L.w[wave];
    const GfTables &g = L.gf;

    gf_load(L.gf, threadIdx.x, 64u * RS_WAVES);
    if (live) {
        const uint8_t *src = a.data + (size_t)urow * a.data_pitch;
        uint8_t *dst = a.out + (size_t)urow * a.out_pitch;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = lane + 64 * c;
            if (j < k) {
                const uint8_t b = src[j];
                w.row[j] = b;
                dst[j] = b;
            }
        }
    }
    __syncthreads();
    if (!live) return;

    const unsigned gl = a.glog[lane];
    const bool gn = lane < nroots && a.gnz[lane] != 0;
    unsigned par = 0;
    for (int j = 0; j < k; j++) {
        const unsigned fb = (unsigned)w.row[j] ^ (unsigned)__builtin_amdgcn_readfirstlane((int)par);
        unsigned nxt = (unsigned)__shfl_down((int)par, 1, 64);
        if (lane == 63) nxt = 0;
        const unsigned t = g.exp[(unsigned)g.log[fb] + gl];
        par = nxt ^ ((fb && gn) ? t : 0u);
    }
    if (lane < nroots) a.out[(size_t)urow * a.out_pitch + (size_t)k + (size_t)lane] = (uint8_t)par;
}

} // namespace

/* g(x) = prod_{i < nroots} (x - alpha^i), highest coefficient first; the caller has checked nroots */
void rs_generator(int nroots, uint8_t *g)
{
    uint8_t low[RS_MAX_ROOTS + 1] = {1};      /* lowest first */
    for (int i = 0; i < nroots; i++) {
        for (int j = i + 1; j >= 1; j--) {
            const unsigned m = low[j] ? H_GF.exp[(unsigned)H_GF.log[low[j]] + (unsigned)i] : 0u;
            low[j] = (uint8_t)(low[j - 1] ^ m);
        }
        low[0] = low[0] ? H_GF.exp[(unsigned)H_GF.log[low[0]] + (unsigned)i] : 0;
    }
    for (int j = 0; j <= nroots; j++) g[j] = low[nroots - j];
}

int launch_rs_encode(const uint8_t *data, size_t data_pitch, int nrows, int k, int nroots, uint8_t *out, size_t out_pitch, hipStream_t s)
{
    if (!data || !out || nrows < 1 || k < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || k + nroots > 255 || data_pitch < (size_t)k ||
        out_pitch < (size_t)(k + nroots))
        return (int)hipErrorInvalidValue;
    RsEncodeArgs a{};
    a.data = data;
    a.data_pitch = data_pitch;
    a.out = out;
    a.out_pitch = out_pitch;
    a.nrows = nrows;
    a.k = k;
    a.nroots = nroots;
    uint8_t gen[RS_MAX_ROOTS + 1];
    rs_generator(nroots, gen);
    for (int l = 0; l < nroots; l++) {
        a.glog[l] = H_GF.log[gen[l + 1]];
        a.gnz[l] = gen[l + 1] != 0;
    }
    const dim3 grid(((unsigned)nrows + RS_WAVES - 1) / RS_WAVES), block(64 * RS_WAVES);
    hipLaunchKernelGGL(rs_encode_kernel, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_rs_decode(const uint8_t *in, size_t in_pitch, int nrows, int n, int nroots, const uint8_t *erase, uint8_t *out, size_t out_pitch,
                     int32_t *info, hipStream_t s)
{
    if (!in || (!out && !info) || nrows < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || n <= nroots || n > 255 || in_pitch < (size_t)n ||
        (out && out_pitch < (size_t)n))
        return (int)hipErrorInvalidValue;
    RsDecodeArgs a{};
    a.in = in;
    a.in_pitch = in_pitch;
    a.erase = erase;
    a.out = out;
    a.out_pitch = out_pitch;
    a.info = info;
    a.nrows = nrows;
    a.n = n;
    a.nroots = nroots;
    const dim3 grid(((unsigned)nrows + RS_WAVES - 1) / RS_WAVES), block(64 * RS_WAVES);
    hipLaunchKernelGGL(rs_decode_kernel, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
