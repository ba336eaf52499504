/*
 * rs_cross.hip -- qpsk_rs_cross_encode_batch, qpsk_rs_cross_decode_batch, qpsk_rs_cross_place_batch (include/qpsk_hip.h, PACKET ERASURE
 * CODE): REED-SOLOMON's (n, k) code laid ACROSS the n packets of a group, one codeword per byte column, so that packets lost whole come
 * back.  The definition is restated in numpy by tests/test_cross_cpu.py (cross_encode_ref, cross_decode_ref -- elimination, not the
 * algorithm below -- cross_place_ref).  Integers only: no tolerance anywhere.
 *
 * ONE WORKGROUP PER GROUP, LANE = COLUMN.  A wave owns 64 adjacent columns at a time (a tile) and walks the packets; every load is 64
 * adjacent bytes of one packet row.  Up to RSX_WAVES waves share a group's tiles.
 *
 * THE REGISTER.  A lane keeps the column's remainder R(x) = c(x) x^nroots mod g(x) as the division's shift register, four bytes to a
 * VGPR, byte 0 of word 0 the highest coefficient: NW = 1, 2, 4, 8 or 16 words hold nroots <= 4 NW bytes (the slots past nroots stay 0
 * because their generator coefficients are 0).  A step shifts the register one byte (v_alignbit per word) and adds feedback x g: the
 * feedback is the lane's, g is the call's, so the product is a multiply by a WAVE-UNIFORM constant, done by shift and xor on whole words:
 * for each bit b of the feedback, word ^= -(bit b) & G[word][b], with G[word][b] = the four coefficients of that word times alpha^b, 8 NW
 * dwords that the host builds, the kernel arguments carry and the workgroup keeps in LDS (a broadcast read; in SGPRs they would not all
 * fit).  Two VALU instructions per four field multiplies, no table lookup.
 * The encoder is this over the k data packets; its register is the parity.
 *
 * THE DECODER runs the same register over all n packets with a missing packet's byte taken as 0 (it is not loaded), so
 *     S_i = sum_l R_l y_l^i,  y_l = alpha^-(l + 1)              (R_l = slot l of the register; S_i = the column's syndrome at alpha^i)
 * f = 0: the column is a codeword iff R = 0.  f > nroots: every column fails, nothing is computed.  Otherwise the missing places p_j have
 * X_j = alpha^(n - 1 - p_j), P(x) = prod_j (x - X_j), Q_j(x) = P(x) / (x - X_j), and the missing bytes v_j solve sum_j v_j X_j^i = S_i:
 *     v_j = sum_l R_l Q_j(y_l) / Q_j(X_j)                       (Q_j has degree f - 1: the first f syndromes; Q_j(X_j) = P'(X_j))
 *     0   = sum_l R_l y_l^t P(y_l),  t < nroots - f             (sum_k P_k S_(t + k): the spare syndromes; all zero iff the column with the
 *                                                                v_j in place is a codeword)
 * Both are ONE nroots x nroots matrix W over the field that depends on the places only.  Wave 0 builds it once per group, a lane per slot
 * l (products in the logarithm, a zero factor X_j = y_l kept apart), the workgroup expands it to the shift-and-xor form
 * T[l][word][b] = four rows of column l times alpha^b in LDS, and behind one barrier a lane applies it to its register: again -(bit) & a
 * uniform dword, the dwords LDS broadcasts.  (With first root alpha^0 Forney's X_j factor is inside Q_j(y_l): nothing is left to forget.)
 * A lane's result word holds v_0 .. v_(f-1) and then the spare sums, which must vanish.
 *
 * Present bytes never change, so the first pass also copies them when the output is another buffer; the f missing places are written from
 * the result word (or copied, in a failed column) in a second, f-long pass, where the old byte is read only to count the places that
 * changed.  No atomics, no scratch, no status word: a failed column is a group's result.
 *
 * rs_cross_place_kernel: one wave per stream walks the push's packets in index order and copies each accepted one with all lanes; stores
 * of one wave to one address stay in order, which is the rule "the later index wins".
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf256.h"
#include "kernels.h"
#include "wave_sync.h"

namespace qpsk {

namespace {

constexpr int RSX_WAVES = 4;

/* G[word][b]: byte c of the dword = g's coefficient for slot 4 word + c, times alpha^b */
struct CrossGen {
    uint32_t g[16][8];
};

template <int NW>
__device__ __forceinline__ void shift_byte(uint32_t (&R)[NW])
{
#pragma unroll
    for (int w = 0; w < NW; w++) R[w] = __builtin_amdgcn_alignbit(w + 1 < NW ? R[w + 1] : 0u, R[w], 8);
}

/* acc ^= x * (the four constants of each word): m(w, b) is the uniform dword for word w, bit b */
template <int NW, typename M>
__device__ __forceinline__ void mul_acc(uint32_t (&acc)[NW], unsigned x, M m)
{
    uint32_t t[8];
#pragma unroll
    for (int b = 0; b < 8; b++) t[b] = 0u - ((x >> b) & 1u);
#pragma unroll
    for (int w = 0; w < NW; w++) {
#pragma unroll
        for (int b = 0; b < 8; b++) acc[w] ^= t[b] & m(w, b);
    }
}

/* G lies in LDS and is read again at every step (z is 0 behind a compiler barrier): 8 NW loop-invariant dwords would otherwise be hoisted
 * into more SGPRs than there are and spilled */
template <int NW>
__device__ __forceinline__ void lfsr_step(uint32_t (&R)[NW], unsigned byte, const uint32_t (*G)[8], int z)
{
    const unsigned fb = (R[0] & 0xFFu) ^ byte;
    shift_byte<NW>(R);
    mul_acc<NW>(R, fb, [&](int w, int b) { return G[z + w][b]; });
}

__device__ __forceinline__ int opaque_zero()
{
    int z = 0;
    asm volatile("" : "+v"(z));
    return z;
}

/* the call's G from the kernel arguments into LDS; the caller's barrier follows */
template <int NW>
__device__ __forceinline__ void load_gen(uint32_t (*dst)[8], const CrossGen &G)
{
    const uint32_t *src = &G.g[0][0];
    for (int i = (int)threadIdx.x; i < 8 * NW; i += (int)blockDim.x) dst[i >> 3][i & 7] = src[i];
}

struct CrossEncodeArgs {
    uint8_t *group;
    size_t pitch;
    int ngroups, k, nroots, len, skip;
    CrossGen gen;
};

template <int NW>
__global__ void __launch_bounds__(64 * RSX_WAVES)
rs_cross_encode_kernel(CrossEncodeArgs a)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), nwaves = (int)(blockDim.x >> 6);
    const int k = a.k, nroots = a.nroots, width = a.len - a.skip;
    const int ntiles = (width + 63) >> 6;
    uint8_t *grp = a.group + (size_t)blockIdx.x * (size_t)(k + nroots) * a.pitch;
    __shared__ __attribute__((aligned(16))) uint32_t G[NW][8];
    load_gen<NW>(G, a.gen);
    __syncthreads();
    for (int tile = wave; tile < ntiles; tile += nwaves) {
        const int col = a.skip + 64 * tile + lane;
        const bool active = col < a.len;
        uint8_t *src = grp + (active ? col : a.skip);
        uint32_t R[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) R[w] = 0;
        for (int p0 = 0; p0 < k; p0 += 4) {
            const int z = opaque_zero();
            unsigned by[4];
#pragma unroll
            for (int u = 0; u < 4; u++) by[u] = (p0 + u < k && active) ? src[(size_t)(p0 + u) * a.pitch] : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (p0 + u < k) lfsr_step<NW>(R, by[u], G, z);
        }
        /* the register is the parity, highest coefficient first: a byte and a shift per parity packet */
        for (int l = 0; l < nroots; l++) {
            if (active) src[(size_t)(k + l) * a.pitch] = (uint8_t)R[0];
            shift_byte<NW>(R);
        }
    }
}

struct CrossDecodeArgs {
    const uint8_t *in;
    size_t pitch;
    uint8_t *out;              /* or NULL; may be `in` with out_pitch = pitch */
    size_t out_pitch;
    const uint8_t *have;       /* [ngroups][n] */
    int32_t *info;             /* [ngroups][4] or NULL */
    uint8_t *colfail;          /* [ngroups][len - skip] or NULL */
    int ngroups, n, nroots, len, skip;
    CrossGen gen;
};

template <int NW>
struct CrossLds {
    GfTables gf;
    uint32_t gen[NW][8];              /* the call's G */
    uint32_t tab[4 * NW][NW][8];      /* T[slot l][result word][bit b] */
    uint8_t wb[4 * NW][4 * NW];       /* W[result row][slot l] */
    uint8_t hv[260];                  /* 1 = packet p is there; 0 from n on */
    uint8_t place[64];                /* p_j, j < min(f, 64) */
    uint8_t xlog[64];                 /* log X_j = n - 1 - p_j */
    uint8_t dlog[64];                 /* log Q_j(X_j) */
    int f;
    int cnt[RSX_WAVES][2];            /* per wave: columns failed, bytes changed */
};

template <int NW>
__global__ void __launch_bounds__(64 * RSX_WAVES)
rs_cross_decode_kernel(CrossDecodeArgs a)
{
    constexpr int NB = 4 * NW;
    __shared__ __attribute__((aligned(16))) CrossLds<NW> L;
    const int tid = (int)threadIdx.x, nthreads = (int)blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
    const int n = a.n, nroots = a.nroots, len = a.len, skip = a.skip, width = len - skip;
    const size_t g = blockIdx.x;
    const uint8_t *grp = a.in + g * (size_t)n * a.pitch;
    uint8_t *ogrp = a.out ? a.out + g * (size_t)n * a.out_pitch : nullptr;
    const bool copy = ogrp && ogrp != grp;      /* the output is another buffer: every byte of it is written */
    const uint8_t *have = a.have + g * (size_t)n;

    {
        /* gf_load()'s loop, written out: through the call the compiler schedules this kernel's prologue in another order */
        const unsigned *s = reinterpret_cast<const unsigned *>(&c_gf);
        unsigned *d = reinterpret_cast<unsigned *>(&L.gf);
        for (int i = tid; i < 192; i += nthreads) d[i] = s[i];
        for (int p = tid; p < 260; p += nthreads) L.hv[p] = (p < n && have[p] != 0) ? 1 : 0;
        if (tid < RSX_WAVES) L.cnt[tid][0] = L.cnt[tid][1] = 0;
        load_gen<NW>(L.gen, a.gen);
    }
    __syncthreads();

    /* ---- the places, and what depends on them alone: wave 0, once per group */
    if (wave == 0) {
        int f = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int p = lane + 64 * c;
            const bool miss = p < n && L.hv[p] == 0;
            const unsigned long long m = (unsigned long long)__ballot(miss);
            const int at = f + __popcll(m & ((1ull << lane) - 1ull));
            if (miss && at < 64) {
                L.place[at] = (uint8_t)p;
                L.xlog[at] = (uint8_t)(n - 1 - p);
            }
            f += __popcll(m);
        }
        if (lane == 0) L.f = f;
        wave_sync();
        if (f >= 1 && f <= nroots) {
            const GfTables &gf = L.gf;
            /* lane j: log Q_j(X_j) = sum over the other places of log (X_j - X_m) */
            {
                unsigned s = 0;
                const unsigned xj = gf.exp[L.xlog[lane < f ? lane : 0]];
                for (int m = 0; m < f; m++) {
                    const unsigned d = xj ^ gf.exp[L.xlog[m]];
                    s += (m != lane) ? (unsigned)gf.log[d] : 0u;
                }
                if (lane < f) L.dlog[lane] = (uint8_t)(s % 255u);
            }
            wave_sync();
            /* lane l: slot l, y_l = alpha^(254 - l).  plog = log of prod (y_l - X_j) over the non-zero factors; zj = the j of a zero one */
            const bool slot = lane < nroots;
            const unsigned ly = 254u - (unsigned)lane, y = gf.exp[ly];
            unsigned plog = 0;
            int zj = -1;
            for (int j = 0; j < f; j++) {
                const unsigned d = y ^ gf.exp[L.xlog[j]];
                if (d == 0)
                    zj = j;
                else
                    plog += gf.log[d];
            }
            plog %= 255u;
            if (lane < NB) {
                for (int j = 0; j < f; j++) {
                    const unsigned d = y ^ gf.exp[L.xlog[j]];
                    const unsigned dl = L.dlog[j];
                    const unsigned whole = gf.exp[(plog + 510u - (unsigned)gf.log[d] - dl) % 255u];      /* P(y) / (y - X_j) / Q_j(X_j) */
                    const unsigned apart = gf.exp[(plog + 255u - dl) % 255u];                            /* y = X_j: the product without that factor */
                    const unsigned v = zj < 0 ? whole : (zj == j ? apart : 0u);
                    L.wb[j][lane] = (uint8_t)(slot ? v : 0u);
                }
                for (int t = 0; f + t < NB; t++) {
                    const unsigned v = gf.exp[(plog + (unsigned)t * ly) % 255u];                         /* y^t P(y) */
                    L.wb[f + t][lane] = (uint8_t)((slot && zj < 0 && f + t < nroots) ? v : 0u);
                }
            }
        }
    }
    __syncthreads();
    const int f = L.f;
    const bool solve = f >= 1 && f <= nroots;      /* uniform over the workgroup */
    if (solve) {
        const GfTables &gf = L.gf;
        for (int i = tid; i < NB * NW * 8; i += nthreads) {
            const int b = i & 7, w = (i >> 3) % NW, l = i / (8 * NW);
            uint32_t word = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const unsigned x = L.wb[4 * w + c][l];
                const unsigned v = gf.exp[(unsigned)gf.log[x] + (unsigned)b];
                word |= (x ? v : 0u) << (8 * c);
            }
            L.tab[l][w][b] = word;
        }
        __syncthreads();
    }

    /* ---- the header bytes, for another buffer only */
    if (copy && skip > 0) {
        for (int i = tid; i < n * skip; i += nthreads) {
            const int p = i / skip, c = i - p * skip;
            ogrp[(size_t)p * a.out_pitch + (size_t)c] = grp[(size_t)p * a.pitch + (size_t)c];
        }
    }

    const int ntiles = (width + 63) >> 6;
    int nfail = 0, nchanged = 0;
    for (int tile = wave; tile < ntiles; tile += nwaves) {
        const int col = skip + 64 * tile + lane;
        const bool active = col < len;
        const uint8_t *src = grp + (active ? col : skip);
        uint8_t *dst = ogrp ? ogrp + (active ? col : skip) : nullptr;
        bool fail = true;
        uint32_t O[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) O[w] = 0;

        if (f > nroots) {
            /* every column fails as it came: nothing to compute */
            if (copy && active)
                for (int p = 0; p < n; p++) dst[(size_t)p * a.out_pitch] = src[(size_t)p * a.pitch];
        } else {
            uint32_t R[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) R[w] = 0;
            for (int p0 = 0; p0 < n; p0 += 4) {
                const int z = opaque_zero();
                unsigned by[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool there = L.hv[p0 + u] != 0;      /* uniform; 0 from n on */
                    by[u] = (there && active) ? src[(size_t)(p0 + u) * a.pitch] : 0u;
                    if (there && active && copy) dst[(size_t)(p0 + u) * a.out_pitch] = (uint8_t)by[u];
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (p0 + u < n) lfsr_step<NW>(R, by[u], L.gen, z);
            }
            if (f == 0) {
                uint32_t any = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) any |= R[w];
                fail = any != 0;
            } else {
                for (int l = 0; l < nroots; l++) {
                    const unsigned x = R[0] & 0xFFu;
                    shift_byte<NW>(R);
                    mul_acc<NW>(O, x, [&](int w, int b) { return L.tab[l][w][b]; });
                }
                /* the bytes from f on are the spare syndromes' sums */
                uint32_t any = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    const int lo = f - 4 * w;
                    const uint32_t mask = lo <= 0 ? 0xFFFFFFFFu : (lo >= 4 ? 0u : 0xFFFFFFFFu << (8 * lo));
                    any |= O[w] & mask;
                }
                fail = any != 0;
                /* the f missing places: the value, or in a failed column the byte that lay there */
                for (int j = 0; j < f; j++) {
                    const unsigned v = O[0] & 0xFFu;
                    shift_byte<NW>(O);
                    if (active) {
                        const size_t p = L.place[j];
                        const unsigned old = src[p * a.pitch];
                        const unsigned val = fail ? old : v;
                        nchanged += val != old ? 1 : 0;
                        if (dst && (copy || val != old)) dst[p * a.out_pitch] = (uint8_t)val;
                    }
                }
            }
        }
        if (active && a.colfail) a.colfail[g * (size_t)width + (size_t)(col - skip)] = fail ? 1 : 0;
        nfail += (active && fail) ? 1 : 0;
    }

    if (a.info) {      /* uniform */
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            nfail += __shfl_xor(nfail, o, 64);
            nchanged += __shfl_xor(nchanged, o, 64);
        }
        if (lane == 0) {
            L.cnt[wave][0] = nfail;
            L.cnt[wave][1] = nchanged;
        }
        __syncthreads();
        if (tid == 0) {
            int fails = 0, changed = 0;
            for (int w = 0; w < RSX_WAVES; w++) {
                fails += L.cnt[w][0];
                changed += L.cnt[w][1];
            }
            int32_t *info = a.info + 4 * g;
            info[0] = fails;
            info[1] = f;
            info[2] = changed;
            info[3] = fails == 0 ? 1 : 0;
        }
    }
}

struct CrossPlaceArgs {
    const uint8_t *bytes;
    size_t byte_pitch;
    const int32_t *count;
    const uint8_t *crc_ok;
    const int32_t *base;       /* or NULL */
    uint8_t *group;
    size_t pitch;
    uint8_t *have;
    int nstreams, max_packets, len, n, ngroups;
};

__global__ void __launch_bounds__(64 * RSX_WAVES)
rs_cross_place_kernel(CrossPlaceArgs a)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const unsigned s = blockIdx.x * (unsigned)RSX_WAVES + (unsigned)wave;
    if (s >= (unsigned)a.nstreams) return;      /* wave-uniform; no barrier follows */
    const int window = a.ngroups * a.n;         /* <= 256 */
    int count = a.count[s];
    count = count < 0 ? 0 : (count > a.max_packets ? a.max_packets : count);
    const unsigned base = a.base ? (unsigned)a.base[s] & 255u : 0u;
    const uint8_t *rows = a.bytes + (size_t)s * (size_t)a.max_packets * a.byte_pitch;
    const uint8_t *ok = a.crc_ok + (size_t)s * (size_t)a.max_packets;
    uint8_t *grp = a.group + (size_t)s * (size_t)window * a.pitch;      /* [ngroups][n] packets: slot d = (d / n, d % n) lies d pitches in */
    uint8_t *have = a.have + (size_t)s * (size_t)window;
    for (int i = 0; i < count; i++) {
        const uint8_t *row = rows + (size_t)i * a.byte_pitch;
        const unsigned d = ((unsigned)row[0] - base) & 255u;
        if (ok[i] == 0 || d >= (unsigned)window) continue;      /* uniform */
        uint8_t *dst = grp + (size_t)d * a.pitch;
        for (int c = lane; c < a.len; c += 64) dst[c] = row[c];
        if (lane == 0) have[d] = 1;
    }
}

/* the call's generator in the shift-and-xor form */
void cross_gen(int nroots, CrossGen *G)
{
    uint8_t gen[RS_MAX_ROOTS + 1];
    rs_generator(nroots, gen);
    for (int w = 0; w < 16; w++)
        for (int b = 0; b < 8; b++) {
            uint32_t word = 0;
            for (int c = 0; c < 4; c++) {
                const int l = 4 * w + c;
                const unsigned x = l < nroots ? gen[l + 1] : 0u;      /* slot l takes the coefficient of x^(nroots - 1 - l) */
                word |= (x ? (uint32_t)H_GF.exp[(unsigned)H_GF.log[x] + (unsigned)b] : 0u) << (8 * c);
            }
            G->g[w][b] = word;
        }
}

int cross_waves(int width)
{
    const int tiles = (width + 63) / 64;
    return tiles < RSX_WAVES ? tiles : RSX_WAVES;
}

} // namespace

int launch_rs_cross_encode(uint8_t *group, size_t pitch, int ngroups, int k, int nroots, int len, int skip, hipStream_t s)
{
    if (!group || ngroups < 1 || k < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || k + nroots > 255 || len < 1 || skip < 0 || skip >= len ||
        pitch < (size_t)len)
        return (int)hipErrorInvalidValue;
    CrossEncodeArgs a{};
    a.group = group;
    a.pitch = pitch;
    a.ngroups = ngroups;
    a.k = k;
    a.nroots = nroots;
    a.len = len;
    a.skip = skip;
    cross_gen(nroots, &a.gen);
    const dim3 grid((unsigned)ngroups), block(64u * (unsigned)cross_waves(len - skip));
    if (nroots <= 4)
        hipLaunchKernelGGL(rs_cross_encode_kernel<1>, grid, block, 0, s, a);
    else if (nroots <= 8)
        hipLaunchKernelGGL(rs_cross_encode_kernel<2>, grid, block, 0, s, a);
    else if (nroots <= 16)
        hipLaunchKernelGGL(rs_cross_encode_kernel<4>, grid, block, 0, s, a);
    else if (nroots <= 32)
        hipLaunchKernelGGL(rs_cross_encode_kernel<8>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(rs_cross_encode_kernel<16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_rs_cross_decode(const uint8_t *in, size_t pitch, int ngroups, int n, int nroots, int len, int skip, const uint8_t *have,
                           uint8_t *out, size_t out_pitch, int32_t *info, uint8_t *colfail, hipStream_t s)
{
    if (!in || !have || (!out && !info) || ngroups < 1 || nroots < 1 || nroots > RS_MAX_ROOTS || n <= nroots || n > 255 || len < 1 ||
        skip < 0 || skip >= len || pitch < (size_t)len || (out && out_pitch < (size_t)len))
        return (int)hipErrorInvalidValue;
    CrossDecodeArgs a{};
    a.in = in;
    a.pitch = pitch;
    a.out = out;
    a.out_pitch = out_pitch;
    a.have = have;
    a.info = info;
    a.colfail = colfail;
    a.ngroups = ngroups;
    a.n = n;
    a.nroots = nroots;
    a.len = len;
    a.skip = skip;
    cross_gen(nroots, &a.gen);
    const dim3 grid((unsigned)ngroups), block(64u * (unsigned)cross_waves(len - skip));
    if (nroots <= 4)
        hipLaunchKernelGGL(rs_cross_decode_kernel<1>, grid, block, 0, s, a);
    else if (nroots <= 8)
        hipLaunchKernelGGL(rs_cross_decode_kernel<2>, grid, block, 0, s, a);
    else if (nroots <= 16)
        hipLaunchKernelGGL(rs_cross_decode_kernel<4>, grid, block, 0, s, a);
    else if (nroots <= 32)
        hipLaunchKernelGGL(rs_cross_decode_kernel<8>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(rs_cross_decode_kernel<16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_rs_cross_place(const uint8_t *bytes, size_t byte_pitch, const int32_t *count, const uint8_t *crc_ok, int nstreams, int max_packets,
                          int len, int n, int ngroups, const int32_t *base, uint8_t *group, size_t pitch, uint8_t *have, hipStream_t s)
{
    if (!bytes || !count || !crc_ok || !group || !have || nstreams < 1 || max_packets < 1 || len < 1 || n < 1 || ngroups < 1 ||
        (long long)n * ngroups > 256 || byte_pitch < (size_t)len || pitch < (size_t)len)
        return (int)hipErrorInvalidValue;
    CrossPlaceArgs a{};
    a.bytes = bytes;
    a.byte_pitch = byte_pitch;
    a.count = count;
    a.crc_ok = crc_ok;
    a.base = base;
    a.group = group;
    a.pitch = pitch;
    a.have = have;
    a.nstreams = nstreams;
    a.max_packets = max_packets;
    a.len = len;
    a.n = n;
    a.ngroups = ngroups;
    const dim3 grid(((unsigned)nstreams + RSX_WAVES - 1) / RSX_WAVES), block(64 * RSX_WAVES);
    hipLaunchKernelGGL(rs_cross_place_kernel, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
