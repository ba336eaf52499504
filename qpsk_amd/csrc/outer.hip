/*
 * outer.hip -- the outer link of a continuous stream (OUTER LINK in include/qpsk_hip.h, restated in numpy by tests/test_outer_cpu.py): word
 * sync with polarity resolution, the convolutional (Forney) byte deinterleaver and aligned words out, and the interleaver that is its
 * transmit twin.
 *
 * outer_push_kernel: ONE WAVE PER STREAM, OUTER_WAVES of them in a workgroup, no barrier anywhere (a wave leaves its loops when ITS stream is
 * through).  A wave works on a WINDOW of raw received bits in its slice of the LDS: what the stream's ring held, and behind it the push, a
 * chunk of OUTER_CHUNK bytes at a time, appended at the bit phase total & 7 (the window begins at a multiple of 8 bits since the reset, so the
 * phase is the same for every stream: a launch constant).  Over the window runs the state machine of the header, every variable of it
 * wave-uniform, as far as the bits allow:
 *   HUNT     lane = candidate bit position, 64 candidates a round; a lane forms its L bytes from two window bytes each and a shift; one ballot,
 *            the first set bit wins.  Candidates whose look-ahead has not arrived end the round, and h stays where they begin.
 *   LOCKED   per completed raw word the sync byte is formed by every lane alike (wave-uniform), the n bytes of Z are a lane-parallel gather at
 *            bit phase u0 & 7 out of I raw words of the window, stored coalesced; lane 0 stores pos and flags.
 * When the machine can go no further, the window is moved down to the first byte it still needs (the oldest raw word in flight, or h) and
 * the next chunk is appended; what is left after the last chunk goes back into the ring.  What stays is bounded by the geometry, not by the
 * push: at most max(I, L) n + 2 bytes (LOCKED: the I - 1 words in flight and a word not yet whole; HUNT: the look-ahead of the first
 * undecided candidate).
 *
 * STATE per stream, state_stride bytes (outer_state_stride): 8 int32 { locked, p, s, c, run, kbits, gk, 0 } and the ring at byte 32.  p is h, or
 * the first bit of raw word c, counted from the ring's first bit; c is capped at I - 1; kbits is what the ring holds; gk is the group index of
 * raw word c under group sync (c is capped, so k(c) is carried) and 0 without it.  Every word of the state
 * is written with ordinary vector stores at the end of a launch and read at the start of the next; inside a launch the window lives in the
 * LDS, where a wave's accesses are in order, so nothing a launch wrote to memory is read back by it.
 *
 * outer_interleave_kernel: the same gather without a bit phase, one thread per byte of the output and of d_hist_out.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "wave_sync.h"

namespace qpsk {

namespace {

constexpr int OUTER_WAVES = 4;
constexpr int OUTER_CHUNK = 1024;      /* bytes of a push appended at a time */
constexpr int OUTER_HDR = 32;

__host__ __device__ constexpr int outer_ring_bytes(int n, int branches, int lock) { return ((branches > lock ? branches : lock) * n + 8 + 15) & ~15; }
/* a wave's slice of the LDS: the ring, a chunk, the byte a phase spills into, and what a two-byte read may touch behind the last bit */
__host__ __device__ constexpr int outer_slice_bytes(int n, int branches, int lock) { return outer_ring_bytes(n, branches, lock) + OUTER_CHUNK + 16; }

/* V(u) over the window */
template <bool MSB>
__device__ __forceinline__ unsigned window_byte(const uint8_t *w, int u)
{
    const int b = u >> 3;
    const unsigned v = ((((unsigned)w[b + 1] << 8) | (unsigned)w[b]) >> (u & 7)) & 255u;
    return MSB ? __brev(v) >> 24 : v;
}

/* m(u): +1, -1 or 0 */
template <bool MSB>
__device__ __forceinline__ int window_match(const uint8_t *w, int u, unsigned sync, bool polarity)
{
    const unsigned v = window_byte<MSB>(w, u);
    return v == sync ? 1 : (polarity && v == (sync ^ 255u)) ? -1 : 0;
}

/* GROUP: group sync (qpsk_outer_reset_group), a variant at compile time so that the ungrouped instantiations keep their code.  What it adds is
 * gk = k(c), the group index of the raw word at p (header slot 6), and in HUNT a lane's mask of the signs of its L bytes, bit i = (m(u + 8 n i)
 * < 0).  The legal masks of s = +1 are the G shifts of ONE wave-uniform mask, p0 = the bits i = 0, G, 2 G, ... (formed once per launch): P_g =
 * (p0 << f) & lmask with f = (G - g) mod G the place of its first set bit, and f < G because L >= G; those of s = -1 are their complements in
 * lmask.  So a lane compares its mask x (or its complement) with the one legal mask that has x's first set bit, instead of with all G. */
template <bool MSB, bool GROUP>
__device__ __forceinline__ void outer_push(const OuterArgs &a, uint8_t *w, int stream, int lane)
{
    const int n = a.n, I = a.branches, L = a.lock;
    const int wordbits = 8 * n, span = wordbits * (L - 1) + 8;      /* HUNT: the bits a candidate needs from its own first bit on */
    const unsigned sync = (unsigned)a.sync;
    const bool polarity = (a.flags & OUTER_POLARITY) != 0;
    const int G = GROUP ? a.group : 1;
    const unsigned lmask = (1u << L) - 1u;
    unsigned p0 = 0;
    if (GROUP)
        for (int i = 0; i < L; i += G) p0 |= 1u << i;
    uint8_t *state = a.state + (size_t)stream * a.state_stride;
    int *hdr = reinterpret_cast<int *>(state);
    int locked, p, s, c, run, avail, gk = 0;
    {
        const int h = lane < 8 ? hdr[lane] : 0;
        locked = __builtin_amdgcn_readlane(h, 0);
        p = __builtin_amdgcn_readlane(h, 1);
        s = __builtin_amdgcn_readlane(h, 2);
        c = __builtin_amdgcn_readlane(h, 3);
        run = __builtin_amdgcn_readlane(h, 4);
        avail = __builtin_amdgcn_readlane(h, 5);
        if (GROUP) gk = __builtin_amdgcn_readlane(h, 6);
    }
    {
        const unsigned *ring = reinterpret_cast<const unsigned *>(state + OUTER_HDR);
        unsigned *w4 = reinterpret_cast<unsigned *>(w);
        const int nd = (avail + 31) >> 5;
        for (int i = lane; i < nd; i += 64) w4[i] = ring[i];
        wave_sync();
    }
    long long pos0 = a.total - avail;      /* the window's first bit, counted from the reset */
    const int ph = (int)(a.total & 7);
    const uint8_t *in = a.bits + (size_t)stream * a.bits_pitch;
    const int nin = (a.nbits + 7) >> 3;
    const unsigned lastmask = (a.nbits & 7) ? (1u << (a.nbits & 7)) - 1u : 255u;
    uint8_t *words = a.words ? a.words + (size_t)stream * (size_t)a.max_words * a.word_pitch : nullptr;
    int count = 0, nlock = 0, nlost = 0;
    /* q mod I of the up to four bytes of a word a lane gathers */
    int back[4];
#pragma unroll
    for (int k = 0; k < 4; k++) back[k] = I - 1 - (lane + 64 * k) % I;

    for (int g0 = 0; g0 < nin; g0 += OUTER_CHUNK) {
        /* ---- append input bytes [g0, g1) at bit `avail` (avail & 7 == ph) */
        const int g1 = min(g0 + OUTER_CHUNK, nin);
        {
            const int kb = avail >> 3, nout = g1 - g0 + (ph ? 1 : 0);
            unsigned carry = (unsigned)w[kb] & ((1u << ph) - 1u);      /* the partial byte the window ends with, already in place */
            for (int k = 0; k < nout; k += 64) {
                const int j = g0 + k + lane;
                unsigned cur = j < g1 ? (unsigned)in[j] : 0u;
                if (j == nin - 1) cur &= lastmask;
                unsigned low = (unsigned)__shfl_up((int)cur, 1, 64) >> (8 - ph);
                if (lane == 0) low = carry;
                if (k + lane < nout) w[kb + k + lane] = (uint8_t)((cur << ph) | low);
                carry = (unsigned)__builtin_amdgcn_readlane((int)cur, 63) >> (8 - ph);
            }
            avail += g1 == nin ? a.nbits - 8 * g0 : 8 * (g1 - g0);
            wave_sync();
        }
        /* ---- the state machine, as far as the window allows */
        for (;;) {
            if (!locked) {
                const int nv = min(avail - span - p + 1, 64);      /* the candidates of this round whose look-ahead is in */
                if (nv <= 0) break;
                const int u = p + lane;
                int m = 0;
                if (lane < nv) m = window_match<MSB>(w, u, sync, GROUP || polarity);
                bool hit = m != 0;
                unsigned x = m < 0 ? 1u : 0u;      /* GROUP: the signs of the L bytes */
                for (int i = 1; i < L && __ballot(hit); i++)      /* the look-ahead, as long as a candidate is left */
                    if (hit) {
                        const int mi = window_match<MSB>(w, u + i * wordbits, sync, GROUP || polarity);
                        if (GROUP) {
                            hit = mi != 0;
                            x |= (mi < 0 ? 1u : 0u) << i;
                        } else
                            hit = mi == m;
                    }
                int sg = 0;      /* GROUP: g, and 16 where s < 0 */
                if (GROUP && hit) {
                    const unsigned y = ~x & lmask;
                    const int fx = __ffs((int)x) - 1, fy = __ffs((int)y) - 1;
                    if (x && fx < G && x == ((p0 << fx) & lmask)) sg = (G - fx) % G;
                    else if (polarity && y && fy < G && y == ((p0 << fy) & lmask)) sg = 16 | (G - fy) % G;
                    else hit = false;      /* L sync bytes in a sign pattern no (s, g) gives: not a lock */
                }
                const unsigned long long hits = __ballot(hit);
                if (hits) {
                    const int first = __ffsll((long long)hits) - 1;
                    if (GROUP) {
                        sg = __builtin_amdgcn_readlane(sg, first);
                        s = sg & 16 ? -1 : 1;
                        gk = sg & 15;
                    } else
                        s = (__ballot(hit && m > 0) >> first) & 1ull ? 1 : -1;
                    p += first;
                    locked = 1;
                    c = run = 0;
                    nlock++;
                } else {
                    p += nv;
                    if (nv < 64) break;
                }
            } else {
                if (p + wordbits > avail) break;
                const unsigned inv = s < 0 ? 255u : 0u;
                const bool miss = (window_byte<MSB>(w, p) ^ inv) != (GROUP && gk == 0 ? sync ^ 255u : sync);      /* E(c) */
                run = miss ? run + 1 : 0;
                if (a.drop > 0 && run == a.drop) {
                    locked = 0;
                    p += 1;
                    nlost++;
                    if (GROUP) gk = 0;      /* g is forgotten */
                    continue;
                }
                if (c >= I - 1) {
                    if (count < a.max_words) {
                        const int first = p - wordbits * (I - 1);      /* raw word c - (I - 1) */
                        if (words) {
                            uint8_t *dst = words + (size_t)count * a.word_pitch;
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const int q = lane + 64 * k;
                                if (q < n) dst[q] = (uint8_t)(window_byte<MSB>(w, p - wordbits * back[k] + 8 * q) ^ inv);
                            }
                        }
                        if (lane == 0) {
                            const size_t at = (size_t)stream * (size_t)a.max_words + (size_t)count;
                            if (a.pos) a.pos[at] = pos0 + p;
                            if (GROUP) {
                                const unsigned kz = (unsigned)((gk - (I - 1) % G + G) % G);      /* k(c - (I - 1)) */
                                const unsigned ez = kz == 0 ? sync ^ 255u : sync;
                                if (a.wflags) a.wflags[at] = (uint8_t)(((window_byte<MSB>(w, first) ^ inv) != ez ? 1u : 0u) | (s < 0 ? 2u : 0u) | kz << 4);
                            } else if (a.wflags)
                                a.wflags[at] = (uint8_t)(((window_byte<MSB>(w, first) ^ inv) != sync ? 1u : 0u) | (s < 0 ? 2u : 0u));
                        }
                    }
                    count++;
                }
                c = min(c + 1, I - 1);
                if (GROUP) gk = gk + 1 == G ? 0 : gk + 1;
                p += wordbits;
            }
        }
        /* ---- move the window down to the first byte still needed */
        {
            const int off = (locked ? p - wordbits * c : p) >> 3;
            if (off > 0) {
                const int nb = ((avail + 7) >> 3) - off;
                for (int k = 0; k < nb; k += 64) {
                    const int i = k + lane;
                    const uint8_t v = i < nb ? w[off + i] : (uint8_t)0;
                    wave_sync();
                    if (i < nb) w[i] = v;
                    wave_sync();
                }
                p -= 8 * off;
                avail -= 8 * off;
                pos0 += 8 * off;
            }
        }
    }
    /* ---- what is left goes back into the ring; the bytes of the last dword beyond the window are zeroed first */
    {
        const int nb = (avail + 7) >> 3, nd = (nb + 3) >> 2;
        if (lane < 4 && nb + lane < 4 * nd) w[nb + lane] = 0;
        wave_sync();
        unsigned *ring = reinterpret_cast<unsigned *>(state + OUTER_HDR);
        const unsigned *w4 = reinterpret_cast<const unsigned *>(w);
        for (int i = lane; i < nd; i += 64) ring[i] = w4[i];
        if (GROUP) {
            if (lane < 7) hdr[lane] = lane == 0 ? locked : lane == 1 ? p : lane == 2 ? s : lane == 3 ? c : lane == 4 ? run : lane == 5 ? avail : gk;
        } else if (lane < 6)
            hdr[lane] = lane == 0 ? locked : lane == 1 ? p : lane == 2 ? s : lane == 3 ? c : lane == 4 ? run : avail;
    }
    if (lane == 0) a.count[stream] = count;
    if (a.info && lane < 4) a.info[4 * (size_t)stream + lane] = lane == 0 ? locked : lane == 1 ? (locked ? s : 0) : lane == 2 ? nlock : nlost;
}

template <bool GROUP>
__global__ void __launch_bounds__(64 * OUTER_WAVES) outer_push_kernel(OuterArgs a, int nstreams)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t outer_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int stream = blockIdx.x * OUTER_WAVES + wave;
    if (stream >= nstreams) return;      /* a whole wave: nothing below waits for another */
    uint8_t *w = outer_lds + (size_t)wave * outer_slice_bytes(a.n, a.branches, a.lock);
    if (a.flags & OUTER_MSB_FIRST) outer_push<true, GROUP>(a, w, stream, lane);
    else outer_push<false, GROUP>(a, w, stream, lane);
}

/* a reset's state: HUNT from bit 0 over an empty ring */
__global__ void __launch_bounds__(64) outer_init_kernel(OuterArgs a, int nstreams)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (size_t)nstreams * 8) return;
    reinterpret_cast<int *>(a.state + (i >> 3) * a.state_stride)[i & 7] = 0;
}

struct InterleaveArgs {
    const uint8_t *in, *hist_in;
    uint8_t *hist_out, *out;
    size_t nrows;
    int nwords, n, branches;
};

/* source word c of a row, c >= -(I - 1): the call's, or the history's, or zeros */
__device__ __forceinline__ uint8_t interleave_source(const InterleaveArgs &a, size_t row, int c, int q)
{
    if (c >= 0) return a.in[(row * (size_t)a.nwords + (size_t)c) * a.n + q];
    return a.hist_in ? a.hist_in[(row * (size_t)(a.branches - 1) + (size_t)(c + a.branches - 1)) * a.n + q] : (uint8_t)0;
}

/* one thread per byte: of the nwords output words of a row, then of the I - 1 words of its d_hist_out */
__global__ void __launch_bounds__(256) outer_interleave_kernel(InterleaveArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_row = (size_t)(a.nwords + (a.hist_out ? a.branches - 1 : 0)) * a.n;
    if (i >= a.nrows * per_row) return;
    const size_t row = i / per_row;
    const unsigned r = (unsigned)(i - row * per_row);
    const int c = (int)(r / (unsigned)a.n), q = (int)(r % (unsigned)a.n);
    if (c < a.nwords) a.out[(row * (size_t)a.nwords + (size_t)c) * a.n + q] = interleave_source(a, row, c - q % a.branches, q);
    else {
        const int k = c - a.nwords;      /* word k of the history behind the call: source word nwords - (I - 1) + k */
        a.hist_out[(row * (size_t)(a.branches - 1) + (size_t)k) * a.n + q] = interleave_source(a, row, a.nwords - (a.branches - 1) + k, q);
    }
}

} // namespace

size_t outer_state_stride(int n, int branches, int lock) { return (size_t)OUTER_HDR + (size_t)outer_ring_bytes(n, branches, lock); }

static bool outer_geometry_fits(const OuterArgs &a, int nstreams)
{
    return nstreams >= 1 && a.state && a.n >= 2 && a.n <= 255 && a.branches >= 1 && a.branches <= 32 && a.n % a.branches == 0 && a.sync >= 0 &&
           a.sync <= 255 && a.lock >= 1 && a.lock <= 16 && a.drop >= 0 && a.drop <= 16 && !(a.flags & ~(OUTER_POLARITY | OUTER_MSB_FIRST)) &&
           a.state_stride >= outer_state_stride(a.n, a.branches, a.lock) && a.state_stride % 4 == 0 &&
           (a.group == 0 || (a.group >= 3 && a.group <= 16 && a.lock >= a.group));
}

int launch_outer_init(const OuterArgs &a, int nstreams, hipStream_t s)
{
    if (!outer_geometry_fits(a, nstreams)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(outer_init_kernel, dim3((unsigned)(((size_t)nstreams * 8 + 63) / 64)), dim3(64), 0, s, a, nstreams);
    return (int)hipGetLastError();
}

int launch_outer_push(const OuterArgs &a, int nstreams, hipStream_t s)
{
    if (!outer_geometry_fits(a, nstreams) || !a.bits || !a.count || a.nbits < 1 || a.nbits > OUTER_MAX_BITS || a.max_words < 0 || a.total < 0 ||
        a.bits_pitch < (size_t)((a.nbits + 7) >> 3) || (a.words && a.word_pitch < (size_t)a.n))
        return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)OUTER_WAVES * outer_slice_bytes(a.n, a.branches, a.lock);
    const dim3 grid((unsigned)((nstreams + OUTER_WAVES - 1) / OUTER_WAVES));
    if (a.group) hipLaunchKernelGGL(outer_push_kernel<true>, grid, dim3(64 * OUTER_WAVES), lds, s, a, nstreams);
    else hipLaunchKernelGGL(outer_push_kernel<false>, grid, dim3(64 * OUTER_WAVES), lds, s, a, nstreams);
    return (int)hipGetLastError();
}

int launch_outer_interleave(const uint8_t *words, int nrows, int nwords, int n, int branches, const uint8_t *hist_in, uint8_t *hist_out,
                            uint8_t *out, hipStream_t s)
{
    if (!words || !out || nrows < 1 || nwords < 1 || n < 2 || n > 255 || branches < 1 || branches > 32 || n % branches) return (int)hipErrorInvalidValue;
    if (branches == 1) hist_out = nullptr;      /* no history: nothing to write */
    const size_t total = (size_t)nrows * (size_t)(nwords + (hist_out ? branches - 1 : 0)) * (size_t)n;
    if ((size_t)(nwords + branches) * (size_t)n > 0xffffffffull || (total + 255) / 256 > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const InterleaveArgs a = {words, branches > 1 ? hist_in : nullptr, hist_out, out, (size_t)nrows, nwords, n, branches};
    hipLaunchKernelGGL(outer_interleave_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace qpsk
