/*
 * nodesync.hip -- the node sync in front of the streaming decoder (NODE SYNC in include/qpsk_hip.h, restated in numpy by
 * tests/test_nodesync_cpu.py): per link a candidate (quarter turn r, delay h in dibits) applied to the soft rows, and the monitor that judges
 * it by the decoder's error count and moves on when it is bad.
 *
 * nodesync_push_kernel: ONE WAVE PER LINK, NS_WAVES of them in a workgroup, no barrier anywhere.  A wave
 *   1. reads its link's header (lanes 0..7) and the decoder's (e, n) of the previous block (lanes 0..1), runs the TICK on them -- every
 *      variable of it wave-uniform -- and stores the header and d_info from lanes 0..7.  The header a wave reads is the one the PREVIOUS launch
 *      wrote; no other wave touches it, so nothing a launch wrote is read back by it and the tick needs no double buffer;
 *   2. copies the link's carried history (the last nshift - 1 input dibits, raw) into its slice of the LDS, so that the delayed source of the
 *      first h outputs does not depend on when the history is rewritten;
 *   3. TRANSFORM: pure data movement at 2-byte granularity.  The output row is cut into a head (up to the first 16-byte boundary of the
 *      OUTPUT), a body of 8-dibit chunks stored as one aligned 16-byte vector each, and a tail.  A body chunk whose delayed source lies inside
 *      this push's row with a dibit to spare on either side is fetched as five aligned dwords and funnel-shifted by 0 or 16 bits (rows are only
 *      2-byte aligned and h moves the source by 2 h bytes, so the source is 0 or 2 bytes off a dword; which, is wave-uniform); every other
 *      chunk, the head and the tail are gathered a dibit at a time (the row, the history, or an erasure).  Both routes hand RAW dibits to ONE
 *      packed transform (turn_packed: the -128 rule, then the turn, four int8 at a time in integer arithmetic), so they cannot differ;
 *   4. stores the new history: the row's last nshift - 1 dibits (ntx >= nshift - 1, so they are all this push's).
 * Nothing between rows is read or written: the aligned dwords of the vector route cover only dibits k0 - 1 .. k0 + 9 of the row, k0 >= 1,
 * k0 + 10 <= ntx.
 *
 * STATE per link, NODESYNC_STRIDE bytes: 8 int32 { c, locked, run, err, cnt, settle_left, switches, 0 } and at byte 32 the history, slot k <
 * nshift - 1 = input dibit total - (nshift - 1) + k (two int8, raw: the -128 rule is the transform's).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "wave_sync.h"

namespace qpsk {

namespace {

constexpr int NS_WAVES = 4;
constexpr int NS_HDR = 32;
static_assert(NS_HDR + 2 * (NODESYNC_MAX_SHIFT - 1) <= (int)NODESYNC_STRIDE && NODESYNC_STRIDE % 4 == 0, "a link's header and history fit its state");

/* four int8 at once, (a0, b0, a1, b1) = two dibits: -128 -> -127, then turn_r.  No carry crosses a byte: the low seven bits of a byte
 * plus 1 reach bit 7 at most */
__device__ __forceinline__ unsigned turn_packed(unsigned x, int r)
{
    const unsigned t = x ^ 0x80808080u;
    x |= (~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu)) >> 7;      /* bytes that are 0x80 become 0x81 */
    if (r & 1) x = ((x >> 8) & 0x00ff00ffu) | ((x << 8) & 0xff00ff00u);       /* (a, b) -> (b, a) */
    const unsigned nx = ~x, neg = ((nx & 0x7f7f7f7fu) + 0x01010101u) ^ (nx & 0x80808080u);
    const unsigned m = r == 0 ? 0u : r == 1 ? 0xff00ff00u : r == 2 ? 0xffffffffu : 0x00ff00ffu;
    return (x & ~m) | (neg & m);
}

struct Source {
    const uint16_t *in;      /* this push's row */
    const uint16_t *hist;    /* the wave's copy of the carried history, H slots */
    int H, have;
    /* raw dibit k of the push, -H <= k < ntx: the row, the history, or an erasure where the link has not seen that dibit */
    __device__ __forceinline__ unsigned operator()(int k) const { return k >= 0 ? (unsigned)in[k] : -k <= have ? (unsigned)hist[H + k] : 0u; }
};

__global__ void __launch_bounds__(64 * NS_WAVES) nodesync_push_kernel(NodeSyncArgs a, int nlinks)
{
    __shared__ uint16_t hist_lds[NS_WAVES][NODESYNC_MAX_SHIFT];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int link = blockIdx.x * NS_WAVES + wave;
    if (link >= nlinks) return;      /* a whole wave: nothing below waits for another */
    uint8_t *state = a.state + (size_t)link * NODESYNC_STRIDE;
    int *hdr = reinterpret_cast<int *>(state);
    uint16_t *shist = reinterpret_cast<uint16_t *>(state + NS_HDR);
    const int H = a.nshift - 1, C = a.nrot * a.nshift;

    /* ---- 1. the tick */
    int c, locked, run, err, cnt, settle_left, switches, verdict = 0;
    {
        const int h = lane < 8 ? hdr[lane] : 0;
        c = __builtin_amdgcn_readlane(h, 0);
        locked = __builtin_amdgcn_readlane(h, 1);
        run = __builtin_amdgcn_readlane(h, 2);
        err = __builtin_amdgcn_readlane(h, 3);
        cnt = __builtin_amdgcn_readlane(h, 4);
        settle_left = __builtin_amdgcn_readlane(h, 5);
        switches = __builtin_amdgcn_readlane(h, 6);
    }
    if (a.vinfo) {
        const int v = lane < 2 ? a.vinfo[4 * (size_t)link + lane] : 0;
        const int e = __builtin_amdgcn_readlane(v, 0), n = __builtin_amdgcn_readlane(v, 1);
        if (n > 0) {
            if (settle_left > 0) {
                settle_left = max(0, settle_left - n);
                verdict = 3;
            } else {
                err += e;
                cnt += n;
                if (cnt >= a.span) {
                    const bool bad = (long long)err * a.thr_den > (long long)a.thr_num * cnt;
                    err = cnt = 0;
                    if (!bad) {
                        run = 0;
                        locked = 1;
                        verdict = 1;
                    } else {
                        verdict = 2;
                        run += 1;
                        if (!locked || run >= a.drop) {
                            c = c + 1 == C ? 0 : c + 1;
                            locked = 0;
                            run = 0;
                            settle_left = a.settle;
                            switches += 1;
                        }
                    }
                }
            }
        }
        if (lane < 7) hdr[lane] = lane == 0 ? c : lane == 1 ? locked : lane == 2 ? run : lane == 3 ? err : lane == 4 ? cnt : lane == 5 ? settle_left : switches;
    }
    const int r = c % a.nrot, h = c / a.nrot;
    if (a.info && lane < 8)
        a.info[8 * (size_t)link + lane] = lane == 0 ? r : lane == 1 ? h : lane == 2 ? locked : lane == 3 ? switches : lane == 4 ? verdict : lane == 5 ? run : lane == 6 ? err : cnt;

    /* ---- 2. the carried history into the LDS */
    uint16_t *lh = hist_lds[wave];
    if (lane < H) lh[lane] = shist[lane];
    wave_sync();

    /* ---- 3. the transform */
    const uint16_t *in = reinterpret_cast<const uint16_t *>(a.soft_in) + (size_t)link * a.in_pitch;
    uint16_t *out = reinterpret_cast<uint16_t *>(a.soft_out) + (size_t)link * a.out_pitch;
    const Source src = {in, lh, H, a.have};
    const int ntx = a.ntx;
    const int head = min(ntx, (int)(((16u - (unsigned)((uintptr_t)out & 15u)) & 15u) >> 1));
    const int nchunk = (ntx - head) >> 3, tail0 = head + 8 * nchunk;
    {
        /* head: lanes 0..6; tail: lanes 8..14 */
        const int j = lane < 8 ? (lane < head ? lane : -1) : (lane < 16 && tail0 + lane - 8 < ntx ? tail0 + lane - 8 : -1);
        if (j >= 0) out[j] = (uint16_t)turn_packed(src(j - h), r);
    }
    for (int q = lane; q < nchunk; q += 64) {
        const int j0 = head + 8 * q, k0 = j0 - h;
        unsigned o[4];
        if (k0 >= 1 && k0 + 10 <= ntx) {
            const uintptr_t p = (uintptr_t)(in + k0);
            const unsigned *w = reinterpret_cast<const unsigned *>(p & ~(uintptr_t)3);
            const unsigned sh = (unsigned)(p & 2u) * 8u;
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            o[0] = __funnelshift_r(w0, w1, sh);
            o[1] = __funnelshift_r(w1, w2, sh);
            o[2] = __funnelshift_r(w2, w3, sh);
            o[3] = __funnelshift_r(w3, w4, sh);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = src(k0 + 2 * i) | (src(k0 + 2 * i + 1) << 16);
        }
        uint4 v;
        v.x = turn_packed(o[0], r);
        v.y = turn_packed(o[1], r);
        v.z = turn_packed(o[2], r);
        v.w = turn_packed(o[3], r);
        *reinterpret_cast<uint4 *>(out + j0) = v;
    }

    /* ---- 4. the history behind this push */
    if (lane < H) shist[lane] = in[ntx - H + lane];
}

/* a reset's state (every word and the history zero), or qpsk_nodesync_set's (the candidate, a fresh monitor; history and switches stay) */
__global__ void __launch_bounds__(64) nodesync_init_kernel(NodeSyncArgs a, int nlinks, const int32_t *cand, bool keep)
{
    const int link = blockIdx.x * 64 + threadIdx.x;
    if (link >= nlinks) return;
    int *w = reinterpret_cast<int *>(a.state + (size_t)link * NODESYNC_STRIDE);
    if (keep) {
        w[0] = (int)(cand ? (unsigned)cand[link] % (unsigned)(a.nrot * a.nshift) : 0u);
        w[1] = w[2] = w[3] = w[4] = 0;
        w[5] = a.settle;
    } else {
        for (int i = 0; i < (int)(NODESYNC_STRIDE / 4); i++) w[i] = 0;
    }
}

} // namespace

static bool nodesync_geometry_fits(const NodeSyncArgs &a, int nlinks)
{
    return nlinks >= 1 && a.state && (a.nrot == 1 || a.nrot == 2 || a.nrot == 4) && a.nshift >= 1 && a.nshift <= NODESYNC_MAX_SHIFT && a.span >= 1 &&
           a.span <= (1 << 24) && a.settle >= 0 && a.settle <= (1 << 24) && a.thr_num >= 0 && a.thr_num <= 65535 && a.thr_den >= 1 &&
           a.thr_den <= 65535 && a.drop >= 1 && a.drop <= 16;
}

int launch_nodesync_init(const NodeSyncArgs &a, int nlinks, const int32_t *cand, bool keep, hipStream_t s)
{
    if (!nodesync_geometry_fits(a, nlinks) || (cand && !keep)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(nodesync_init_kernel, dim3((unsigned)((nlinks + 63) / 64)), dim3(64), 0, s, a, nlinks, cand, keep);
    return (int)hipGetLastError();
}

int launch_nodesync_push(const NodeSyncArgs &a, int nlinks, hipStream_t s)
{
    if (!nodesync_geometry_fits(a, nlinks) || !a.soft_in || !a.soft_out || a.ntx < 1 || a.ntx < a.nshift - 1 || a.ntx > NODESYNC_MAX_NTX ||
        a.in_pitch < (size_t)a.ntx || a.out_pitch < (size_t)a.ntx || a.have < 0 || a.have > a.nshift - 1 || (uintptr_t)a.soft_in % 2 ||
        (uintptr_t)a.soft_out % 2)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(nodesync_push_kernel, dim3((unsigned)((nlinks + NS_WAVES - 1) / NS_WAVES)), dim3(64 * NS_WAVES), 0, s, a, nlinks);
    return (int)hipGetLastError();
}

} // namespace qpsk
