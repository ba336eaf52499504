/*
 * deframe_hunt.h -- the sync-word hunt of both deframers (deframe.hip, deframe_coded.hip), written once: one wave per stream, the new row
 * behind the stream's carried tail, every position whose word is complete scored against the sync word, the hunt / collect state walked
 * over the candidates.  What a packet's payload becomes is the caller's policy.
 *
 * A stream's sequence D is everything pushed since the reset; X = [the last T = min(len, nsync-1) values of D][this push's row] is the
 * part this push reads.  Position p_x of X starts a word that completes in THIS push (its last dibit lies in the row), so every position
 * of D is scored exactly once, in the push that brings its last dibit.  A packet found in this push has its payload starting in the
 * row (p* + nsync > len); a packet still collecting at the end of a push keeps its received payload dibits in the stream's pending
 * buffer and is completed by a later push.
 *
 * Scoring in bit planes.  The ring values of X are two planes of bits (bit 0, bit 1), built 64 positions at a time by two ballots of a
 * coalesced load, so a plane word is wave-uniform.  Lane l of step s scores position 64 s + l: its 64-position windows are funnel
 * shifts of three consecutive plane words, and with the sync word's planes in the kernel arguments
 *     diff = (x - s) & 3:   diff0 = x0 ^ s0,   diff1 = x1 ^ s1 ^ (~x0 & s0)
 * one popcount per rotation counts the word's dibits matching under that rotation (sync.hip's score, the same tie rule).  A ballot of
 * "best score >= min_score" is the step's candidate mask; the hunt walks it in wave-uniform code: O(packets + steps).
 *
 * The policy, with N payload dibits to a packet (all calls are made by the whole wave, in wave-uniform code):
 *     unsigned ring(long long i)                          the ring value of row symbol i
 *     void complete(slot, pos, rot, score, have, row0)    packet `slot` of this push is finished: its first `have` payload dibits are in
 *                                                         the pending buffer, the other N - have start at row symbol row0
 *     void collect(have, row0, cnt, rot)                  append row symbols [row0, row0 + cnt) to the pending buffer at `have`
 */
#ifndef QPSK_DEFRAME_HUNT_H
#define QPSK_DEFRAME_HUNT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "qpsk_device.h"
#include "deframe_bits.h"

namespace qpsk {

constexpr int HUNT_WAVES = 4;     /* streams per workgroup: one wave each */
constexpr int HUNT_CHUNK = 4;     /* steps of 64 positions per load batch (4 + 2 plane words): more spills SGPRs */

__device__ __forceinline__ unsigned ring_at(const float2 *row, long long i) { return ring_of((unsigned)data_rule(row[i])); }

/* one push of stream `stream` (st: its state); complete() is called for the packets below cap, all are counted */
template <class Policy>
__device__ __forceinline__ void deframe_hunt(const DeframeHuntArgs &a, int stream, int N, int cap, uint8_t *st, Policy &p)
{
    const int lane = threadIdx.x & 63;
    const int n = a.nsync;
    const long long nsym = a.nsym;
    DeframeHeader *hd = reinterpret_cast<DeframeHeader *>(st);
    uint8_t *tail = st + DEFRAME_TAIL_OFFSET;

    const long long len = hd->len;
    long long h = hd->h;
    int pending = hd->pending, have = hd->have;
    const int T = (int)(len < (long long)(n - 1) ? len : (long long)(n - 1));
    int count = 0;

    /* 1. the packet collecting since an earlier push */
    if (pending) {
        const long long ppos = hd->ppos;
        const int prot = hd->prot, pscore = hd->pscore;
        if (nsym >= N - have) {
            if (count < cap) p.complete(count, ppos, prot, pscore, have, 0);
            count++;
            pending = 0;
        } else {
            p.collect(have, 0, (int)nsym, prot);
            have += (int)nsym;
        }
    }

    /* 2. the hunt over the positions whose word completes in this push: p_x in [0, P), global p = len - T + p_x; in-push offsets are
     *    32-bit (X < 2^22), hx = h - (len - T) */
    const long long base0 = len - T;
    const int X = T + (int)nsym;
    const int P = X - n + 1;
    if (!pending && P > 0 && h < base0 + P) {
        int hx = h > base0 ? (int)(h - base0) : 0;
        const int s0 = hx >> 6;                                          /* steps below h hold no candidate */
        const int steps = (P + 63) >> 6;
        auto xload = [&](int w) -> unsigned {
            const int j = 64 * w + lane;
            if (j >= X) return 0u;
            return j < T ? (unsigned)tail[j] : p.ring(j - T);
        };
        const unsigned long long m0 = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        const unsigned long long m1 = n > 64 ? (n == 128 ? ~0ull : ((1ull << (n - 64)) - 1ull)) : 0ull;
        bool moved = false;
        /* a chunk: steps s .. s + HUNT_CHUNK - 1 from plane words s .. s + HUNT_CHUNK + 1.  The words are not kept across a packet (the
         * packet's work needs the registers): the chunk after a packet starts at the step that holds the new hx */
        for (int s = s0; s < steps;) {
            unsigned long long lo[HUNT_CHUNK + 2], hi[HUNT_CHUNK + 2];
            {
                unsigned v[HUNT_CHUNK + 2];
#pragma unroll
                for (int k = 0; k < HUNT_CHUNK + 2; k++) v[k] = k < 2 || s + k - 2 < steps ? xload(s + k) : 0u;
#pragma unroll
                for (int k = 0; k < HUNT_CHUNK + 2; k++) { lo[k] = ballot64(v[k] & 1u); hi[k] = ballot64(v[k] & 2u); }
            }
            int px = -1, pk = 0;
#pragma unroll
            for (int k = 0; k < HUNT_CHUNK; k++) {
                const int gx = 64 * (s + k);
                if (px >= 0 || s + k >= steps || gx + 63 < hx) continue;
                const unsigned long long x0 = funnel64(lo[k], lo[k + 1], lane), x1 = funnel64(hi[k], hi[k + 1], lane);
                unsigned long long d0 = x0 ^ a.sync_lo[0];
                unsigned long long d1 = x1 ^ a.sync_hi[0] ^ (~x0 & a.sync_lo[0]);
                int c1 = __popcll(~d1 & d0 & m0), c2 = __popcll(d1 & ~d0 & m0), c3 = __popcll(d1 & d0 & m0);
                if (n > 64) {
                    const unsigned long long y0 = funnel64(lo[k + 1], lo[k + 2], lane), y1 = funnel64(hi[k + 1], hi[k + 2], lane);
                    d0 = y0 ^ a.sync_lo[1];
                    d1 = y1 ^ a.sync_hi[1] ^ (~y0 & a.sync_lo[1]);
                    c1 += __popcll(~d1 & d0 & m1); c2 += __popcll(d1 & ~d0 & m1); c3 += __popcll(d1 & d0 & m1);
                }
                int best = n - c1 - c2 - c3, r = 0;                      /* the first rotation with the largest count */
                if (c1 > best) { best = c1; r = 1; }
                if (c2 > best) { best = c2; r = 2; }
                if (c3 > best) { best = c3; r = 3; }
                const unsigned long long mask = ballot64(gx + lane < P && gx + lane >= hx && best >= a.min_score);
                if (mask) {
                    const int l = __builtin_ctzll(mask);
                    pk = __builtin_amdgcn_readlane(best * 4 + r, l);
                    px = gx + l;
                }
            }
            if (px < 0) {
                s += HUNT_CHUNK;
                continue;
            }
            hx = px + n + N;
            moved = true;
            const int row0 = px + n - T;                                 /* >= 0: the payload starts in the row */
            if (hx > X) {                                                /* collects into the next pushes */
                const int got = (int)nsym - row0;
                p.collect(0, row0, got, pk & 3);
                pending = 1;
                have = got;
                if (lane == 0) { hd->ppos = base0 + px; hd->prot = pk & 3; hd->pscore = pk >> 2; }
                break;
            }
            if (count < cap) p.complete(count, base0 + px, pk & 3, pk >> 2, 0, row0);      /* row0 + N <= nsym: the payload lies in the row */
            count++;
            s = hx >> 6;
        }
        if (moved) h = base0 + hx;
    }

    /* 3. the carried tail: the last min(len + nsym, nsync - 1) values of D, read before any lane writes */
    const long long len2 = len + nsym;
    const int T2 = X < n - 1 ? X : n - 1;
    unsigned tv[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int i = lane + 64 * q;
        const int j = X - T2 + i;
        tv[q] = i < T2 ? (j < T ? (unsigned)tail[j] : p.ring(j - T)) : 0u;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int i = lane + 64 * q;
        if (i < T2) tail[i] = (uint8_t)tv[q];
    }
    if (lane == 0) {
        hd->len = len2;
        hd->h = h;
        hd->pending = pending;
        hd->have = have;
        a.count[stream] = count;
    }
}

} // namespace qpsk
#endif
