/*
 * rx_pipe2_geom.h -- the two-frame unit geometry of rx_pipe2_kernel (rx_pipe2.hip), which rx_lean_kernel (rx_lean.hip) lays its windows out
 * by and rx_hist_kernel (rx_hist.hip) takes its chunk size from, and the ring rows and control block of rx_lean_kernel, which rx_hist_kernel
 * uses as they are.  Every static_assert stands beside the constants it guards; those on a generated stream's constants stand in the unit
 * that includes the stream.
 */
#ifndef QPSK_RX_PIPE2_GEOM_H
#define QPSK_RX_PIPE2_GEOM_H
#include "rx_pipe.h"

namespace qpsk {

#define QPSK_PIPE2_MAXFIR 9  /* FIR waves per workgroup: three per SIMD, so at most 168 VGPRs.  (Two per SIMD with three units
                                each and a deeper LDS prefetch in 256 VGPRs: 0.31 against 0.29 ms at 8192 frames.) */
namespace pipe2 {
constexpr int QL = 32, R = 2, UF = 2;                    /* lanes per frame, symbols per lane, frames per unit */
constexpr int S = GeomNarrow::S, CH = S * C;              /* 64 symbols = 512 samples per chunk per frame */
constexpr int PAD = R * C, PADS = 2;                      /* position p lives at slot p + 2 (p/16): lanes 18 slots = 144 bytes apart, so a
                                                             lane's positions (t, t+1), t even, are one aligned 16-byte word and the
                                                             16 lanes of a ds_read_b128 pass start in 16 different bank quads */
constexpr int TSTEPS = NTAPS + C * (R - 1);               /* 135 window positions per lane per chunk */
constexpr int NLD = CH / 128;                             /* 16-byte loads per frame per chunk */
constexpr int BLK = 128 + PADS * (128 / PAD);             /* slots per 128-sample block */
constexpr int WS = 720;                                   /* slots per frame window: positions 0..637 -> slots 0..715 */
__device__ __host__ constexpr int slot_of(int p) { return p + PADS * (p / PAD); }
constexpr int MAX_UNITS = 16, MAX_FIR = QPSK_PIPE2_MAXFIR, MAX_UW = (MAX_UNITS + MAX_FIR - 1) / MAX_FIR;   /* units per workgroup, FIR waves, units per FIR wave */
constexpr int MAX_THREADS = 64 * (MAX_FIR + 1 + (MAX_FIR - 1) / 3);   /* 12 hardware waves */
static_assert(S == QL * R && CH % 128 == 0 && slot_of(CH + HIST - 1) < WS && WS % 2 == 0 && PAD % 2 == 0 &&
              PAD * (QL - 1) + TSTEPS - 1 <= CH + HIST - 1 - (C - 1), "window geometry: every position a lane reads is written for every index < C");
static_assert(MAX_UNITS <= MAX_WAVES, "one ready[] counter per unit");

/* what a FIR wave keeps per unit (wave-uniform except where noted) */
struct Unit {
    int u;                    /* unit number in the workgroup = its ready[] counter; frames 2u, 2u + 1 */
    bool fv[UF], all_valid;   /* frames inside the batch */
    const float4 *src[UF];
    int ix[UF];               /* the frames' decimation offsets (< C): sample 2*lane of a chunk lives at window position
                                 2*lane + HIST - ix; when ix is even the lane's pair is one aligned 16-byte word */
    float4 hist[UF];          /* per lane: the pair it loaded from the LAST block of the previous chunk */
};
} // namespace pipe2

/* rx_lean_kernel's LDS control block and ring rows (the whole LDS picture: rx_lean.hip, which adds the windows and the parameter blocks) */
namespace lean {
struct Ctl {
    int ready[MAX_WAVES];     /* chunks produced, per unit */
    int consumed;             /* chunks consumed by the serial wave */
    int abort_flag;
    int pad_[2];
};
struct GeomLean : GeomNarrow {                        /* ring geometry seen by costas_wave / flush_records */
    static constexpr int DSTRIDE = 194;               /* float2 slots per row: 1552 bytes */
    static constexpr int ZSTRIDE = 388;               /* floats per row */
};
constexpr int ROW_BYTES = 1552, Z_OFFSET_BYTES = 1024;
static_assert(GeomLean::DSTRIDE * 8 == ROW_BYTES && GeomLean::ZSTRIDE * 4 == ROW_BYTES &&
              Z_OFFSET_BYTES == DR * GeomNarrow::S * 8 && Z_OFFSET_BYTES + DR * GeomNarrow::S * 4 <= ROW_BYTES &&
              ROW_BYTES % 16 == 0 && (ROW_BYTES / 4) % 64 == 4, "ring rows: symbols, records, bank spread");
static_assert(sizeof(Ctl) % 16 == 0 && offsetof(Ctl, ready) == 0 && offsetof(Ctl, consumed) == 64 &&
              offsetof(Ctl, abort_flag) == 68, "fir_lean_asm.h addresses the counters by these offsets");
} // namespace lean

} // namespace qpsk
#endif
