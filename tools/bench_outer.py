"""Time the outer link of a continuous stream at 4096 streams x 2048 bits per push -- what one qpsk_viterbi_stream_push of 2048 steps at
(depth, window) = (128, 256) emits -- next to that push itself and to qpsk_rs_decode_batch on the words the link yields: existing code,
the yardsticks.  One process, events as bench.py times its steps, rounds interleaved, medians.

The bit stream is RS (204, 188) codewords with the sync byte 0x47 as byte 0 of the data, interleaved (I = 12) or not (I = 1).  204 and 256
bytes meet again after 13056 bytes = 64 words = 51 pushes, and the interleaver is run cyclically over the 64 words, so the 51 pushes are
repeated for ever without a seam: the link stays in steady lock at every bit phase a push can begin with.  The legs:
  outer_204_12, outer_204_1   qpsk_outer_push in steady lock (lock 2, drop 3, POLARITY), all five outputs
  outer_hunt                  the same push on random bytes with lock = 16, which never locks: every bit position a candidate
  interleave_204_12           qpsk_outer_interleave_batch on the 64 words of a cycle (51 pushes' bytes in one call)
  viterbi_stream_push         the push that produces such bits, in steady state at (128, 256)
  rs_decode_204_188           qpsk_rs_decode_batch on one clean word per stream (a push yields 256 / 204 = 1.25 of them)

Prints one JSON line and writes the record to --out (profiles/outer.txt).
Usage: python tools/bench_outer.py [--streams 4096] [--steps 30] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, K, SYNC = 204, 188, 0x47
PUSH_BYTES, CYCLE_WORDS, CYCLE_PUSHES = 256, 64, 51


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    S, nbits = args.streams, 8 * PUSH_BYTES
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)      # noqa: E731
    m0 = qpsk_amd.Modem()
    g = torch.Generator(device=dev).manual_seed(1)
    data = torch.randint(0, 256, (S * CYCLE_WORDS, K), dtype=torch.uint8, device=dev, generator=g)
    data[:, 0] = SYNC
    sent = m0.rs_encode(data, N - K).contiguous().reshape(S, CYCLE_WORDS, N)
    cyc = {1: sent, 12: m0.outer_interleave(sent, 12, sent[:, -11:].contiguous())[0]}      # the history of a cycle is its own end
    noise = torch.randint(0, 256, (S, CYCLE_WORDS * N), dtype=torch.uint8, device=dev, generator=g)
    pitch = CYCLE_WORDS * N

    legs, checks = [], {}

    def outer_leg(name, src, branches, lock):
        m = qpsk_amd.Modem()
        m.outer_reset(S, N, branches, SYNC, lock, 3)
        mw = m.outer_max_words(nbits)
        out = dict(count=torch.empty((S,), dtype=torch.int32, device=dev), words=torch.empty((S, mw, N), dtype=torch.uint8, device=dev),
                   pos=torch.empty((S, mw), dtype=torch.int64, device=dev), flags=torch.empty((S, mw), dtype=torch.uint8, device=dev),
                   info=torch.empty((S, 4), dtype=torch.int32, device=dev))
        k = [0]

        def fn():
            m._check(m.L.qpsk_outer_push(m.h, P(src, PUSH_BYTES * (k[0] % CYCLE_PUSHES)), pitch, nbits, mw, P(out["count"]), P(out["words"]), 0,
                                         P(out["pos"]), P(out["flags"]), P(out["info"])))
            k[0] += 1
        total = 0
        for _ in range(CYCLE_PUSHES):      # one cycle: the lock, the branches filled
            fn()
            total += int(out["count"].sum())
        m.sync()
        checks[name] = dict(words_in_first_cycle=total, locked=int(out["info"][:, 0].sum()), lost=int(out["info"][:, 3].sum()))
        legs.append((name, fn, m.sync))
        return m, out

    m12, out12 = outer_leg("outer_204_12", cyc[12].reshape(S, -1), 12, 2)
    # what is timed is what is meant: in steady lock every emitted word is a word that was sent, with a clean flag
    assert checks["outer_204_12"]["locked"] == S and (out12["flags"][:, 0] == 0).all()
    w = out12["words"][:, 0].cpu().numpy()
    at = ((out12["pos"][:, 0].cpu().numpy() // (8 * N)) - 11) % CYCLE_WORDS
    assert (w == sent.cpu().numpy()[np.arange(S), at]).all(), "the deinterleaved words are not the sent ones"
    m1, out1 = outer_leg("outer_204_1", cyc[1].reshape(S, -1), 1, 2)
    assert checks["outer_204_1"]["locked"] == S
    mh, outh = outer_leg("outer_hunt", noise, 12, 16)
    assert checks["outer_hunt"]["locked"] == 0 and checks["outer_hunt"]["words_in_first_cycle"] == 0

    il_out = torch.empty_like(sent)
    il_hist = sent[:, -11:].contiguous()

    def interleave():
        m0._check(m0.L.qpsk_outer_interleave_batch(m0.h, P(sent), S, CYCLE_WORDS, N, 12, P(il_hist), None, P(il_out)))
    legs.append(("interleave_204_12", interleave, m0.sync))

    # the yardsticks: the stream decoder's push that emits 2048 bits, and the RS decode of a word per stream
    mv = qpsk_amd.Modem()
    mv.viterbi_stream_reset(S, 128, 256)
    dibits, _ = mv.conv_encode_stream(cyc[12].reshape(S, -1)[:, :PUSH_BYTES].contiguous(), nbits)
    ideal = torch.where((dibits[..., None] >> torch.arange(2, device=dev)) & 1 != 0, -64.0, 64.0)
    soft = (ideal + 24.0 * torch.randn(ideal.shape, device=dev, generator=g)).round().clamp(-127, 127).to(torch.int8).contiguous()
    vbits = torch.empty((S, PUSH_BYTES), dtype=torch.uint8, device=dev)
    vinfo = torch.empty((S, 4), dtype=torch.int32, device=dev)
    nb = C.c_int(0)

    def vpush():
        mv._check(mv.L.qpsk_viterbi_stream_push(mv.h, P(soft), 0, nbits, P(vbits), PUSH_BYTES, P(vinfo), C.byref(nb)))
    for _ in range(3):
        vpush()
    mv.sync()
    assert nb.value == nbits      # steady state: a push emits as many bits as it takes steps
    legs.append(("viterbi_stream_push", vpush, mv.sync))

    mr = qpsk_amd.Modem()
    rs_in = sent[:, 0].contiguous()
    rs_out = torch.empty_like(rs_in)
    rs_info = torch.empty((S, 4), dtype=torch.int32, device=dev)

    def rs():
        mr._check(mr.L.qpsk_rs_decode_batch(mr.h, P(rs_in), 0, S, N, N - K, None, P(rs_out), 0, P(rs_info)))
    legs.append(("rs_decode_204_188", rs, mr.sync))

    def timed(fn, sync):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        sync()
        return e0.elapsed_time(e1) / args.steps

    res = {k: [] for k, _, _ in legs}
    for _ in range(args.rounds):
        for k, fn, sync in legs:
            res[k].append(timed(fn, sync))
    med = {k: float(np.median(v)) for k, v in res.items()}
    ratio = {k: med[k] / med["viterbi_stream_push"] for k in med}
    rec = {"streams": S, "bits_per_push": nbits, "kernels": {"push": m12.last_kernel(), "interleave": m0.last_kernel(), "stream": mv.last_kernel()},
           "ms_per_call": med, "over_viterbi_stream_push": ratio, "interleave_ms_per_push_equivalent": med["interleave_204_12"] / CYCLE_PUSHES,
           "checks": checks, "all": res}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("the outer link at %d streams x %d bits per push, words of (204, 188) (tools/bench_outer.py: one process, events, %d interleaved "
                "rounds of %d calls, medians in ms per call)\n\n" % (S, nbits, args.rounds, args.steps))
        for k, _, _ in legs:
            f.write("  %-20s %9.4f   x %6.3f of viterbi_stream_push   rounds %s\n" % (k, med[k], ratio[k], " ".join("%.4f" % v for v in res[k])))
        f.write("\n  interleave_204_12 covers the bytes of %d pushes in one call: %.5f ms per push's bytes\n" % (CYCLE_PUSHES, med["interleave_204_12"] / CYCLE_PUSHES))
        f.write("  rs_decode_204_188 decodes one clean word per stream; a push yields 1.25\n")
        f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
