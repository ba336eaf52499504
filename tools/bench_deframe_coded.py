"""Time qpsk_deframer_push_coded at 4096 streams x 2048 symbols next to the uncoded push, qpsk_viterbi_batch and one
qpsk_streams_rx_pcm block of the same shape (fs 19200, rs 2400, 16384-sample blocks), in one process, with events as bench.py times
its steps; rounds interleaved, medians.  64-dibit word (min_score 56), 64-byte packets: a coded packet is 64 + 534 symbols.

  block          qpsk_streams_rx_pcm, costas_frame[] requested
  uncoded        qpsk_deframer_push on that block's d_costas (a second context: a context holds one deframer); no packets
  empty_gain     qpsk_deframer_push_coded on the same d_costas with d_gain: the hunt, and a decode launch whose waves all retire
  empty_nogain   the same with d_gain NULL: soft_sums_kernel in front
  one            coded push, one packet per stream and push (synthetic d_costas, the packet inside the row), d_gain given
  one_nogain     the same with d_gain NULL
  one_hunt       the same with d_bytes, d_crc_ok, d_info NULL: no decode launch, the hunt and the soft rows alone
  viterbi        qpsk_viterbi_batch on 4096 contiguous rows of 534 steps (the same packets' soft rows from qpsk_soft_batch)
  eight          coded push completing 8 packets per stream: rows of 8 x 598 + 64 symbols (longer than a block), d_gain given

Every coded leg starts from a freshly reset deframer.  Prints one JSON line and writes the record to --out (profiles/deframe_coded.txt).
Usage: python tools/bench_deframe_coded.py [--streams 4096] [--steps 30] [--rounds 5] [--only LEG]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deframe_coded.txt"))
    ap.add_argument("--only", default=None, help="time one leg alone (for a kernel trace of its own); writes no record")
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    S, fs, rs, L = args.streams, 19200.0, 2400.0, 16384
    m = qpsk_amd.Modem(fs=fs, rs=rs, frame_size=L)
    mu = qpsk_amd.Modem(fs=fs, rs=rs, frame_size=L)
    N = m.nsym
    m.streams_reset(S, 1500.0)
    g = torch.Generator(device=dev).manual_seed(1)
    pcm = (torch.randn((S, L), device=dev, generator=g) * 6000).to(torch.int16)
    sym = torch.empty((S, N), dtype=torch.uint8, device=dev)
    costas = torch.empty((S, N, 2), dtype=torch.float32, device=dev)
    freq = torch.empty(S, dtype=torch.float32, device=dev)
    phase = torch.empty(S, dtype=torch.float32, device=dev)
    index = torch.empty(S, dtype=torch.int32, device=dev)
    nsync, nbytes, M = 64, 64, 8
    Nc = 8 * (nbytes + 2) + 6
    rng = np.random.default_rng(3)
    word = rng.integers(0, 4, nsync).astype(np.uint8)
    m.deframer_reset_coded(S, word, nbytes, 56, max_packets=M)
    mu.deframer_reset(S, word, nbytes, 56, max_packets=M)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731

    # the packets, built with the library: payload + CRC -> conv_encode -> scramble; one per stream
    payload = rng.integers(0, 256, (S, nbytes)).astype(np.uint8)
    crc = m.crc16(payload)
    packet = np.concatenate([payload, (crc >> 8).astype(np.uint8)[:, None], (crc & 255).astype(np.uint8)[:, None]], axis=1)
    body = m.scramble(m.conv_encode(packet, 8 * (nbytes + 2), tail=True)).cpu().numpy()
    pkt = np.concatenate([np.tile(word, (S, 1)), body], axis=1)          # (S, 598)

    def plant(nsym, offsets):
        d = np.zeros((S, nsym), np.uint8)      # a constant filler: no window of it, or of it and a packet's edge, reaches min_score
        for s in range(S):
            for o in offsets(s):
                d[s, o:o + pkt.shape[1]] = pkt[s]
        z = np.stack([1.0 - 2.0 * (d & 1), 1.0 - 2.0 * (d >> 1)], axis=-1) * 0.7 + 0.2 * rng.standard_normal((S, nsym, 2))
        return torch.from_numpy(z.astype(np.float32)).to(dev)

    first = rng.integers(0, N - pkt.shape[1], S)
    z_one = plant(N, lambda s: [int(first[s])])
    N8 = 8 * pkt.shape[1] + 64
    z_eight = plant(N8, lambda s: [int(first[s]) % 64 + k * pkt.shape[1] for k in range(8)])
    gain = torch.full((S,), 90.0, dtype=torch.float32, device=dev)
    count = torch.empty(S, dtype=torch.int32, device=dev)
    out = torch.empty((S, M, nbytes + 2), dtype=torch.uint8, device=dev)
    pos = torch.empty((S, M), dtype=torch.int64, device=dev)
    rot = torch.empty((S, M), dtype=torch.int32, device=dev)
    score = torch.empty((S, M), dtype=torch.int32, device=dev)
    ok = torch.empty((S, M), dtype=torch.uint8, device=dev)
    info = torch.empty((S, M, 4), dtype=torch.int32, device=dev)

    def block():
        m._check(m.L.qpsk_streams_rx_pcm(m.h, P(pcm), P(sym), P(freq), P(phase), P(costas), P(index)))

    block()
    m.sync()

    def uncoded():
        mu._check(mu.L.qpsk_deframer_push(mu.h, P(costas), None, N, P(count), P(out), P(pos), P(rot), P(score), P(ok)))

    def coded(z, gn, decode=True):
        def fn():
            m._check(m.L.qpsk_deframer_push_coded(m.h, P(z), z.shape[1], P(gn), P(count), P(out) if decode else None, P(pos), P(rot), P(score),
                                                  P(ok) if decode else None, P(info) if decode else None))
        return fn

    soft = m.soft(z_one, gain=gain, lag=torch.from_numpy(first.astype(np.int32)).to(dev), rot=torch.zeros(S, dtype=torch.int32, device=dev),
                  first=nsync, nout=Nc)["soft"]
    flip = m.scramble(np.zeros((1, Nc), np.uint8))[0].contiguous()
    bits = torch.empty((S, (Nc + 7) // 8), dtype=torch.uint8, device=dev)
    vinfo = torch.empty((S, 4), dtype=torch.int32, device=dev)

    def viterbi():
        m._check(m.L.qpsk_viterbi_batch(m.h, P(soft), 0, S, Nc, P(flip), 0, P(bits), P(vinfo)))

    # what is timed is what is meant: one packet per stream, all good, and the batch decoder returns the same bytes
    coded(z_one, gain)()
    kernels = m.last_kernel()
    viterbi()
    m.sync()
    assert (count.cpu().numpy() == 1).all() and ok.cpu().numpy()[:, 0].all()
    assert np.array_equal(out.cpu().numpy()[:, 0], bits.cpu().numpy()[:, :nbytes + 2]) and np.array_equal(out.cpu().numpy()[:, 0], packet)
    coded(z_eight, gain)()
    m.sync()
    assert (count.cpu().numpy() == 8).all() and ok.cpu().numpy().all()
    coded(costas, gain)()
    m.sync()
    found_in_noise = int(count.cpu().numpy().sum())

    def fresh():
        """every coded leg starts from a freshly reset deframer, not from the state the leg before it left"""
        m.deframer_reset_coded(S, word, nbytes, 56, max_packets=M)

    def timed(fn, sync, steps, before=None, expect=None):
        if before:
            before()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        sync()
        if expect is not None:      # the last timed push still found what the leg is about
            assert (count.cpu().numpy() == expect).all(), expect
        return e0.elapsed_time(e1) / steps

    legs = (("block", block, m.sync, None, None), ("uncoded", uncoded, mu.sync, None, None),
            ("empty_gain", coded(costas, gain), m.sync, fresh, None), ("empty_nogain", coded(costas, None), m.sync, fresh, None),
            ("one", coded(z_one, gain), m.sync, fresh, 1), ("one_nogain", coded(z_one, None), m.sync, fresh, 1),
            ("one_hunt", coded(z_one, gain, decode=False), m.sync, fresh, 1), ("viterbi", viterbi, m.sync, None, None),
            ("eight", coded(z_eight, gain), m.sync, fresh, 8))
    if args.only:      # one leg alone, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/... --only one)
        legs = tuple(leg for leg in legs if leg[0] == args.only)
        assert legs, "unknown leg %s" % args.only
    res = {leg[0]: [] for leg in legs}
    for _ in range(args.rounds):
        for k, fn, sync, before, expect in legs:
            res[k].append(timed(fn, sync, args.steps, before, expect))
    med = {k: float(np.median(v)) for k, v in res.items()}
    rec = {"streams": S, "nsym": N, "nsym_eight": N8, "nsync": nsync, "nbytes": nbytes, "nsteps": Nc, "kernels": kernels,
           "packets_found_in_noise": found_in_noise, "ms_per_call": med, "all": res}
    if not args.only:
        rec.update({"empty_gain_over_uncoded": med["empty_gain"] / med["uncoded"], "empty_nogain_over_uncoded": med["empty_nogain"] / med["uncoded"],
                    "decode_in_push_over_viterbi_batch": (med["one"] - med["one_hunt"]) / med["viterbi"],
                    "one_over_block": med["one"] / med["block"], "one_nogain_over_block": med["one_nogain"] / med["block"]})
    line = json.dumps(rec)
    print(line)
    if not args.only:
        with open(args.out, "w") as f:
            f.write("qpsk_deframer_push_coded, %d streams x %d symbols (tools/bench_deframe_coded.py: one process, events, %d interleaved rounds of %d "
                    "calls, medians in ms per call)\n\n" % (S, N, args.rounds, args.steps))
            for k, *_ in legs:
                f.write("  %-13s %9.4f   rounds %s\n" % (k, med[k], " ".join("%.4f" % v for v in res[k])))
            f.write("\n" + line + "\n")

if __name__ == "__main__":
    main()
