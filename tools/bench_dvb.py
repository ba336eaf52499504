"""Time DVB-S transport framing: qpsk_outer_push under group sync next to the ungrouped link, and qpsk_dispersal_batch next to a
device-to-device copy of the same bytes and to the qpsk_rs_decode_batch that feeds it.  One process, events as bench.py times its steps,
rounds interleaved, medians.  The shape is tools/bench_outer.py's: 4096 streams x 2048 bits per push, words of (204, 188) behind I = 12;
64 words are 51 pushes and 8 groups of 8, so the 51 pushes repeat for ever without a seam and the link stays in steady lock.  The legs:
  group_lock, plain_lock   qpsk_outer_push in steady lock at lock 8, drop 3, POLARITY: group 8 on words whose every eighth sync byte is
                           inverted / no group on words that all begin with 0x47.  The same lock, so the same ring and look-ahead
  group_hunt, plain_hunt   the same two links on random bytes, which never lock: every bit position a candidate
  dispersal_8192           qpsk_dispersal_batch on 4096 x 2 rows of 188 at pitch 204 with d_flags (what one push's words are), out of place
  dispersal_2e20           the same on 2^20 rows
  copy_8192, copy_2e20     a device-to-device copy (torch's copy_ of a contiguous uint8 tensor: hipMemcpyAsync) of rows x 188 bytes
  rs_decode_8192           qpsk_rs_decode_batch (204, 188) on 4096 x 2 clean words: the stage in front of the dispersal

Prints one JSON line and writes the record to --out (profiles/dvb.txt).
Usage: python tools/bench_dvb.py [--streams 4096] [--steps 30] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, K, SYNC, G, LOCK = 204, 188, 0x47, 8, 8
PUSH_BYTES, CYCLE_WORDS, CYCLE_PUSHES = 256, 64, 51


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--big", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvb.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    S, nbits = args.streams, 8 * PUSH_BYTES
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)      # noqa: E731
    m0 = qpsk_amd.Modem()
    g = torch.Generator(device=dev).manual_seed(1)
    data = torch.randint(0, 256, (S, CYCLE_WORDS, K), dtype=torch.uint8, device=dev, generator=g)
    cyc = {}
    for name in ("plain", "group"):
        data[:, :, 0] = SYNC
        if name == "group":
            data[:, ::G, 0] = SYNC ^ 0xFF
        sent = m0.rs_encode(data.reshape(-1, K), N - K).contiguous().reshape(S, CYCLE_WORDS, N)
        cyc[name] = (sent, m0.outer_interleave(sent, 12, sent[:, -11:].contiguous())[0].reshape(S, -1))      # the history of a cycle is its own end
    noise = torch.randint(0, 256, (S, CYCLE_WORDS * N), dtype=torch.uint8, device=dev, generator=g)
    pitch = CYCLE_WORDS * N

    legs, checks = [], {}

    def outer_leg(name, src, group):
        m = qpsk_amd.Modem()
        m.outer_reset(S, N, 12, SYNC, LOCK, 3, group=group)
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

    mg, outg = outer_leg("group_lock", cyc["group"][1], G)
    # what is timed is what is meant: in steady lock every emitted word is the word that was sent, its flag clean and its group index right
    assert checks["group_lock"]["locked"] == S
    at = ((outg["pos"][:, 0].cpu().numpy() // (8 * N)) - 11) % CYCLE_WORDS
    assert (outg["words"][:, 0].cpu().numpy() == cyc["group"][0].cpu().numpy()[np.arange(S), at]).all(), "the deinterleaved words are not the sent ones"
    assert (outg["flags"][:, 0].cpu().numpy() == (at % G) << 4).all()
    outer_leg("plain_lock", cyc["plain"][1], 0)
    assert checks["plain_lock"]["locked"] == S
    outer_leg("group_hunt", noise, G)
    outer_leg("plain_hunt", noise, 0)
    for name in ("group_hunt", "plain_hunt"):
        assert checks[name]["locked"] == 0 and checks[name]["words_in_first_cycle"] == 0

    md = qpsk_amd.Modem()

    def dispersal_legs(tag, R):
        rows = torch.randint(0, 256, (R, N), dtype=torch.uint8, device=dev, generator=g)
        out = torch.empty_like(rows)
        flags = (torch.arange(R, device=dev) % G << 4).to(torch.uint8)
        tight, tight_out = torch.empty((R * K,), dtype=torch.uint8, device=dev), torch.empty((R * K,), dtype=torch.uint8, device=dev)

        def disp():
            md._check(md.L.qpsk_dispersal_batch(md.h, P(rows), N, R, K, G, 1, P(flags), 0, P(out), N))

        def copy():
            tight_out.copy_(tight)
        disp()
        md.sync()
        want = np.frombuffer(qpsk_amd.dispersal_sequence(K, G, True), np.uint8)
        assert (out[1, 1:K].cpu().numpy() == rows[1, 1:K].cpu().numpy() ^ want[K:2 * K - 1]).all() and int(out[0, 0]) == int(rows[0, 0]) ^ 0xFF
        legs.append(("dispersal_" + tag, disp, md.sync))
        legs.append(("copy_" + tag, copy, torch.cuda.synchronize))
        return R * K

    nbytes = {"8192": dispersal_legs("8192", 2 * S), "2e20": dispersal_legs("2e20", args.big)}

    mr = qpsk_amd.Modem()
    rs_in = cyc["group"][0][:, :2].contiguous().reshape(-1, N)
    rs_out = torch.empty_like(rs_in)
    rs_info = torch.empty((rs_in.shape[0], 4), dtype=torch.int32, device=dev)

    def rs():
        mr._check(mr.L.qpsk_rs_decode_batch(mr.h, P(rs_in), 0, rs_in.shape[0], N, N - K, None, P(rs_out), 0, P(rs_info)))
    legs.append(("rs_decode_8192", rs, mr.sync))

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
    spread = {k: (max(v) - min(v)) / med[k] for k, v in res.items()}
    ratios = {"group_lock_over_plain_lock": med["group_lock"] / med["plain_lock"], "group_hunt_over_plain_hunt": med["group_hunt"] / med["plain_hunt"],
              "copy_over_dispersal_8192": med["copy_8192"] / med["dispersal_8192"], "copy_over_dispersal_2e20": med["copy_2e20"] / med["dispersal_2e20"],
              "dispersal_8192_over_rs_decode_8192": med["dispersal_8192"] / med["rs_decode_8192"]}
    gbs = {k: 2 * nbytes[k.split("_")[1]] / med[k] / 1e6 for k in med if k.startswith(("dispersal_", "copy_"))}      # read + written
    rec = {"streams": S, "bits_per_push": nbits, "big_rows": args.big, "kernels": {"push": mg.last_kernel(), "dispersal": md.last_kernel()},
           "ms_per_call": med, "round_spread_over_median": spread, "ratios": ratios, "GB_per_s_read_plus_written": gbs, "checks": checks, "all": res}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("DVB-S transport framing at %d streams x %d bits per push, words of (204, 188), I = 12, G = 8, lock 8 (tools/bench_dvb.py: one "
                "process, events, %d interleaved rounds of %d calls, medians in ms per call)\n\n" % (S, nbits, args.rounds, args.steps))
        for k, _, _ in legs:
            f.write("  %-16s %9.4f   spread %5.1f %%   rounds %s%s\n" % (k, med[k], 100 * spread[k], " ".join("%.4f" % v for v in res[k]),
                                                                       "   %.0f GB/s read + written" % gbs[k] if k in gbs else ""))
        f.write("\n")
        for k, v in ratios.items():
            f.write("  %-36s %.3f\n" % (k, v))
        f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
