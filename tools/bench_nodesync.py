"""Time the node sync at 4096 links x 2048 dibits per push -- the rows one qpsk_viterbi_stream_push of 2048 steps at rate 1/2 takes -- next to
that push itself at (depth, window) = (128, 256) on the node sync's output and to a device-to-device copy of the same 16 MB: existing code
and the memory system, the yardsticks.  One process, events as bench.py times its steps, rounds interleaved, medians.

The node sync runs as it does in a loop: nrot = 4 x nshift = 8 candidates mixed over the links (every quarter turn, every delay 0..7, so the
source rows sit at every alignment the delay can give them), d_vinfo given (the decoder's d_info of its last push, on the device) and
d_info written.  The monitor's threshold is 65535 / 1, which no count exceeds: every link stays on its candidate, so every call moves the same
bytes.  The legs:
  nodesync_push          qpsk_nodesync_push, tick and transform
  nodesync_push_r0h0     the same with every link on candidate 0: the aligned-source case
  viterbi_stream_push    qpsk_viterbi_stream_push in steady state on the node sync's rows
  copy_d2d               torch's copy_ of the same int8 tensor to another

Prints one JSON line and writes the record to --out (profiles/nodesync.txt).
Usage: python tools/bench_nodesync.py [--links 4096] [--steps 30] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NTX, NROT, NSHIFT = 2048, 4, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nodesync.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    S = args.links
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    g = torch.Generator(device=dev).manual_seed(1)

    # rows a decoder is meant for: coded random bits at +-64 with Gaussian noise of sigma 24
    mv = qpsk_amd.Modem()
    mv.viterbi_stream_reset(S, 128, 256)
    data = torch.randint(0, 256, (S, NTX // 8), dtype=torch.uint8, device=dev, generator=g)
    dibits, _ = mv.conv_encode_stream(data, NTX)
    ideal = torch.where((dibits[..., None] >> torch.arange(2, device=dev)) & 1 != 0, -64.0, 64.0)
    soft = (ideal + 24.0 * torch.randn(ideal.shape, device=dev, generator=g)).round().clamp(-127, 127).to(torch.int8).contiguous()
    out = torch.empty_like(soft)
    copy = torch.empty_like(soft)
    vbits = torch.empty((S, NTX // 8), dtype=torch.uint8, device=dev)
    vinfo = torch.zeros((S, 4), dtype=torch.int32, device=dev)
    nb = C.c_int(0)

    def vpush():
        mv._check(mv.L.qpsk_viterbi_stream_push(mv.h, P(out), 0, NTX, P(vbits), NTX // 8, P(vinfo), C.byref(nb)))

    legs, checks = [], {}

    def nodesync_leg(name, cand):
        m = qpsk_amd.Modem()
        m.nodesync_reset(S, NROT, NSHIFT, span=4096, settle=0, threshold=(65535, 1), drop=2)
        m.nodesync_set(cand)
        info = torch.empty((S, 8), dtype=torch.int32, device=dev)

        def fn():
            m._check(m.L.qpsk_nodesync_push(m.h, P(soft), 0, NTX, P(vinfo), P(out), 0, P(info)))
        fn()
        m.sync()
        h = info.cpu().numpy()
        # what is timed is what is meant: no link has left its candidate
        assert (h[:, 0] + NROT * h[:, 1] == cand.cpu().numpy()).all() and not h[:, 3].any()
        checks[name] = dict(candidates=int(np.unique(h[:, 0] + NROT * h[:, 1]).size), switches=int(h[:, 3].sum()))
        legs.append((name, fn, m.sync))
        return m

    mixed = (torch.arange(S, dtype=torch.int32, device=dev) * 7) % (NROT * NSHIFT)
    mn = nodesync_leg("nodesync_push_r0h0", torch.zeros(S, dtype=torch.int32, device=dev))
    assert torch.equal(out, soft)                                  # candidate 0 on rows without -128: the copy
    mm = nodesync_leg("nodesync_push", mixed)
    for _ in range(3):
        vpush()
    mv.sync()
    assert nb.value == NTX      # steady state: a push emits as many bits as it takes steps
    legs.append(("viterbi_stream_push", vpush, mv.sync))
    legs.append(("copy_d2d", lambda: copy.copy_(soft), torch.cuda.synchronize))

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
    ratio = {k: med[k] / med["copy_d2d"] for k in med}
    nbytes = soft.numel()
    rec = {"links": S, "dibits_per_push": NTX, "bytes_each_way": nbytes, "kernels": {"push": mm.last_kernel(), "stream": mv.last_kernel()},
           "ms_per_call": med, "over_copy_d2d": ratio, "gb_per_s_read_plus_written": {k: 2 * nbytes / med[k] / 1e6 for k in med if k != "viterbi_stream_push"},
           "checks": checks, "all": res}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("the node sync at %d links x %d dibits per push, %d candidates mixed over the links, d_vinfo given (tools/bench_nodesync.py: one "
                "process, events, %d interleaved rounds of %d calls, medians in ms per call)\n\n" % (S, NTX, NROT * NSHIFT, args.rounds, args.steps))
        for k, _, _ in legs:
            f.write("  %-20s %9.4f   x %6.3f of copy_d2d   rounds %s\n" % (k, med[k], ratio[k], " ".join("%.4f" % v for v in res[k])))
        f.write("\n  %d bytes are read and as many written per call by the node sync and by the copy\n" % nbytes)
        f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
