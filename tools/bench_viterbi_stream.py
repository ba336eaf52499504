"""Time a steady-state qpsk_viterbi_stream_push at 4096 streams x 2048 steps, rate 1/2, for (depth, window) = (128, 256), (128, 1024) and
(64, 64), next to qpsk_viterbi_batch on 4096 rows x 2048 steps on its scratch route -- existing code, the yardstick -- in one process, with
events as bench.py times its steps; rounds interleaved, medians.  The input is a coded random stream (qpsk_conv_encode_stream_batch) at +-64
with Gaussian noise; every decoder has seen more than depth + window steps before it is timed, so every timed push makes
2048 / window decisions of (depth + window) trace-back steps each.

A decision walks (depth + window) / window trace-back steps per trellis step: 1.5, 1.125 and 2 for the three legs.  The record also gives the
least-squares split  ms = forward + walk * (depth + window) / window  over the three legs: what the forward pass and one trace-back step
per step cost, without a profiling build.

Prints one JSON line and writes the record to --out (profiles/viterbi_stream.txt).
Usage: python tools/bench_viterbi_stream.py [--streams 4096] [--steps 30] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ((128, 256), (128, 1024), (64, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--nsteps", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi_stream.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    S, n = args.streams, args.nsteps
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    mb = qpsk_amd.Modem()
    g = torch.Generator(device=dev).manual_seed(1)
    data = torch.randint(0, 256, (S, n // 8), dtype=torch.uint8, device=dev, generator=g)
    dibits, _ = mb.conv_encode_stream(data, n)
    ideal = torch.where((dibits[..., None] >> torch.arange(2, device=dev)) & 1 != 0, -64.0, 64.0)
    soft = (ideal + 24.0 * torch.randn(ideal.shape, device=dev, generator=g)).round().clamp(-127, 127).to(torch.int8).contiguous()
    bits = torch.empty((S, n // 8), dtype=torch.uint8, device=dev)
    info = torch.empty((S, 4), dtype=torch.int32, device=dev)
    nb = C.c_int(0)

    mb.tune(viterbi_lds=0)

    def batch():
        mb._check(mb.L.qpsk_viterbi_batch(mb.h, P(soft), 0, S, n, None, 2, P(bits), P(info)))

    batch()
    batch_kernel = mb.last_kernel()
    mb.sync()
    assert batch_kernel == "viterbi_kernel", batch_kernel
    want = bits.cpu().numpy().copy()
    assert np.array_equal(want[:, :-8], data.cpu().numpy()[:, :-8]), "the noise level is meant to decode clean (an open end's last bits apart)"

    streams = {}
    for depth, window in LEGS:
        m = qpsk_amd.Modem()
        m.viterbi_stream_reset(S, depth, window)

        def fn(m=m):
            m._check(m.L.qpsk_viterbi_stream_push(m.h, P(soft), 0, n, P(bits), n // 8, P(info), C.byref(nb)))
        # what is timed is what is meant: the first push and a flush give the batch decoder's bits; then into the steady state
        first = m.viterbi_stream(soft)
        rest = m.viterbi_stream_flush()
        m.sync()
        got = np.concatenate([first["bits"].cpu().numpy(), rest["bits"].cpu().numpy()], axis=1)
        assert first["nbits"] + rest["nbits"] == n and np.array_equal(got[:, :-8], want[:, :-8]), (depth, window)
        for _ in range(-(-(depth + window) // n) + 1):
            fn()
        m.sync()
        assert nb.value == n, (depth, window, nb.value)      # steady state: a push emits as many bits as it takes steps
        streams["stream_%d_%d" % (depth, window)] = (fn, m)

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

    legs = [("viterbi_batch", batch, mb.sync)] + [(k, fn, m.sync) for k, (fn, m) in streams.items()]
    res = {k: [] for k, _, _ in legs}
    for _ in range(args.rounds):
        for k, fn, sync in legs:
            res[k].append(timed(fn, sync))
    med = {k: float(np.median(v)) for k, v in res.items()}
    ratio = {k: med[k] / med["viterbi_batch"] for k in streams}
    # ms = forward + walk * (D + W) / W over the three legs
    A = np.array([[1.0, (d + w) / w] for d, w in LEGS])
    y = np.array([med["stream_%d_%d" % dw] for dw in LEGS])
    (forward, walk), *_ = np.linalg.lstsq(A, y, rcond=None)
    rec = {"streams": S, "nsteps": n, "kernels": {"batch": batch_kernel, "stream": streams["stream_128_256"][1].last_kernel()},
           "ms_per_call": med, "over_viterbi_batch": ratio, "fit_ms": {"forward": float(forward), "walk_per_unit": float(walk)}, "all": res}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("qpsk_viterbi_stream_push in steady state, %d streams x %d steps per push, rate 1/2 (tools/bench_viterbi_stream.py: one process, "
                "events, %d interleaved rounds of %d calls, medians in ms per call)\n\n" % (S, n, args.rounds, args.steps))
        for k, _, _ in legs:
            f.write("  %-16s %9.4f   x %5.2f of viterbi_batch   rounds %s\n" % (k, med[k], med[k] / med["viterbi_batch"],
                                                                               " ".join("%.4f" % v for v in res[k])))
        f.write("\n  fit over the three stream legs, ms = forward + walk * (depth + window) / window:  forward %.4f  walk %.4f\n" % (forward, walk))
        f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
