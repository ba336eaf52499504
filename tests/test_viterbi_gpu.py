"""qpsk_conv_encode_batch / qpsk_viterbi_batch / Modem.conv_encode / Modem.viterbi on the GPU: decoded bits and all four info words bit for
bit against test_viterbi_cpu.viterbi_ref (the definition of include/qpsk_hip.h restated in numpy) on both routes (decision words in LDS,
in the scratch buffer), the encoder against conv_encode_ref, the whole coded link of the CPU test on the device, and the error contract."""
import ctypes as C

import numpy as np
import pytest

from test_rx_data_cpu import dibits_to_bytes
from test_soft_cpu import soft_ref
from test_viterbi_cpu import LINK, OPEN_END, OPEN_START, coded_link, conv_encode_ref, crc_ok, link_verdicts, pack_bits, viterbi_ref

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG = -2
LDS_ROUTE, SCRATCH_ROUTE = "viterbi_lds_kernel", "viterbi_kernel"
LDS_MAX_STEPS = 8192                    # kernels.h, VITERBI_LDS_MAX_BYTES / 8: longer rows never take the LDS route
GUARD = 64                              # elements behind every output that must stay untouched
ALL_FLAGS = (0, OPEN_START, OPEN_END, OPEN_START | OPEN_END)


def modem(**kw):
    import qpsk_amd
    kw.setdefault("fs", 19200.0)
    kw.setdefault("rs", 2400.0)
    kw.setdefault("frame_size", 16384)
    return qpsk_amd.Modem(**kw)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run(m, soft, flip=None, flags=0, pitch=0, nsteps=None, want=("bits", "info"), route=None):
    """the raw call with guarded outputs; soft: numpy (R, n, 2) int8, or a device tensor of pitched rows (then nsteps is given)"""
    import torch
    q = soft if hasattr(soft, "data_ptr") else torch.from_numpy(np.ascontiguousarray(soft, np.int8)).cuda()
    R = q.shape[0]
    n = q.shape[1] if nsteps is None else nsteps
    nb = (n + 7) // 8
    f = None if flip is None else torch.from_numpy(np.ascontiguousarray(flip, np.uint8)).cuda()
    bufs = {}
    if "bits" in want:
        bufs["bits"] = torch.full((R * nb + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    if "info" in want:
        bufs["info"] = torch.full((R * 4 + GUARD,), 0x55555555, dtype=torch.int32, device="cuda")
    m.tune(viterbi_lds=route)
    m._check(m.L.qpsk_viterbi_batch(m.h, ptr(q), pitch, R, n, ptr(f), flags, ptr(bufs.get("bits")), ptr(bufs.get("info"))))
    kernel = m.last_kernel()
    torch.cuda.synchronize()
    out = {"kernel": kernel}
    for k, b in bufs.items():
        h = b.cpu().numpy()
        size = h.size - GUARD
        assert np.all(h[size:] == (0x55 if k == "bits" else 0x55555555)), "guard behind %s overwritten" % k
        out[k] = h[:size].reshape((R, nb) if k == "bits" else (R, 4))
    return out


def assert_equal(got, want, what=""):
    for k in ("info", "bits"):
        if k in got:
            bad = np.nonzero((got[k] != want[k]).any(axis=1))[0]
            assert np.array_equal(got[k], want[k]), (what, k, "rows", bad[:8], got[k][bad[:2]], want[k][bad[:2]])


def random_soft(R, n, seed, kind="full"):
    rng = np.random.default_rng(seed)
    if kind == "full":
        return rng.integers(-128, 128, (R, n, 2)).astype(np.int8)
    if kind == "ties":
        return rng.integers(-1, 2, (R, n, 2)).astype(np.int8)
    if kind == "saturated":
        return rng.choice(np.array([-127, 127], np.int8), (R, n, 2))
    raise ValueError(kind)


def noisy_codewords(R, nbits, seed, sigma=40.0):
    """coded random bits (tail on) at +-64 with Gaussian noise: rows a decoder is meant for -> (soft, bits)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (R, nbits), dtype=np.uint8)
    d = conv_encode_ref(pack_bits(bits), nbits)
    x = np.stack([np.where(d & 1, -64.0, 64.0), np.where(d & 2, -64.0, 64.0)], axis=-1) + sigma * rng.standard_normal(d.shape + (2,))
    return np.clip(np.rint(x), -127, 127).astype(np.int8), bits


# ------------------------------------------------------------------------------------------ 6. random rows, every shape, both routes
@pytest.mark.parametrize("n", [1, 5, 6, 7, 63, 64, 65, 511, 512, 513, 2054, 4102])
def test_random_rows_bit_for_bit_on_both_routes(n):
    m = modem()
    key = np.random.default_rng(n).integers(0, 4, n).astype(np.uint8)
    for R in (1, 3):
        soft = random_soft(R, n, 10 * n + R)
        soft[0, n // 2, 0] = -128                       # taken as -127
        for flags in ALL_FLAGS:
            for flip in (None, key):
                want = viterbi_ref(soft, flip=flip, flags=flags)
                for route, name in ((0, SCRATCH_ROUTE), (1, LDS_ROUTE), (None, LDS_ROUTE)):
                    got = run(m, soft, flip=flip, flags=flags, route=route)
                    assert got["kernel"] == name, (route, got["kernel"])
                    assert_equal(got, want, (R, flags, flip is None, route))
    m.sync()
    m.close()


@pytest.mark.parametrize("kind", ["saturated", "ties", "zeros", "minus128"])
def test_saturating_tying_and_empty_rows(kind):
    m = modem()
    for n in (70, 2054):
        if kind == "zeros":
            soft = np.zeros((3, n, 2), np.int8)
        elif kind == "minus128":
            soft = np.full((3, n, 2), -128, np.int8)
            soft[1, ::3] = 127
        else:
            soft = random_soft(3, n, n, kind)
        for flags in ALL_FLAGS:
            want = viterbi_ref(soft, flags=flags)
            for route in (0, 1):
                assert_equal(run(m, soft, flags=flags, route=route), want, (kind, n, flags, route))
    m.sync()
    m.close()


def test_the_longest_row_and_the_big_batch():
    m = modem()
    # 131072 steps: beyond the LDS route whatever the tuning says
    soft, bits = noisy_codewords(2, 131072 - 6, 3)
    soft[1] = random_soft(1, 131072, 4)[0]
    want = viterbi_ref(soft)
    assert np.array_equal(want["bits"][0][:len(bits[0]) // 8], pack_bits(bits[0])[:len(bits[0]) // 8])      # the restatement decodes it
    for route in (None, 1):
        got = run(m, soft, route=route)
        assert got["kernel"] == SCRATCH_ROUTE
        assert_equal(got, want, route)
    # 4096 rows of 2054 steps: more rows than the LDS holds at once -> the scratch route by the library's own choice; LDS when told to
    soft, _ = noisy_codewords(4096, 2048, 5, sigma=45.0)
    soft[::7] = random_soft(len(soft[::7]), 2054, 6)
    key = np.random.default_rng(9).integers(0, 4, 2054).astype(np.uint8)
    want = viterbi_ref(soft, flip=key, flags=OPEN_END)
    for route, name in ((None, SCRATCH_ROUTE), (1, LDS_ROUTE)):
        got = run(m, soft, flip=key, flags=OPEN_END, route=route)
        assert got["kernel"] == name
        assert_equal(got, want, route)
    m.sync()
    m.close()


def test_pitched_rows_and_each_output_alone():
    import torch
    m = modem()
    R, n, pitch = 5, 700, 731
    soft = random_soft(R, n, 12)
    buf = np.full((R, pitch, 2), 0x7F, np.int8)
    buf[:, :n] = soft
    bt = torch.from_numpy(buf).cuda()
    for flags in (0, OPEN_START | OPEN_END):
        want = viterbi_ref(soft, flags=flags)
        for route in (0, 1):
            assert_equal(run(m, bt, flags=flags, pitch=pitch, nsteps=n, route=route), want, (flags, route))
            for outs in (("bits",), ("info",)):
                assert_equal(run(m, soft, flags=flags, want=outs, route=route), want, (flags, route, outs))
    # an odd 2-byte boundary for the first row
    flat = torch.zeros(2 * R * n + 2, dtype=torch.int8, device="cuda")
    flat[2:] = torch.from_numpy(soft.reshape(-1)).cuda()
    view = flat[2:].view(R, n, 2)
    assert view.data_ptr() % 4 == 2
    assert_equal(run(m, view, nsteps=n), viterbi_ref(soft))
    m.sync()
    m.close()


def test_python_front_end_and_noisy_codewords_come_back():
    m = modem()
    soft, bits = noisy_codewords(64, 1024, 21)
    got = m.viterbi(soft)
    m.sync()
    out = got["bits"].cpu().numpy()
    assert np.array_equal(out, viterbi_ref(soft)["bits"])
    assert np.array_equal(np.unpackbits(out, axis=1, bitorder="little")[:, :1024], bits)      # 64 +- 40: every row decodes clean
    info = got["info"].cpu().numpy()
    assert not info[:, 1].any() and not info[:, 2].any() and info[:, 3].min() > 0
    m.close()


# ------------------------------------------------------------------------------------------ 7. the encoder
@pytest.mark.parametrize("nbits", [1, 7, 8, 9, 63, 64, 65, 1000, 1024, 131066])
def test_encoder_equals_the_restatement(nbits):
    import torch
    m = modem()
    R = 3 if nbits > 10000 else 17
    rng = np.random.default_rng(nbits)
    packed = rng.integers(0, 256, (R, (nbits + 7) // 8), dtype=np.uint8)        # the padding bits of the last byte are garbage on purpose
    for tail in (True, False):
        got = m.conv_encode(packed, nbits, tail=tail)
        assert m.last_kernel() == "conv_encode_kernel"
        m.sync()
        assert np.array_equal(got.cpu().numpy(), conv_encode_ref(packed, nbits, tail=tail)), (nbits, tail)
    # guarded raw call
    n = nbits + 6
    out = torch.full((R * n + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    pt = torch.from_numpy(packed).cuda()
    m._check(m.L.qpsk_conv_encode_batch(m.h, ptr(pt), R, nbits, 1, ptr(out)))
    m.sync()
    assert torch.all(out[R * n:] == 0x55)
    m.close()


# ------------------------------------------------------------------------------------------ 8. the whole coded link on the device
def test_coded_link_on_the_device_equals_the_cpu_test(oracle):
    """test_viterbi_cpu's link, with the library's own calls: conv_encode -> scramble (the transmitted body equals the CPU's) ...
    rx_batch_ext(costas) / rx_batch_data -> sync -> soft -> viterbi(flip = keystream) -> crc16: every stage bit for bit the CPU test's"""
    import torch
    k = LINK
    lk = coded_link(oracle)
    hard_fail, good, want, soft_cpu = link_verdicts(oracle, lk)
    nsteps, nbytes, F = lk["nsteps"], k["nbytes"], k["frames"]
    m = modem(timing_mode=1, fixed_index=126 % k["C"])
    # transmit side: payload + CRC -> coded -> scrambled, on the device
    crc = m.crc16(lk["payloads"])
    packets = np.concatenate([lk["payloads"], (crc >> 8).astype(np.uint8)[:, None], (crc & 0xFF).astype(np.uint8)[:, None]], axis=1)
    body = m.scramble(m.conv_encode(packets, 8 * (nbytes + 2)))
    m.sync()
    assert m.scramble(torch.zeros((1, nsteps), dtype=torch.uint8)).cpu().numpy()[0].tolist() == lk["key"].tolist()
    assert np.array_equal(body.cpu().numpy(), oracle_scrambled_bodies(oracle, packets))
    # receive side
    xt = torch.from_numpy(lk["x"]).cuda()
    idx = torch.full((F,), 126 % k["C"], dtype=torch.int32)
    rx = m.rx_batch_ext(xt, index=idx, want_costas=True)
    data = m.rx_batch_data(xt, index=idx)["data"]
    s = m.sync(data, lk["sync"], 0, 255, nsteps + 4 * (nbytes + 2))
    soft = m.soft(rx, skip=256, lag=s["lag"], rot=s["rot"], first=k["nsync"], nout=nsteps)
    dec = m.viterbi(soft, flip=lk["key"])
    m.sync()
    assert np.array_equal(rx["costas"].cpu().numpy().view(np.uint32), np.asarray(lk["costas"], np.float32).view(np.uint32))
    for name in ("lag", "rot", "out"):
        assert np.array_equal(s[name].cpu().numpy(), lk["s"][name]), name
    assert np.array_equal(soft["soft"].cpu().numpy(), soft_cpu)
    bits, info = dec["bits"].cpu().numpy(), dec["info"].cpu().numpy()
    assert np.array_equal(bits, want["bits"]) and np.array_equal(info, want["info"])
    out = np.ascontiguousarray(bits[:, :nbytes + 2])
    got_crc = m.crc16(np.ascontiguousarray(out[:, :nbytes]))
    ok = (out[:, nbytes].astype(np.uint16) << 8 | out[:, nbytes + 1]) == got_crc
    assert int(ok.sum()) == good == F and np.array_equal(out[:, :nbytes], lk["payloads"])
    plain = dibits_to_bytes(m.scramble(s["out"][:, nsteps:]).cpu().numpy())
    assert sum(not crc_ok(oracle, p, nbytes) for p in plain) == hard_fail >= F // 2
    m.close()


def oracle_scrambled_bodies(orc, packets):
    return np.stack([orc.scramble_stream(conv_encode_ref(p[None, :], 8 * len(p))[0]) for p in packets])


# ------------------------------------------------------------------------------------------ 9. the error contract
def test_argument_errors_launch_nothing():
    import torch
    m = modem()
    R, n = 4, 100
    soft = torch.zeros((R, n, 2), dtype=torch.int8, device="cuda")
    flip = torch.zeros(n, dtype=torch.uint8, device="cuda")
    bits = torch.full((R * 13,), 0x55, dtype=torch.uint8, device="cuda")
    info = torch.full((R, 4), 0x55555555, dtype=torch.int32, device="cuda")

    def raw(soft=soft, pitch=0, R=R, n=n, flip=flip, flags=0, bits=bits, info=info, h=m.h):
        p = lambda a: a if isinstance(a, C.c_void_p) else ptr(a)      # noqa: E731
        return m.L.qpsk_viterbi_batch(h, p(soft), pitch, R, n, p(flip), flags, p(bits), p(info))

    assert raw() == 0
    m.sync()
    bits.fill_(0x55)
    info.fill_(0x55555555)
    cases = [dict(soft=None), dict(R=0), dict(R=-1), dict(n=0), dict(n=131073), dict(pitch=n - 1), dict(pitch=-3), dict(flags=4), dict(flags=-1),
             dict(flags=0x100), dict(bits=None, info=None), dict(soft=C.c_void_p(soft.data_ptr() + 1)), dict(h=None)]
    for i, c in enumerate(cases):
        assert raw(**c) == QPSK_ERR_ARG, (i, c)
    enc_in = torch.zeros((R, 13), dtype=torch.uint8, device="cuda")
    enc_out = torch.full((R * 106,), 0x55, dtype=torch.uint8, device="cuda")
    for a in ((None, ptr(enc_in), R, 100, 1, ptr(enc_out)), (m.h, None, R, 100, 1, ptr(enc_out)), (m.h, ptr(enc_in), R, 100, 1, None),
              (m.h, ptr(enc_in), 0, 100, 1, ptr(enc_out)), (m.h, ptr(enc_in), R, 0, 1, ptr(enc_out)), (m.h, ptr(enc_in), R, 100, 2, ptr(enc_out)),
              (m.h, ptr(enc_in), R, 131067, 1, ptr(enc_out)), (m.h, ptr(enc_in), R, 131073, 0, ptr(enc_out))):
        assert m.L.qpsk_conv_encode_batch(*a) == QPSK_ERR_ARG, a[2:5]
    m.sync()
    assert torch.all(bits == 0x55) and torch.all(info == 0x55555555) and torch.all(enc_out == 0x55)
    # the context still works
    z = random_soft(R, n, 1)
    assert_equal(run(m, z), viterbi_ref(z))
    m.sync()
    m.close()


def test_other_state_is_left_alone():
    """neither reads nor updates the histogram mode's guess"""
    import torch
    from oracle.pyoracle import TIMING_HIST
    from sigutil import make_frames
    L, F = 2048, 1024
    m = modem(frame_size=L, timing_mode=TIMING_HIST)
    x, _ = make_frames(F, L, 8, m.taps, 19200.0, offset_hz=40.0, base_seed=21, noise=0.01)
    xt = torch.from_numpy(x).cuda()
    m.rx_batch(xt)
    rx = m.rx_batch(xt, want_costas=True)
    st0, st1 = (C.c_int32 * 5)(), (C.c_int32 * 5)()
    m._check(m.L.qpsk_test_hist_state(m.h, st0))
    soft = m.soft(rx, skip=32)
    got = m.viterbi(soft, open_end=True)
    m.sync()
    m._check(m.L.qpsk_test_hist_state(m.h, st1))
    assert list(st0) == list(st1)
    want = viterbi_ref(soft_ref(rx["costas"].cpu().numpy(), skip=32)["soft"], flags=OPEN_END)
    assert np.array_equal(got["bits"].cpu().numpy(), want["bits"]) and np.array_equal(got["info"].cpu().numpy(), want["info"])
    m.close()
