"""qpsk_conv_encode_punct_batch / qpsk_viterbi_punct_batch / Modem.conv_encode, Modem.viterbi with puncture= on the GPU: decoded bits and all
four info words bit for bit against test_punct_cpu.viterbi_punct_ref (PUNCTURING of include/qpsk_hip.h restated in numpy) on both routes,
the two identities the header states, the encoder against conv_encode_punct_ref, a loopback that stays on the device, and the error
contract.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_punct_cpu import (ALL_FLAGS, ALL_PATTERNS, BAD_PATTERNS, NAMED, conv_encode_punct_ref, depuncture_ref, punct_nsent, punct_ntx,
                            viterbi_punct_ref)
from test_viterbi_cpu import OPEN_END, pack_bits, viterbi_ref
from test_viterbi_gpu import GUARD, assert_equal, modem, ptr, random_soft
from test_viterbi_gpu import run as run_half

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG = -2
LDS_ROUTE, SCRATCH_ROUTE = "viterbi_punct_lds_kernel", "viterbi_punct_kernel"
ROUTES = ((0, SCRATCH_ROUTE), (1, LDS_ROUTE), (None, LDS_ROUTE))


def run(m, soft, nsteps, pattern, flip=None, flags=0, pitch=0, want=("bits", "info"), route=None):
    """the raw call with guarded outputs; soft: numpy (R, ntx or pitch, 2) int8"""
    import torch
    q = torch.from_numpy(np.ascontiguousarray(soft, np.int8)).cuda()
    R, nb = q.shape[0], (nsteps + 7) // 8
    f = None if flip is None else torch.from_numpy(np.ascontiguousarray(flip, np.uint8)).cuda()
    bufs = {}
    if "bits" in want:
        bufs["bits"] = torch.full((R * nb + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    if "info" in want:
        bufs["info"] = torch.full((R * 4 + GUARD,), 0x55555555, dtype=torch.int32, device="cuda")
    m.tune(viterbi_lds=route)
    m._check(m.L.qpsk_viterbi_punct_batch(m.h, ptr(q), pitch, R, nsteps, *pattern, ptr(f), flags, ptr(bufs.get("bits")), ptr(bufs.get("info"))))
    kernel = m.last_kernel()
    torch.cuda.synchronize()
    out = {"kernel": kernel}
    for k, b in bufs.items():
        h = b.cpu().numpy()
        size = h.size - GUARD
        assert np.all(h[size:] == (0x55 if k == "bits" else 0x55555555)), "guard behind %s overwritten" % k
        out[k] = h[:size].reshape((R, nb) if k == "bits" else (R, 4))
    return out


def transmitted(R, nsteps, pattern, seed):
    """random soft rows as transmitted, (R, ntx, 2): the pad value of an odd nsent is garbage like the rest, one -128 in every row at a
    value that is read"""
    soft = random_soft(R, punct_ntx(nsteps, pattern), seed)
    flat = soft.reshape(R, -1)
    flat[:, punct_nsent(nsteps, pattern) // 2] = -128
    return soft


# ------------------------------------------------------------------------------------------ 1. random rows, every shape, both routes
@pytest.mark.parametrize("n", [1, 5, 6, 7, 63, 64, 65, 129, 513, 2054])
def test_random_rows_bit_for_bit_on_both_routes(n):
    """64 is coprime to 3, 5 and 7: the blocks of 64 steps and the periods drift against each other.  The references of every pattern and
    flip are computed in one viterbi_ref call per flag value (its rows are independent)"""
    m = modem()
    cases, rows = [], []
    for name, pattern in sorted(ALL_PATTERNS.items()):
        soft = transmitted(3, n, pattern, 10 * n + len(name))
        key = np.random.default_rng(n).integers(0, 4, soft.shape[1]).astype(np.uint8)
        for flip in (None, key):
            cases.append((name, pattern, soft, flip))
            rows.append(depuncture_ref(soft, n, pattern, flip))
    odd = [name for name, pattern, _, _ in cases if punct_nsent(n, pattern) & 1]
    assert odd or n == 1, n                                             # every length but 1 meets an odd nsent under some pattern
    for flags in ALL_FLAGS:
        ref = viterbi_ref(np.concatenate(rows), flags=flags)
        for i, (name, pattern, soft, flip) in enumerate(cases):
            want = {k: ref[k][3 * i:3 * i + 3] for k in ("bits", "info")}
            for R in (1, 3):
                for route, kernel in ROUTES:
                    got = run(m, soft[:R], n, pattern, flip=flip, flags=flags, route=route)
                    assert got["kernel"] == kernel, (route, got["kernel"])
                    assert_equal(got, {k: v[:R] for k, v in want.items()}, (name, R, flags, flip is None, route))
    m.sync()
    m.close()


@pytest.mark.parametrize("n", [5, 7, 65])
def test_the_pad_value_and_the_gap_of_a_pitched_row_are_never_read(n):
    m = modem()
    seen_odd = 0
    for name, pattern in sorted(ALL_PATTERNS.items()):
        ntx, nsent = punct_ntx(n, pattern), punct_nsent(n, pattern)
        seen_odd += nsent & 1
        soft = transmitted(3, n, pattern, n + len(name))
        key = np.random.default_rng(n + 1).integers(0, 4, ntx).astype(np.uint8)
        want = viterbi_punct_ref(soft, n, pattern, flip=key, flags=OPEN_END)
        outs = []
        for fill in (0x7F, -0x80):
            buf = np.full((3, ntx + 5, 2), fill, np.int8)
            buf[:, :ntx] = soft
            if nsent & 1:
                buf[:, ntx - 1, 1] = fill                                # the pad value
            for route in (0, 1):
                outs.append(run(m, buf, n, pattern, flip=key, flags=OPEN_END, pitch=ntx + 5, route=route))
                assert_equal(outs[-1], want, (name, fill, route))
        assert all(np.array_equal(o["bits"], outs[0]["bits"]) and np.array_equal(o["info"], outs[0]["info"]) for o in outs)
    assert seen_odd >= 2, seen_odd
    m.sync()
    m.close()


def test_a_row_longer_than_the_lds_limit_takes_the_scratch_route():
    m = modem()
    n, pattern = 8200, NAMED["7/8"]
    soft = transmitted(2, n, pattern, 82)
    key = np.random.default_rng(83).integers(0, 4, soft.shape[1]).astype(np.uint8)
    want = viterbi_punct_ref(soft, n, pattern, flip=key)
    for route in (None, 1):
        got = run(m, soft, n, pattern, flip=key, route=route)
        assert got["kernel"] == SCRATCH_ROUTE, got["kernel"]
        assert_equal(got, want, route)
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. the two identities, GPU against GPU
@pytest.mark.parametrize("n", [65, 2054])
def test_identity_1_the_punctured_call_equals_the_rate_half_call_on_the_zero_filled_row(n):
    m = modem()
    for name, pattern in sorted(ALL_PATTERNS.items()):
        soft = transmitted(3, n, pattern, n + 7 * len(name))
        key = np.random.default_rng(n).integers(0, 4, soft.shape[1]).astype(np.uint8)
        for flip in (None, key):
            filled = depuncture_ref(soft, n, pattern, flip)
            for flags in (0, OPEN_END):
                for route in (0, 1):
                    a = run(m, soft, n, pattern, flip=flip, flags=flags, route=route)
                    b = run_half(m, filled, flip=None, flags=flags, route=route)
                    assert "punct" in a["kernel"] and "punct" not in b["kernel"]
                    assert_equal(a, b, (name, flip is None, flags, route))
    m.sync()
    m.close()


@pytest.mark.parametrize("n", [7, 65, 2054])
def test_identity_2_the_pattern_1_1_1_equals_the_rate_half_call_with_the_same_flip(n):
    m = modem()
    soft = random_soft(3, n, n)
    soft[:, n // 2, 1] = -128
    key = np.random.default_rng(n).integers(0, 4, n).astype(np.uint8)
    for flip in (None, key):
        for flags in ALL_FLAGS:
            for route in (0, 1):
                a = run(m, soft, n, NAMED["1/2"], flip=flip, flags=flags, route=route)
                b = run_half(m, soft, flip=flip, flags=flags, route=route)
                assert "punct" in a["kernel"] and "punct" not in b["kernel"]
                assert_equal(a, b, (flip is None, flags, route))
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 3. ties, saturation, all zeros
@pytest.mark.parametrize("kind", ["saturated", "ties", "zeros"])
def test_saturating_tying_and_empty_rows_at_rate_3_4(kind):
    m = modem()
    pattern = NAMED["3/4"]
    for n in (70, 2054):
        ntx = punct_ntx(n, pattern)
        soft = np.zeros((3, ntx, 2), np.int8) if kind == "zeros" else random_soft(3, ntx, n, kind)
        for flags in ALL_FLAGS:
            want = viterbi_punct_ref(soft, n, pattern, flags=flags)
            for route in (0, 1):
                assert_equal(run(m, soft, n, pattern, flags=flags, route=route), want, (kind, n, flags, route))
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 4. the encoder
@pytest.mark.parametrize("nbits", [1, 7, 64, 527, 528])
def test_encoder_equals_the_restatement(nbits):
    import torch
    m = modem()
    R = 5
    rng = np.random.default_rng(nbits)
    packed = rng.integers(0, 256, (R, (nbits + 7) // 8), dtype=np.uint8)        # the padding bits of the last byte are garbage on purpose
    pt = torch.from_numpy(packed).cuda()
    odd = 0
    for name, pattern in sorted(ALL_PATTERNS.items()):
        for tail in (True, False):
            want = conv_encode_punct_ref(packed, nbits, pattern, tail=tail)
            nsent = punct_nsent(nbits + (6 if tail else 0), pattern)
            got = m.conv_encode(packed, nbits, tail=tail, puncture=pattern)
            assert m.last_kernel() == "conv_encode_punct_kernel"
            m.sync()
            assert np.array_equal(got.cpu().numpy(), want), (name, nbits, tail)
            if nsent & 1:
                odd += 1
                assert not (got.cpu().numpy()[:, -1] & 2).any()          # the pad bit is 0
            ntx = want.shape[1]
            out = torch.full((R * ntx + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
            m._check(m.L.qpsk_conv_encode_punct_batch(m.h, ptr(pt), R, nbits, 1 if tail else 0, *pattern, ptr(out)))
            m.sync()
            assert np.array_equal(out[:R * ntx].cpu().numpy().reshape(R, ntx), want) and torch.all(out[R * ntx:] == 0x55), (name, tail)
    assert odd, nbits
    key = "3/4"
    assert np.array_equal(m.conv_encode(packed, nbits, puncture=key).cpu().numpy(), conv_encode_punct_ref(packed, nbits, NAMED[key]))
    m.close()


# ------------------------------------------------------------------------------------------ 5. a loopback that stays on the device
@pytest.mark.parametrize("name", sorted(NAMED))
def test_device_loopback(name):
    """conv_encode(puncture) -> scramble -> soft values at +-64 -> viterbi(puncture, flip = keystream) returns the bits, no channel errors"""
    import torch
    m = modem()
    R, nbits = 6, 528
    nsteps = nbits + 6
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, (R, nbits), dtype=np.uint8)
    tx = m.scramble(m.conv_encode(pack_bits(bits), nbits, puncture=name))
    ntx = m.punct_ntx(nsteps, name)
    assert tx.shape == (R, ntx) and ntx == punct_ntx(nsteps, NAMED[name])
    key = m.scramble(torch.zeros((1, ntx), dtype=torch.uint8))[0]
    d = tx.to(torch.int16)
    soft = torch.stack([64 - 128 * (d & 1), 64 - 64 * (d & 2)], dim=-1).to(torch.int8)
    got = m.viterbi(soft, flip=key, nsteps=nsteps, puncture=name)
    assert "punct" in m.last_kernel()
    m.sync()
    out = np.unpackbits(got["bits"].cpu().numpy(), axis=1, bitorder="little")
    assert np.array_equal(out[:, :nbits], bits) and not out[:, nbits:nsteps].any()
    info = got["info"].cpu().numpy()
    assert not info[:, 3].any() and np.all(info[:, 0] == 64 * punct_nsent(nsteps, NAMED[name])) and not info[:, 1:3].any()
    with pytest.raises(ValueError):
        m.viterbi(soft, flip=key, puncture=name)                        # nsteps is required: ntx does not determine it
    m.close()


# ------------------------------------------------------------------------------------------ 6. the error contract
def test_argument_errors_launch_nothing():
    import torch
    m = modem()
    R, n, pattern = 4, 100, NAMED["3/4"]
    ntx = punct_ntx(n, pattern)
    soft = torch.zeros((R, ntx, 2), dtype=torch.int8, device="cuda")
    flip = torch.zeros(ntx, dtype=torch.uint8, device="cuda")
    bits = torch.full((R * 13,), 0x55, dtype=torch.uint8, device="cuda")
    info = torch.full((R, 4), 0x55555555, dtype=torch.int32, device="cuda")

    def raw(soft=soft, pitch=0, R=R, n=n, pattern=pattern, flip=flip, flags=0, bits=bits, info=info, h=m.h):
        p = lambda a: a if isinstance(a, C.c_void_p) else ptr(a)      # noqa: E731
        return m.L.qpsk_viterbi_punct_batch(h, p(soft), pitch, R, n, *pattern, p(flip), flags, p(bits), p(info))

    assert raw() == 0
    m.sync()
    bits.fill_(0x55)
    info.fill_(0x55555555)
    cases = [dict(soft=None), dict(R=0), dict(n=0), dict(n=131073), dict(pitch=ntx - 1), dict(pitch=-3), dict(flags=4), dict(flags=0x100),
             dict(bits=None, info=None), dict(soft=C.c_void_p(soft.data_ptr() + 1)), dict(h=None)] + [dict(pattern=b) for b in BAD_PATTERNS]
    for i, c in enumerate(cases):
        assert raw(**c) == QPSK_ERR_ARG, (i, c)
    enc_in = torch.zeros((R, 13), dtype=torch.uint8, device="cuda")
    enc_out = torch.full((R * 106,), 0x55, dtype=torch.uint8, device="cuda")
    enc = lambda h, i, R, nbits, flags, pattern, o: m.L.qpsk_conv_encode_punct_batch(h, i, R, nbits, flags, *pattern, o)  # noqa: E731
    for a in ((None, ptr(enc_in), R, 100, 1, pattern, ptr(enc_out)), (m.h, None, R, 100, 1, pattern, ptr(enc_out)),
              (m.h, ptr(enc_in), R, 100, 1, pattern, None), (m.h, ptr(enc_in), 0, 100, 1, pattern, ptr(enc_out)),
              (m.h, ptr(enc_in), R, 0, 1, pattern, ptr(enc_out)), (m.h, ptr(enc_in), R, 100, 2, pattern, ptr(enc_out)),
              (m.h, ptr(enc_in), R, 131067, 1, pattern, ptr(enc_out))) + tuple((m.h, ptr(enc_in), R, 100, 1, b, ptr(enc_out)) for b in BAD_PATTERNS):
        assert enc(*a) == QPSK_ERR_ARG, a[2:6]
    sw = (C.c_uint8 * 16)(*([1, 2, 3, 0] * 4))
    for b in BAD_PATTERNS:
        assert m.L.qpsk_deframer_reset_coded_punct(m.h, 2, sw, 16, 14, 4, 4, 0, 64.0, *b) == QPSK_ERR_ARG, b
    with pytest.raises(ValueError):
        m.punct_ntx(100, "4/5")
    m.sync()
    assert torch.all(bits == 0x55) and torch.all(info == 0x55555555) and torch.all(enc_out == 0x55)
    # the context still works
    z = transmitted(R, n, pattern, 1)
    assert_equal(run(m, z, n, pattern), viterbi_punct_ref(z, n, pattern))
    m.sync()
    m.close()
