"""Data decisions (qpsk_rx_batch_data) and sync-word alignment (qpsk_sync_batch): what can be checked without a GPU.

data_rule() and sync_ref() below restate include/qpsk_hip.h in numpy; the GPU tests (test_rx_data_gpu.py) compare the kernels with them.
The packet test composes a whole link on the CPU oracle: payload + CRC-16 -> dibits -> scramble -> [prefix][sync][payload] ->
transmit -> receive (test_rx_ext_cpu.oracle_ext, costas_frame[]) -> data rule -> sync -> descramble -> pack -> CRC.
"""
import numpy as np
import pytest

from oracle.pyoracle import TAU
from sigutil import CONSTELLATION, splitmix64
from test_rx_ext_cpu import declared, oracle_ext

RING = np.array([0, 1, 3, 2], np.uint8)       # a dibit's place on the circle in quarter turns (its own inverse)
DATA_SYMBOLS = ("qpsk_rx_batch_data", "qpsk_sync_batch", "qpsk_multi_set_data")


def data_rule(costas):
    """(..., 2) float32 costas_frame[] -> (...) uint8: (z.im < 0) << 1 | (z.re < 0)"""
    z = np.asarray(costas, np.float32)
    return (((z[..., 1] < 0.0).astype(np.uint8) << 1) | (z[..., 0] < 0.0).astype(np.uint8)).astype(np.uint8)


def sync_ref(data, sync, lag_min, lag_max, nout):
    """-> dict(out (F, nout) uint8, lag, rot, score (F,) int32) by the definition: max score, ties to the smallest lag, then rotation"""
    data = np.atleast_2d(np.asarray(data, np.uint8))
    rs = RING[np.asarray(sync, np.uint8)].astype(np.int64)
    n = len(rs)
    F = data.shape[0]
    out = dict(out=np.zeros((F, nout), np.uint8), lag=np.zeros(F, np.int32), rot=np.zeros(F, np.int32), score=np.zeros(F, np.int32))
    for f in range(F):
        rd = RING[data[f] & 3].astype(np.int64)
        win = np.lib.stride_tricks.sliding_window_view(rd, n)[lag_min:lag_max + 1]          # (W, n)
        d = (win - rs) & 3
        sc = np.stack([(d == r).sum(axis=1) for r in range(4)], axis=1)                     # (W, 4): score(lag_min + w, r)
        k = int(np.argmax(sc.reshape(-1)))                                                  # first maximum: smallest lag, then rotation
        L, r = lag_min + k // 4, k % 4
        out["lag"][f], out["rot"][f], out["score"][f] = L, r, sc[k // 4, r]
        out["out"][f] = RING[(rd[L + n:L + n + nout] - r) & 3]
    return out


def bytes_to_dibits(b):
    """byte k -> dibits 4k .. 4k+3, low bits first (the packing of qpsk_pack_symbols)"""
    b = np.asarray(b, np.uint8)
    return np.stack([(b >> (2 * j)) & 3 for j in range(4)], axis=-1).reshape(*b.shape[:-1], -1).astype(np.uint8)


def dibits_to_bytes(d):
    d = np.asarray(d, np.uint8).reshape(*np.shape(d)[:-1], -1, 4)
    return (d[..., 0] | (d[..., 1] << 2) | (d[..., 2] << 4) | (d[..., 3] << 6)).astype(np.uint8)


def transmit(sym, L, C, taps, fs, offset_hz=0.0, phase=0.0, noise=0.0, seed=0):
    """sigutil.make_frames for given symbols, with a carrier phase: (L, 2) float32"""
    up = np.zeros(L, np.complex128)
    up[::C] = CONSTELLATION[np.asarray(sym)[:L // C]]
    y = np.convolve(up, np.asarray(taps, np.float64))[:L] * 1.85
    n = np.arange(L, dtype=np.float64)
    y = y * np.exp(1j * (2 * np.pi * offset_hz * n / fs + phase))
    if noise > 0.0:
        rng = np.random.Generator(np.random.PCG64(splitmix64(seed + 77)))
        y = y + noise * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    out = np.zeros((L, 2), np.float32)
    out[:, 0], out[:, 1] = y.real, y.imag
    return out


def make_packet_frame(orc, rng, nsym, prefix, sync, nbytes):
    """[prefix random dibits][sync][scrambled payload + CRC-16 (big-endian) as dibits][random fill] -> (symbols, payload bytes)"""
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8)
    crc = orc.crc16(payload.tobytes())
    packet = np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])
    body = orc.scramble_stream(bytes_to_dibits(packet))
    sym = rng.integers(0, 4, nsym, dtype=np.uint8)
    sym[prefix:prefix + len(sync)] = sync
    sym[prefix + len(sync):prefix + len(sync) + len(body)] = body
    return sym, payload


# ------------------------------------------------------------------- ABI (fails without the feature)
def test_data_entry_points_are_declared_bound_and_exported(qpsk_lib):
    from qpsk_amd.lib import API_SYMBOLS
    for name in DATA_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name


def test_python_front_ends_exist():
    import qpsk_amd
    for name in ("rx_batch_data", "sync"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    assert callable(getattr(qpsk_amd.MultiJob, "set_data", None))


def test_sync_kernel_is_built_and_writes_no_scalar_memory():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "qpsk_amd", "csrc", "sync.hip")).read().lower()
    assert "sync.o" in open(os.path.join(root, "qpsk_amd", "csrc", "Makefile")).read()
    for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_d" + "cache_"):
        assert word not in src, word


def test_data_streams_are_generated_and_differ_only_in_the_flush():
    """tools/gen_lean_asm.py --data (run by the Makefile): the five streams, through the generator's register-liveness guard, with the
    ROT45 multiply and the sum / difference gone and nothing else changed"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = lambda *a: subprocess.run([sys.executable, "tools/gen_lean_asm.py", *a], cwd=root, capture_output=True, text=True,  # noqa: E731
                                    check=True).stdout
    data, product = run("--data"), run()
    names = [ln.split("(")[0].split()[-1] for ln in data.splitlines() if ln.startswith("__device__")]
    assert names == ["fir_lean_loop1_data", "fir_lean_loop2_data", "fir_lean_loop1_dma_data", "fir_lean_loop2_dma_data",
                     "fir_lean_loop2_dma2w_data"]
    body = lambda text: [ln.strip() for ln in text.splitlines() if ln.strip().startswith('"')]  # noqa: E731
    d, p = body(data), body(product)
    dropped = [ln for ln in p if ln not in d]
    # what the data streams lack: the ROT45 multiplies, the sum / difference, and the selects that read them (they read T instead)
    assert dropped and all(("v_pk_mul_f32" in ln and "op_sel_hi:[1,0]" in ln) or ln.startswith(('"v_sub_f32', '"v_add_f32', '"v_cndmask'))
                           for ln in dropped), [ln for ln in dropped if "cndmask" not in ln][:4]
    # six instructions fewer per unit and flush (two packed multiplies, two subtractions, two additions), stream by stream
    import re
    count = lambda text: [(int(u), int(n)) for u, n in re.findall(r"/\* (\d) unit\(s\) per wave: (\d+) instructions", text)]  # noqa: E731
    assert [(u, n - 6 * u) for u, n in count(product)] == count(data)


# ------------------------------------------------------------------- the numpy restatements, on hand cases
def test_data_rule_hand_cases():
    z = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1], [0.0, 0.0], [-0.0, -0.0], [-0.0, 1], [1, -0.0], [np.nan, -1], [-1, np.nan]],
                 np.float32)
    assert list(data_rule(z)) == [0, 1, 3, 2, 0, 0, 0, 0, 2, 1]
    # at the loop's rotation 0 the transmitted constellation point, turned 45 degrees onto the diagonal, gives back its dibit
    rot = np.exp(1j * np.pi / 4) * CONSTELLATION.astype(np.complex128)
    assert list(data_rule(np.stack([rot.real, rot.imag], -1).astype(np.float32))) == [0, 1, 2, 3]


def test_ring_is_its_own_inverse():
    assert list(RING[RING]) == [0, 1, 2, 3]


def test_sync_ref_hand_cases():
    sync = np.array([0, 1, 2, 3, 3, 0], np.uint8)
    data = np.zeros(40, np.uint8)
    data[7:13] = sync
    data[13:17] = [1, 2, 3, 0]
    r = sync_ref(data, sync, 0, 30, 4)
    assert (r["lag"][0], r["rot"][0], r["score"][0]) == (7, 0, 6) and list(r["out"][0]) == [1, 2, 3, 0]
    # the same word and payload turned by every quarter turn: the lag stays, the rotation is found, the payload comes back
    for q in range(4):
        turned = RING[(RING[data] + q) & 3]
        r = sync_ref(turned, sync, 0, 30, 4)
        assert (r["lag"][0], r["rot"][0], r["score"][0]) == (7, q, 6) and list(r["out"][0]) == [1, 2, 3, 0]
    # exact ties: the smallest lag wins, then the smallest rotation; only the low two bits are read
    r = sync_ref(np.full(20, 4 | 1, np.uint8), [1, 1], 3, 10, 0)
    assert (r["lag"][0], r["rot"][0], r["score"][0]) == (3, 0, 2)
    r = sync_ref(np.zeros(20, np.uint8), [1, 1], 2, 10, 0)
    assert (r["lag"][0], r["rot"][0], r["score"][0]) == (2, 3, 2)       # ring[0] - ring[1] = -1 = 3 quarter turns
    # a window of one lag, the whole row
    r = sync_ref(np.arange(12, dtype=np.uint8) & 3, [3, 2], 0, 0, 10)
    assert (r["lag"][0], r["rot"][0], r["score"][0]) == (0, 2, 2) and r["out"].shape == (1, 10)


def test_pack_round_trip():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(dibits_to_bytes(bytes_to_dibits(b)), b)


# ------------------------------------------------------------------- a whole link on the oracle
def test_packet_through_the_oracle(oracle):
    """payload + CRC -> scramble -> [prefix][sync][payload] -> transmit with a carrier phase -> receive at offset 6 -> data rule -> sync ->
    descramble -> pack: the CRC matches and L* = prefix + 126 // C, at all four carrier quarter turns"""
    fs, rs, C, L = 19200.0, 2400.0, 8, 16384
    nsym, nbytes, prefix = L // C, 64, 100
    taps = oracle.rrc_make(np.float32(fs), np.float32(rs), np.float32(0.35))
    rng = np.random.default_rng(31)
    sync = rng.integers(0, 4, 64, dtype=np.uint8)
    frames, payloads = [], []
    for f in range(4):
        sym, pl = make_packet_frame(oracle, rng, nsym, prefix, sync, nbytes)
        frames.append(transmit(sym, L, C, taps, fs, offset_hz=30.0, phase=0.3 + f * np.pi / 2, noise=0.02, seed=f))
        payloads.append(pl)
    x = np.stack(frames)
    got = oracle_ext(oracle, x, fs, rs, np.full(4, 126 % C, np.int32), None, loop_bw=np.float32(TAU / 100.0), want_costas=True)
    data = data_rule(got["costas"])
    nout = 4 * (nbytes + 2)
    s = sync_ref(data, sync, 0, 255, nout)
    rots = set()
    for f in range(4):
        assert s["lag"][f] == prefix + 126 // C and s["score"][f] == len(sync), (f, s["lag"][f], s["score"][f])
        rots.add(int(s["rot"][f]))
        packet = dibits_to_bytes(oracle.scramble_stream(s["out"][f]))
        assert np.array_equal(packet[:nbytes], payloads[f])
        crc = oracle.crc16(packet[:nbytes].tobytes())
        assert (int(packet[nbytes]) << 8 | int(packet[nbytes + 1])) == crc
    assert len(rots) == 4, rots
