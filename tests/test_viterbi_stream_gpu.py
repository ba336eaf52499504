"""qpsk_viterbi_stream_* and qpsk_conv_encode_stream_batch on the GPU: the emitted bits, their count and all four info words of EVERY call bit
for bit against test_viterbi_stream_cpu.viterbi_stream_ref (VITERBI STREAM of include/qpsk_hip.h restated in numpy).  Every stream of every
case has its own random content, full-range int8 with erasures and -128 sprinkled in; the shapes are the smallest that reach each branch:
pushes that end off a 64-step block (pending pairs), rings of two blocks and of a size neither D nor W divides, the limit D + W = 8192,
positions past 2^31, every named pattern.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_coded_gpu import planted_costas, push_all, rows_of
from test_punct_cpu import NAMED, popc
from test_viterbi_cpu import OPEN_END, dibits_to_soft, pack_bits, unpack_bits, viterbi_ref
from test_viterbi_gpu import assert_equal, modem, ptr
from test_viterbi_gpu import run as run_batch
from test_viterbi_stream_cpu import TERMINATED, conv_encode_stream_ref, push_steps, random_soft, viterbi_stream_ref

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
GUARD = 64
FLUSH_PITCH = 1024                      # a flush emits fewer than D + W <= 8192 bits
SPLIT = (1, 63, 64, 65, 127, 129, 2)


def call(m, S, want, bits_pitch, fn):
    """a raw push or flush with guarded outputs: fn(d_bits, bits_pitch, d_info, h_nbits) -> rc"""
    import torch
    bits = torch.full((S * bits_pitch + GUARD,), 0x55, dtype=torch.uint8, device="cuda") if "bits" in want else None
    info = torch.full((S * 4 + GUARD,), 0x55555555, dtype=torch.int32, device="cuda") if "info" in want else None
    n = C.c_int(-9)
    m._check(fn(ptr(bits), bits_pitch, ptr(info), C.byref(n)))
    out = dict(kernel=m.last_kernel(), nbits=n.value)
    torch.cuda.synchronize()
    nb = (n.value + 7) // 8
    if bits is not None:
        h = bits.cpu().numpy()
        rows = h[:S * bits_pitch].reshape(S, bits_pitch)
        assert (h[S * bits_pitch:] == 0x55).all() and (rows[:, nb:] == 0x55).all(), "bytes beyond the call's bits were written"
        out["bits"] = rows[:, :nb]
    if info is not None:
        h = info.cpu().numpy()
        assert (h[S * 4:] == 0x55555555).all(), "guard behind info overwritten"
        out["info"] = h[:S * 4].reshape(S, 4)
    return out


def push(m, soft, want=("bits", "info"), slack=0, pitch=0, ntx=None):
    """soft: numpy (S, ntx, 2) int8 or, with pitch, a device tensor (S, pitch, 2); the bits rows are `slack` bytes further apart than needed"""
    import torch
    q = soft if hasattr(soft, "data_ptr") else torch.from_numpy(np.ascontiguousarray(soft, np.int8)).cuda()
    ntx = q.shape[1] if ntx is None else ntx
    nbits = m.viterbi_stream_emits(ntx)
    got = call(m, q.shape[0], want, nbits // 8 + slack,
               lambda b, bp, i, n: m.L.qpsk_viterbi_stream_push(m.h, ptr(q), pitch, ntx, b, bp, i, n))
    assert got["nbits"] == nbits, "qpsk_viterbi_stream_emits and the push disagree"
    return got


def flush(m, S, flags=0, want=("bits", "info")):
    return call(m, S, want, FLUSH_PITCH, lambda b, bp, i, n: m.L.qpsk_viterbi_stream_flush(m.h, flags, b, bp, i, n))


def same(got, want, what=""):
    assert got["nbits"] == want["nbits"], (what, got["nbits"], want["nbits"])
    assert_equal(got, want, what)


def pieces(total, split=SPLIT):
    """the repeating split, cut off at total"""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(split[k % len(split)], total - sum(out)))
        k += 1
    return out


def run_both(m, ref, soft, sizes, what=""):
    """push soft (S, ntx, 2) in pushes of `sizes` dibits through the device and the restatement, every call compared -> the device's calls"""
    calls, at = [], 0
    for k, size in enumerate(sizes):
        got = push(m, soft[:, at:at + size])
        same(got, ref.push(soft[:, at:at + size]), (what, "push", k, size))
        calls.append(got)
        at += size
    assert at == soft.shape[1]
    return calls


def all_bits(calls):
    return np.concatenate([unpack_bits(c["bits"], c["nbits"]) for c in calls], axis=1)


# ------------------------------------------------------------------------------------------ 1. push splits and partition independence
def test_pushes_off_the_block_grid_on_a_ring_of_two_blocks_and_one_push_of_the_same():
    S, N = 5, 1000
    m = modem()
    soft = random_soft(np.random.default_rng(1), S, N)
    ref = viterbi_stream_ref(S, 64, 64)
    m.viterbi_stream_reset(S, 64, 64)
    calls = run_both(m, ref, soft, pieces(N))
    assert calls[0]["kernel"] == "viterbi_stream_kernel"
    got = flush(m, S)
    same(got, ref.flush(), "flush")
    assert got["kernel"] == "viterbi_stream_flush_kernel" and got["nbits"] == N - (N // 64 * 64 - 64)
    cut = all_bits(calls + [got])
    # the same content in one push (the flush left the streams as after a reset)
    one = push(m, soft)
    same(one, ref.push(soft), "one push")
    end = flush(m, S)
    same(end, ref.flush(), "its flush")
    whole = all_bits([one, end])
    assert whole.shape == (S, N) and np.array_equal(cut, whole)
    assert np.array_equal(sum(c["info"][:, :2].astype(np.int64) for c in calls + [got]), one["info"][:, :2].astype(np.int64) + end["info"][:, :2])
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. window and depth combinations
@pytest.mark.parametrize("depth,window", [(192, 128), (64, 192)])
def test_rings_that_neither_depth_nor_window_divides(depth, window):
    S, N = 3, 1500
    m = modem()
    soft = random_soft(np.random.default_rng(depth), S, N)
    ref = viterbi_stream_ref(S, depth, window)
    m.viterbi_stream_reset(S, depth, window)
    calls = run_both(m, ref, soft, pieces(N, (300, 1, 450, 77)))
    assert sum(c["nbits"] for c in calls) == N // window * window - depth
    same(flush(m, S, TERMINATED), ref.flush(TERMINATED), "flush")
    m.sync()
    m.close()


def test_the_limit_of_8192_steps_of_ring_and_a_refused_reset_that_leaves_the_armed_stream():
    S, N = 2, 9000
    m = modem()
    soft = random_soft(np.random.default_rng(4096), S, N)
    ref = viterbi_stream_ref(S, 4096, 4096)
    m.viterbi_stream_reset(S, 4096, 4096)
    same(push(m, soft[:, :4000]), ref.push(soft[:, :4000]), "push 0")
    for depth, window in ((4160, 4096), (4096, 4160), (64, 8192), (0, 64), (64, 32), (96, 64), (64, 100)):
        assert m.L.qpsk_viterbi_stream_reset(m.h, S, depth, window, 1, 1, 1) == QPSK_ERR_ARG, (depth, window)
    assert m.L.qpsk_viterbi_stream_reset(m.h, 0, 64, 64, 1, 1, 1) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_stream_reset(m.h, S, 64, 64, 3, 0x8, 0x1) == QPSK_ERR_ARG      # a mask bit above the period
    got = push(m, soft[:, 4000:8200])                         # the decision at 8192 walks the whole ring and emits the first 4096 bits
    same(got, ref.push(soft[:, 4000:8200]), "push 1")
    assert got["nbits"] == 4096
    same(push(m, soft[:, 8200:]), ref.push(soft[:, 8200:]), "push 2")
    same(flush(m, S), ref.flush(), "flush")
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 3. punctured pushes
@pytest.mark.parametrize("name", ["2/3", "3/4", "5/6", "7/8"])
def test_punctured_pushes_of_whole_periods_and_a_refused_push_of_a_broken_one(name):
    pattern = NAMED[name]
    K = popc(pattern[1]) + popc(pattern[2])
    unit = K // 2 if K % 2 == 0 else K                       # the dibits of the shortest legal push: 7/8 -> 4
    sizes = [unit * k for k in (1, 2, 9, 65)] * 2            # 7/8: ntx = 4, 8, 36, 260
    S = 3
    m = modem()
    soft = random_soft(np.random.default_rng(K), S, sum(sizes))
    ref = viterbi_stream_ref(S, 64, 64, pattern)
    m.viterbi_stream_reset(S, 64, 64, puncture=name)
    at = sum(sizes[:3])
    calls = run_both(m, ref, soft[:, :at], sizes[:3], name)
    assert calls[0]["kernel"] == "viterbi_stream_punct_kernel"
    bad = unit - 1 if unit > 1 else 0
    assert push_steps(bad, pattern) is None
    import torch
    q = torch.from_numpy(soft[:, :max(bad, 1)].copy()).cuda()
    buf = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
    assert m.L.qpsk_viterbi_stream_push(m.h, ptr(q), 0, bad, ptr(buf), 64, None, None) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_stream_emits(m.h, bad) == QPSK_ERR_ARG
    calls += run_both(m, ref, soft[:, at:], sizes[3:], name)  # the refused push left the state alone
    assert sum(c["nbits"] for c in calls) > 0
    same(flush(m, S), ref.flush(), "flush")
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 4. property 2 against the row decoders themselves
@pytest.mark.parametrize("name,N", [("1/2", 700), ("3/4", 702)])      # behind 3/4 a push holds whole periods of 3 steps
@pytest.mark.parametrize("flags", [0, TERMINATED])
def test_a_flush_before_anything_was_emitted_equals_the_batch_decoder(name, N, flags):
    pattern = NAMED[name]
    S = 4
    ntx = N * (popc(pattern[1]) + popc(pattern[2])) // pattern[0] // 2
    assert push_steps(ntx, pattern) == N
    m = modem()
    soft = random_soft(np.random.default_rng(N + flags), S, ntx)
    m.viterbi_stream_reset(S, 512, 512, puncture=name)
    a = m.viterbi_stream(soft[:, :240])                       # the Python binding's calls
    b = m.viterbi_stream(soft[:, 240:])
    assert a["nbits"] == 0 and b["nbits"] == 0 and tuple(b["bits"].shape) == (S, 0)
    assert (a["info"].cpu().numpy() == [0, 0, -1, 0]).all() and (b["info"].cpu().numpy()[:, :2] == 0).all()
    got = m.viterbi_stream_flush(terminated=bool(flags))
    row_flags = dict(open_end=not flags)
    want = m.viterbi(soft, **row_flags) if name == "1/2" else m.viterbi(soft, nsteps=N, puncture=name, **row_flags)
    assert got["nbits"] == N
    assert np.array_equal(got["bits"].cpu().numpy(), want["bits"].cpu().numpy())
    winfo, ginfo = want["info"].cpu().numpy(), got["info"].cpu().numpy()
    assert np.array_equal(ginfo[:, 0], winfo[:, 3]) and np.array_equal(ginfo[:, 2], winfo[:, 1])
    ref = viterbi_stream_ref(S, 512, 512, pattern)
    ref.push(soft)
    want_ref = ref.flush(flags)
    assert np.array_equal(ginfo, want_ref["info"]) and np.array_equal(got["bits"].cpu().numpy(), want_ref["bits"])
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 5. pitches, canaries, NULL outputs
def test_pitched_rows_null_outputs_and_a_bits_pitch_one_byte_short():
    import torch
    S, N, P = 3, 520, 531
    m = modem()
    soft = random_soft(np.random.default_rng(5), S, N)
    buf = np.full((S, P, 2), 0x7F, np.int8)
    buf[:, :N // 2] = soft[:, :N // 2]
    ref = viterbi_stream_ref(S, 64, 128)
    m.viterbi_stream_reset(S, 64, 128)
    want = ref.push(soft[:, :N // 2])
    same(push(m, torch.from_numpy(buf).cuda(), pitch=P, ntx=N // 2, slack=5), want, "pitched")
    q = torch.from_numpy(soft[:, N // 2:].copy()).cuda()
    nbits = m.viterbi_stream_emits(N // 2)
    assert nbits == 256
    out = torch.full((S * 64,), 0x55, dtype=torch.uint8, device="cuda")
    info = torch.full((S * 4,), 0x55555555, dtype=torch.int32, device="cuda")
    n = C.c_int(-9)
    assert m.L.qpsk_viterbi_stream_push(m.h, ptr(q), 0, N // 2, None, 0, None, C.byref(n)) == QPSK_ERR_ARG        # every output NULL
    assert m.L.qpsk_viterbi_stream_push(m.h, ptr(q), 0, N // 2, ptr(out), nbits // 8 - 1, ptr(info), C.byref(n)) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_stream_push(m.h, ptr(q), N // 2 - 1, N // 2, ptr(out), 64, ptr(info), C.byref(n)) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_stream_push(m.h, None, 0, N // 2, ptr(out), 64, ptr(info), C.byref(n)) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_stream_flush(m.h, 0, None, 0, None, C.byref(n)) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_stream_flush(m.h, 2, ptr(out), 64, ptr(info), C.byref(n)) == QPSK_ERR_ARG              # unknown flag
    assert m.L.qpsk_viterbi_stream_flush(m.h, 0, ptr(out), (N // 2 - 192 + 7) // 8 - 1, ptr(info), C.byref(n)) == QPSK_ERR_ARG      # 68 bits are waiting: one byte short
    torch.cuda.synchronize()
    assert n.value == -9 and (out.cpu().numpy() == 0x55).all() and (info.cpu().numpy() == 0x55555555).all()     # nothing launched
    want = ref.push(soft[:, N // 2:])                         # the state is untouched: the legal push matches
    only_bits = push(m, soft[:, N // 2:], want=("bits",))
    assert set(only_bits) == {"kernel", "nbits", "bits"}
    same(only_bits, want, "bits only")
    want = ref.flush()
    only_info = flush(m, S, want=("info",))
    same(only_info, want, "info only")
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 6. reset and flush state
def test_state_errors_rearming_and_a_flush_that_leaves_a_fresh_stream():
    import torch
    m = modem()
    soft = random_soft(np.random.default_rng(6), 4, 600)
    q = torch.from_numpy(soft).cuda()
    out = torch.zeros(4 * 1024, dtype=torch.uint8, device="cuda")
    assert m.L.qpsk_viterbi_stream_push(m.h, ptr(q), 0, 600, ptr(out), 1024, None, None) == QPSK_ERR_STATE
    assert m.L.qpsk_viterbi_stream_flush(m.h, 0, ptr(out), 1024, None, None) == QPSK_ERR_STATE
    assert m.L.qpsk_viterbi_stream_emits(m.h, 600) == QPSK_ERR_STATE
    assert m.L.qpsk_test_viterbi_stream_advance(m.h, 0) == QPSK_ERR_STATE
    m.viterbi_stream_reset(4, 64, 64)
    assert m.last_kernel() == "viterbi_stream_init_kernel"
    ref = viterbi_stream_ref(4, 64, 64)
    run_both(m, ref, soft, [333, 267])
    # a reset in mid-stream re-arms to a fresh state
    m.viterbi_stream_reset(4, 64, 64)
    ref = viterbi_stream_ref(4, 64, 64)
    run_both(m, ref, soft[:, ::-1], [100, 500])
    # another stream count and another pattern
    m.viterbi_stream_reset(2, 128, 64, puncture="3/4")
    ref = viterbi_stream_ref(2, 128, 64, NAMED["3/4"])
    run_both(m, ref, soft[:2], [200, 400])
    same(flush(m, 2), ref.flush(), "flush")
    # after the flush: as after a reset, and a flush of nothing emits nothing
    run_both(m, ref, soft[2:], [90, 510])
    same(flush(m, 2, TERMINATED), ref.flush(TERMINATED), "second flush")
    empty = flush(m, 2)
    same(empty, ref.flush(), "flush of nothing")
    assert empty["nbits"] == 0
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 7. isolation
def test_a_batch_decode_on_the_scratch_route_and_a_coded_deframer_push_between_two_pushes():
    S = 3
    rng = np.random.default_rng(7)
    m, other = modem(), modem()
    soft = random_soft(rng, S, 900)
    rows = random_soft(rng, 6, 700)
    sync = rng.integers(0, 4, 20, dtype=np.uint8)
    z = rows_of(planted_costas(rng, S, 1500, sync, 8), [700, 800])
    for x in (m, other):
        x.deframer_reset_coded(S, sync, 8, 12)
    ref = viterbi_stream_ref(S, 128, 64)
    m.viterbi_stream_reset(S, 128, 64)
    run_both(m, ref, soft[:, :450], [450])
    got_rows = run_batch(m, rows, flags=OPEN_END, route=0)
    assert got_rows["kernel"] == "viterbi_kernel"
    assert_equal(got_rows, viterbi_ref(rows, flags=OPEN_END), "batch between pushes")
    first = push_all(m, z[:1])
    run_both(m, ref, soft[:, 450:], [450])
    second = push_all(m, z[1:])
    same(flush(m, S), ref.flush(), "flush")
    want = push_all(other, z[:1]), push_all(other, z[1:])     # the same deframer pushes with no stream decoder beside them
    assert (first, second) == want and sum(len(s) for s in first + second) > 0
    m.sync()
    other.sync()
    m.close()
    other.close()


# ------------------------------------------------------------------------------------------ 8. positions past 2^31
def test_positions_past_2_to_the_31_change_nothing():
    S, depth, window = 3, 192, 128                            # a ring of 5 blocks: 2^40 / 64 is no multiple of it
    m = modem()
    soft = random_soft(np.random.default_rng(8), S, 1400)
    ref = viterbi_stream_ref(S, depth, window)
    m.viterbi_stream_reset(S, depth, window)
    run_both(m, ref, soft[:, :300], [300])
    assert m.L.qpsk_test_viterbi_stream_advance(m.h, 1 << 40) == QPSK_ERR_STATE      # fewer than depth + window steps so far
    run_both(m, ref, soft[:, 300:421], [121])
    for delta in (-1, (1 << 62) + window, 64, window + 1):
        assert m.L.qpsk_test_viterbi_stream_advance(m.h, delta) == QPSK_ERR_ARG, delta
    m.viterbi_stream_advance(1 << 40)
    calls = run_both(m, ref, soft[:, 421:], [3, 400, 576])
    assert sum(c["nbits"] for c in calls) == 1024 - 128
    m.viterbi_stream_advance((1 << 62) // window * window)
    same(flush(m, S), ref.flush(), "flush")
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 9. loopback on the device
@pytest.mark.parametrize("name", ["1/2", "7/8"])
def test_loopback_through_the_stream_encoder_in_three_chunks(name):
    import torch
    pattern = NAMED[name]
    S, chunk = 4, 840                                         # whole periods and whole dibits of both patterns
    m = modem()
    data = np.random.default_rng(9).integers(0, 2, (S, 3 * chunk)).astype(np.uint8)
    m.viterbi_stream_reset(S, 64, 64, puncture=name)
    state, want_state, out = None, None, []
    for k in range(3):
        part = pack_bits(data[:, k * chunk:(k + 1) * chunk])
        dibits, state = m.conv_encode_stream(part, chunk, state=state, puncture=name)
        assert m.last_kernel() == "conv_encode_stream_kernel"
        want_dibits, want_state = conv_encode_stream_ref(part, chunk, pattern, want_state)
        assert np.array_equal(dibits.cpu().numpy(), want_dibits) and np.array_equal(state.cpu().numpy(), want_state)
        soft = torch.where((dibits[..., None] >> torch.arange(2, device=dibits.device)) & 1 != 0, -64, 64).to(torch.int8)
        assert np.array_equal(soft.cpu().numpy(), dibits_to_soft(want_dibits))
        out.append(m.viterbi_stream(soft))
    out.append(m.viterbi_stream_flush())
    m.sync()
    got = np.concatenate([unpack_bits(o["bits"].cpu().numpy(), o["nbits"]) for o in out], axis=1)
    assert np.array_equal(got, data)
    assert not sum(o["info"].cpu().numpy()[:, 0] for o in out).any()
    # what the encoder refuses: half a period, an odd number of sent bits, aliased states
    b = torch.zeros((S, 105), dtype=torch.uint8, device="cuda")
    st = torch.zeros(S, dtype=torch.uint8, device="cuda")
    o = torch.zeros((S, 1024), dtype=torch.uint8, device="cuda")
    assert m.L.qpsk_conv_encode_stream_batch(m.h, ptr(b), S, 10, 7, 0x51, 0x2F, None, None, ptr(o)) == QPSK_ERR_ARG
    assert m.L.qpsk_conv_encode_stream_batch(m.h, ptr(b), S, 2, 2, 0x1, 0x3, None, None, ptr(o)) == QPSK_ERR_ARG
    assert m.L.qpsk_conv_encode_stream_batch(m.h, ptr(b), S, 8, 1, 1, 1, ptr(st), ptr(st), ptr(o)) == QPSK_ERR_ARG
    # the two states inside one allocation: S bytes each, touching on either side (accepted, the row encoded as ever), one byte shared (refused)
    part, before = pack_bits(data[:, :chunk]), np.array([5, 63, 0, 17], np.uint8)
    want_dibits, want_state = conv_encode_stream_ref(part, chunk, pattern, before)
    d_part, both = torch.from_numpy(part).cuda(), torch.zeros(2 * S, dtype=torch.uint8, device="cuda")
    for i0, o0, accepted in ((0, S, True), (S, 0, True), (0, S - 1, False), (S - 1, 0, False)):
        both.zero_()
        both[i0:i0 + S] = torch.from_numpy(before).cuda()
        rc = m.L.qpsk_conv_encode_stream_batch(m.h, ptr(d_part), S, chunk, *pattern, C.c_void_p(both.data_ptr() + i0), C.c_void_p(both.data_ptr() + o0), ptr(o))
        if not accepted:
            assert rc == QPSK_ERR_ARG and b"d_state_out overlaps d_state_in" in m.L.qpsk_last_error(), (i0, o0, rc)
            continue
        assert rc == 0, (i0, o0, m.L.qpsk_last_error())
        m.sync()
        assert np.array_equal(o.reshape(-1)[:want_dibits.size].cpu().numpy().reshape(want_dibits.shape), want_dibits)
        assert np.array_equal(both[o0:o0 + S].cpu().numpy(), want_state) and np.array_equal(both[i0:i0 + S].cpu().numpy(), before)
    m.sync()
    m.close()
