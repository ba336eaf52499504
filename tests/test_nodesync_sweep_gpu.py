"""qpsk_nodesync_* on the GPU over the sets of nodesync_rows: candidate x head x input alignment in full, every int8 pair, a switch at every
push through every candidate, the longest push, products that need 64 bits.  Every output byte and every d_info word of every push against
test_nodesync_cpu.nodesync_ref, bit for bit, through the raw call with the poison and guard checks of test_nodesync_gpu.ns_push (the input's
first row may begin 4 bytes behind a 16-byte boundary here, so the buffers are laid out by nodesync_rows.image: the very images the scalar
port runs on in test_nodesync_port_cpu.py).  Every launch is nodesync_push_kernel or nodesync_init_kernel.  A set's reference is computed
once and serves both of its streams: they differ in where the input stands, not in what it holds."""
import ctypes as C

import numpy as np
import pytest

from nodesync_rows import GUARD, get, image, run_ref, walk_recut
from test_nodesync_cpu import minus128, turn_ref
from test_nodesync_gpu import POISON, QPSK_ERR_ARG, cand_tensor, same
from test_viterbi_gpu import modem, ptr

pytestmark = pytest.mark.gpu


def push_at(m, step, in_off):
    """ns_push with the input's first row in_off bytes behind a 16-byte boundary; d_vinfo goes in as a device tensor"""
    import torch
    _, soft, vinfo, ip, op, want_info = step
    S, ntx = soft.shape[:2]
    d_in_all = torch.from_numpy(image(soft, ip or ntx, S, ntx, in_off)).cuda()
    d_out_all = torch.from_numpy(image(None, op or ntx, S, ntx, 2)).cuda()
    assert d_in_all.data_ptr() % 16 == 0 and d_out_all.data_ptr() % 16 == 0
    d_v = None if vinfo is None else torch.from_numpy(np.ascontiguousarray(vinfo, np.int32)).cuda()
    info = torch.full((S * 8 + GUARD,), POISON, dtype=torch.int32, device="cuda") if want_info else None
    m._check(m.L.qpsk_nodesync_push(m.h, C.c_void_p(d_in_all.data_ptr() + in_off), ip, ntx, ptr(d_v), C.c_void_p(d_out_all.data_ptr() + 2), op, ptr(info)))
    assert m.last_kernel() == "nodesync_push_kernel"
    torch.cuda.synchronize()
    h = d_out_all.cpu().numpy()
    pitch = op or ntx
    rows = h[2:2 + 2 * S * pitch].reshape(S, pitch, 2)
    assert (h[:2] == 0x55).all() and (h[2 + 2 * S * pitch:] == 0x55).all() and (rows[:, ntx:] == 0x55).all(), "bytes outside the rows were written"
    assert np.array_equal(d_in_all.cpu().numpy(), image(soft, ip or ntx, S, ntx, in_off)), "the input was written"
    out = dict(soft=rows[:, :ntx].copy().view(np.int8))
    if info is not None:
        h = info.cpu().numpy()
        assert (h[S * 8:] == POISON).all(), "guard behind d_info overwritten"
        out["info"] = h[:S * 8].reshape(S, 8)
    return out


def run_set(m, s, stream=0, before=None):
    """every step of a set on the device, each push compared with the reference -> the pushes' outputs.  before: {push index: a call made
    in front of that push}"""
    want, got = run_ref(s), []
    for step in s["steps"]:
        if step[0] == "reset":
            m.nodesync_reset(step[1], **step[2])
            assert m.last_kernel() == "nodesync_init_kernel"
        elif step[0] == "set":
            m.nodesync_set(None if step[1] is None else cand_tensor(step[1]))
            assert m.last_kernel() == "nodesync_init_kernel"
        else:
            k = len(got)
            if before and k in before:
                before[k]()
            got.append(push_at(m, step, s["streams"][stream]))
            same(got[-1], {key: v for key, v in want[k].items() if key in got[-1]}, (s["name"], "stream", stream, "push", k, "ntx", step[1].shape[1]))
    m.sync()
    return got


@pytest.mark.parametrize("nshift", [2, 32])
def test_every_candidate_at_every_head_and_both_input_alignments(nshift):
    s = get("sweep(%d)" % nshift)
    m = modem()
    for stream in range(2):
        got = run_set(m, s, stream)
        assert np.array_equal(got[-1]["info"][:, 0] + 4 * got[-1]["info"][:, 1], (np.arange(len(s["cand"])) // 8) % s["C"])
    m.close()


def test_every_int8_pair_beside_two_sets_of_neighbours():
    s = get("every_pair()")
    m = modem()
    got = run_set(m, s)
    assert not any((g["soft"] == -128).any() for g in got)
    x = s["steps"][2][1][0]                                       # the definition once more, on the first push of the links at h = 0
    for r in range(4):
        assert np.array_equal(got[0]["soft"][r], turn_ref(minus128(x), r))
    m.close()


def test_products_of_which_one_side_passes_2_31():
    m = modem()
    got = run_set(m, get("products()"))
    assert [g["info"][0, 2:5].tolist() for g in got] == [[0, 1, 2], [1, 0, 1]]
    m.close()


def test_a_switch_at_every_push_through_every_delay_and_the_wrap():
    """all 130 pushes and the set in their middle, bit for bit; then the cuts: with A(l, t) the device's output for dibit t of link l (the
    pushes concatenated) and B(l, t) nodesync_ref's over the same dibits, ticks and set with the lengths of every pair of pushes swapped,
    A(l, t) == B(l, t) for every dibit t that lies in the push of the same index in both runs -- there both stand on the same candidate
    l + p + 1 (+ 37 behind the set), and the output may depend on nothing else.  That is every dibit but the one between the two cuts inside
    each pair."""
    s = get("walk()")
    m = modem()
    got = run_set(m, s)
    for k, g in enumerate(got):
        assert (g["info"][:, 3] == k + 1).all(), k               # switches counts every move; the set left it alone
    A = np.concatenate([g["soft"] for g in got], axis=1)
    B, push_b, push_a = walk_recut()
    agree = push_a == push_b
    assert A.shape == B.shape and 0.95 < agree.mean() < 1.0
    assert np.array_equal(A[:, agree], B[:, agree])
    m.close()


def test_the_longest_push_and_the_refusal_of_one_dibit_more():
    import torch
    s = get("limit()")
    m = modem()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def one_too_many():
        before = m.last_kernel()
        rc = m.L.qpsk_nodesync_push(m.h, ptr(buf), 0, (1 << 20) + 1, None, ptr(buf[2048:]), 0, None)
        assert rc == QPSK_ERR_ARG and b"ntx = 1048577 outside" in m.L.qpsk_last_error(), (rc, m.L.qpsk_last_error())
        assert m.last_kernel() == before
    got = run_set(m, s, before={2: one_too_many})                # the push behind the refusal finds history and candidate as they were
    assert got[0]["soft"].shape[1] == 1 << 20 and got[0]["info"][0, :2].tolist() == [3, 31]
    # 31 dibits at h = 31: every one is the turn of the push before's last 31, none of this push's row
    assert np.array_equal(got[1]["soft"][0], turn_ref(minus128(s["soft"][0, (1 << 20) - 31:1 << 20]), 3))
    m.close()
