"""qpsk_viterbi_stream_* on the GPU over the NEW sets of vstream_rows: flushes on the block grid with bits waiting, streams of a few steps,
ties of the best state and of the steps, the rings' corners (decisions while the trace grows, one window of 4096, 128 blocks with
dblk = 127), thirty one-period pushes of every pattern, 300 streams, rows 2 bytes off a dword at odd pitches, the longest push.  Every call
goes through the raw C entry with the guards of test_viterbi_stream_gpu.call (0x55 behind bits and info, the bytes beyond a call's bits
untouched) and is compared with test_viterbi_stream_cpu.viterbi_stream_ref -- the definition, not the port -- bit for bit: the bits, their
count and all four info words, with no tolerance; the kernel of every call is checked.  The scalar port runs the same sets in
test_vstream_port_cpu.py, where the faults these sets are there to catch are listed."""
import numpy as np
import pytest

from test_viterbi_gpu import modem
from test_viterbi_stream_gpu import flush, push, same
from vstream_rows import NEW, get, run_ref, soft_image

pytestmark = pytest.mark.gpu


def run_set(name):
    """every step of a set on the device, each call compared with the reference -> the calls' outputs"""
    import torch
    s = get(name)
    want, got = run_ref(s, state=False), []
    m = modem()
    S = kernel = None
    for step in s["steps"]:
        if step[0] == "reset":
            S, pattern = step[1], step[4]
            m.viterbi_stream_reset(S, step[2], step[3], puncture=pattern)
            assert m.last_kernel() == "viterbi_stream_init_kernel"
            kernel = "viterbi_stream_kernel" if tuple(pattern) == (1, 1, 1) else "viterbi_stream_punct_kernel"
        elif step[0] == "advance":
            m.viterbi_stream_advance(step[1])
        elif step[0] == "push":
            soft, o = step[1], step[2]
            ntx, pitch = soft.shape[1], o["pitch"] or soft.shape[1]
            image = soft_image(soft, o["pitch"], o["off"], o["fill"])
            d_all = torch.from_numpy(image).cuda()
            assert d_all.data_ptr() % 4 == 0
            rows = d_all[o["off"]:o["off"] + 2 * S * pitch].view(torch.int8).view(S, pitch, 2)
            g = push(m, rows, want=o["want"], slack=o["slack"], pitch=o["pitch"], ntx=ntx)
            assert g["kernel"] == kernel, (name, len(got), g["kernel"])
            assert np.array_equal(d_all.cpu().numpy(), image), "the input was written"
            same(g, want[len(got)], (name, "call", len(got), "push", ntx))
            got.append(g)
        else:
            g = flush(m, S, step[1], want=step[2])
            assert g["kernel"] == "viterbi_stream_flush_kernel"
            same(g, want[len(got)], (name, "call", len(got), "flush", step[1]))
            got.append(g)
    assert len(got) == len(want)
    m.sync()
    m.close()
    return got


@pytest.mark.parametrize("name", NEW)
def test_the_device_equals_the_reference_on_the_set(name):
    got = run_set(name)
    assert sum(g["nbits"] for g in got) > 0
