"""The chunk loops of the decoder's scratch route and the one scratch buffer behind several calls.

qpsk_viterbi_batch, qpsk_viterbi_punct_batch and the decode of qpsk_deframer_push_coded cut a call into launches of at most 1 GiB of
decision words; no shape a test can afford reaches that, so the tuning key QPSK_VITERBI_CHUNK_ROWS lowers the cap and
qpsk_test_viterbi_launches says how many launches a call made (a key that did nothing would otherwise pass everything here).  Every row of
every case has its own random content, so a row of chunk 2 that lands on chunk 1's outputs, or is decoded from chunk 1's input, shows.
The references are the numpy restatements of the other test files; everything is bit for bit, there is no tolerance anywhere.
"""
import functools

import numpy as np
import pytest

from test_deframe_coded_cpu import coded_steps, deframe_coded_ref, dibits_to_costas, make_coded_packet
from test_deframe_coded_gpu import KEYS, raw_push, rec, rows_of
from test_deframe_coded_gpu import modem as plain_modem
from test_deframe_coded_gpu import push_all as push_coded
from test_deframe_coded_gpu import want_all as want_half
from test_deframe_coded_punct_gpu import want_all as want_punct
from test_deframe_cpu import turn
from test_punct_cpu import NAMED, deframe_coded_punct_ref, make_coded_punct_packet, punct_ntx, viterbi_punct_ref
from test_punct_gpu import run as run_punct
from test_punct_gpu import transmitted
from test_viterbi_cpu import OPEN_END, OPEN_START, viterbi_ref
from test_viterbi_gpu import assert_equal, modem, random_soft, run

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG = -2
CHUNKS = (None, 1, 2, 3, 7, 8)                 # None first: the unchunked run every other one must equal
BOTH_OPEN = OPEN_START | OPEN_END
CANARY = dict(bytes=0xA5, pos=-7, rot=-7, score=-7, crc_ok=0xA5, info=-7)      # raw_push's fill values


def launches_of(rows, chunk):
    return -(-rows // (rows if chunk is None else min(chunk, rows)))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("bits", "info") if k in a or k in b)


# ------------------------------------------------------------------------------------------ 1. batch decodes in chunks, rate 1/2
@pytest.mark.parametrize("R,n", [(7, 65), (7, 700), (3, 8200)])
def test_rate_half_batch_in_chunks_equals_the_unchunked_call_and_the_reference(R, n):
    import torch
    m = modem()
    soft = random_soft(R, n, 31 * n + R)
    soft[np.arange(R), (np.arange(R) * 37 + 5) % n, np.arange(R) & 1] = -128          # one in each row, taken as -127
    key = np.random.default_rng(n).integers(0, 4, n).astype(np.uint8)
    pitch = n + 31
    buf = np.full((R, pitch, 2), 0x7F, np.int8)
    buf[:, :n] = soft
    pitched = torch.from_numpy(buf).cuda()
    for flags in (0, BOTH_OPEN):
        want = viterbi_ref(soft, flip=key, flags=flags)
        whole = None
        for chunk in CHUNKS:
            m.tune(viterbi_chunk_rows=chunk)
            got = run(m, soft, flip=key, flags=flags, route=0)
            assert got["kernel"] == "viterbi_kernel", got["kernel"]
            assert m.viterbi_launches() == launches_of(R, chunk), (chunk, m.viterbi_launches())
            assert_equal(got, want, (flags, chunk))
            whole = whole or got
            assert same(got, whole), (flags, chunk)
            if flags == 0:                                   # r0 * row_pitch differs from r0 * n
                p = run(m, pitched, flip=key, pitch=pitch, nsteps=n, route=0)
                assert m.viterbi_launches() == launches_of(R, chunk) and p["kernel"] == "viterbi_kernel"
                assert_equal(p, want, ("pitched", chunk))
            else:                                            # the NULL side of each per-chunk offset
                for outs in (("bits",), ("info",)):
                    o = run(m, soft, flip=key, flags=flags, want=outs, route=0)
                    assert m.viterbi_launches() == launches_of(R, chunk) and set(o) == {"kernel", outs[0]}
                    assert_equal(o, want, (outs, chunk))
    # the key is the scratch route's alone: in LDS one launch, whatever it says; a row beyond the LDS limit stays on the scratch route
    want = viterbi_ref(soft, flip=key)
    for chunk in (1, 2):
        m.tune(viterbi_chunk_rows=chunk)
        got = run(m, soft, flip=key, route=1)
        if n <= 8192:
            assert got["kernel"] == "viterbi_lds_kernel" and m.viterbi_launches() == 1
        else:
            assert got["kernel"] == "viterbi_kernel" and m.viterbi_launches() == launches_of(R, chunk)
        assert_equal(got, want, ("lds", chunk))
    m.sync()
    m.close()


def test_a_chunk_of_no_rows_is_refused_and_a_negative_value_is_the_library_s_choice():
    m = modem()
    soft = random_soft(5, 70, 1)
    want = viterbi_ref(soft)
    m.tune(viterbi_chunk_rows=2)
    assert m.L.qpsk_ctx_set_tuning(m.h, b"QPSK_VITERBI_CHUNK_ROWS", 0) == QPSK_ERR_ARG
    assert_equal(run(m, soft, route=0), want)
    assert m.viterbi_launches() == 3                         # the refused call changed nothing
    m._check(m.L.qpsk_ctx_set_tuning(m.h, b"QPSK_VITERBI_CHUNK_ROWS", -5))
    assert_equal(run(m, soft, route=0), want)
    assert m.viterbi_launches() == 1
    # a refused call made no launch, and says so
    assert m.L.qpsk_viterbi_batch(m.h, None, 0, 5, 70, None, 0, None, None) == QPSK_ERR_ARG and m.viterbi_launches() == 0
    m.sync()
    m.close()


def test_the_environment_sets_the_key_at_context_creation_and_refuses_no_rows(monkeypatch):
    """read once, by qpsk_ctx_create: a number >= 1 is the cap, 0 is refused like the tuning call's, text that is no integer leaves the key unset"""
    import qpsk_amd
    soft = random_soft(5, 70, 2)
    want = viterbi_ref(soft)
    for text, launches in (("2", 3), ("abc", 1), ("-1", 1), ("2x", 1)):
        monkeypatch.setenv("QPSK_VITERBI_CHUNK_ROWS", text)
        m = modem()
        monkeypatch.delenv("QPSK_VITERBI_CHUNK_ROWS")                   # no later call reads it
        assert_equal(run(m, soft, route=0), want, text)
        assert m.viterbi_launches() == launches, (text, m.viterbi_launches())
        m.sync()
        m.close()
    monkeypatch.setenv("QPSK_VITERBI_CHUNK_ROWS", "0")
    with pytest.raises(qpsk_amd.QpskError, match="QPSK_VITERBI_CHUNK_ROWS"):
        modem()


# ------------------------------------------------------------------------------------------ 2. the same behind a puncturing pattern
@pytest.mark.parametrize("n", [65, 513])
@pytest.mark.parametrize("name", ["2/3", "7/8"])
def test_punctured_batch_in_chunks_equals_the_unchunked_call_and_the_reference(name, n):
    m = modem()
    R, pattern = 7, NAMED[name]
    ntx = punct_ntx(n, pattern)
    soft = transmitted(R, n, pattern, 13 * n + len(name))    # one -128 in each row
    key = np.random.default_rng(n + 1).integers(0, 4, ntx).astype(np.uint8)      # over the transmitted dibits
    buf = np.full((R, ntx + 5, 2), 0x7F, np.int8)
    buf[:, :ntx] = soft
    for flags in (0, BOTH_OPEN):
        want = viterbi_punct_ref(soft, n, pattern, flip=key, flags=flags)
        whole = None
        for chunk in CHUNKS:
            m.tune(viterbi_chunk_rows=chunk)
            got = run_punct(m, soft, n, pattern, flip=key, flags=flags, route=0)
            assert got["kernel"] == "viterbi_punct_kernel", got["kernel"]
            assert m.viterbi_launches() == launches_of(R, chunk), (chunk, m.viterbi_launches())
            assert_equal(got, want, (flags, chunk))
            whole = whole or got
            assert same(got, whole), (flags, chunk)
            if flags == 0:
                p = run_punct(m, buf, n, pattern, flip=key, pitch=ntx + 5, route=0)
                assert m.viterbi_launches() == launches_of(R, chunk)
                assert_equal(p, want, ("pitched", chunk))
            else:
                for outs in (("bits",), ("info",)):
                    o = run_punct(m, soft, n, pattern, flip=key, flags=flags, want=outs, route=0)
                    assert m.viterbi_launches() == launches_of(R, chunk)
                    assert_equal(o, want, (outs, chunk))
    want = viterbi_punct_ref(soft, n, pattern, flip=key)
    for chunk in (1, 2):
        m.tune(viterbi_chunk_rows=chunk)
        got = run_punct(m, soft, n, pattern, flip=key, route=1)
        assert got["kernel"] == "viterbi_punct_lds_kernel" and m.viterbi_launches() == 1
        assert_equal(got, want, ("lds", chunk))
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 3. the coded deframer's decode in chunks
DF = dict(S=5, M=4, nsync=16, nbytes=2, total=700, packets=(6, 0, 2, 5, 2), cuts=[200, 250, 250])
DF_CHUNKS = (None, 1, 3, 4, 7, 19, 20, 21)


@functools.lru_cache(maxsize=None)
def deframer_case(name):
    """five streams of short packets, every packet with its own payload and rotation: streams 0 and 3 hold more back-to-back packets than
    max_packets, stream 1 none, streams 2 and 4 two each -> everything the tests below share, references included (computed once)"""
    k = DF
    pattern = None if name == "1/2" else NAMED[name]
    rng = np.random.default_rng(2054 + len(name) + ord(name[0]))
    sync = rng.integers(0, 4, k["nsync"], dtype=np.uint8)
    make = (lambda: make_coded_packet(rng, sync, k["nbytes"])[0]) if pattern is None else \
           (lambda: make_coded_punct_packet(rng, sync, k["nbytes"], pattern)[0])
    d = rng.integers(0, 4, (k["S"], k["total"]), dtype=np.uint8)
    for s, c in enumerate(k["packets"]):
        t = int(rng.integers(3, 40))
        for _ in range(c):
            pkt = turn(make(), int(rng.integers(0, 4)))
            d[s, t:t + len(pkt)] = pkt
            t += len(pkt) + (0 if c > 2 else int(rng.integers(20, 200)))
        assert t <= k["total"]
    amp = rng.uniform(0.4, 2.0, k["S"])
    z = np.stack([dibits_to_costas(d[s], amp=amp[s], noise=0.15 * amp[s], rng=rng) for s in range(k["S"])])
    gain = rng.uniform(40.0, 90.0, k["S"]).astype(np.float32)
    min_score = k["nsync"] - 1
    if pattern is None:
        one = [deframe_coded_ref([z[s]], [gain[s]], sync, min_score, k["nbytes"])[0] for s in range(k["S"])]
    else:
        one = [deframe_coded_punct_ref([z[s]], [gain[s]], sync, min_score, k["nbytes"], pattern)[0] for s in range(k["S"])]
    assert [len(w) for w in one] == list(k["packets"])                       # the reference finds what was planted, and nothing else
    rows = rows_of(z, k["cuts"])
    edges = np.cumsum(k["cuts"])[:-1]
    Nc = coded_steps(k["nbytes"]) if pattern is None else punct_ntx(coded_steps(k["nbytes"]), pattern)
    gains3 = rng.uniform(40.0, 90.0, (3, k["S"])).astype(np.float32)
    want3 = {}
    for with_gain in (True, False):
        g = gains3 if with_gain else None
        want3[with_gain] = want_half(rows, g, sync, min_score, k["nbytes"]) if pattern is None else \
            want_punct(rows, g, sync, min_score, k["nbytes"], pattern)
        per_push = [sum(1 for r in w if r[0] == p) for w in want3[with_gain] for p in range(3)]
        assert max(per_push) <= k["M"]
    pending = sum(bool(((edges >= r[1] + k["nsync"]) & (edges < r[1] + k["nsync"] + Nc)).any()) for w in want3[True] for r in w)
    assert pending >= 1                                                       # a packet is pending across a push edge
    return dict(sync=sync, pattern=pattern, name=None if pattern is None else name, z=z, gain=gain, min_score=min_score, one=one, rows=rows,
                gains3=gains3, want3=want3, Nc=Nc)


def reset(m, c):
    m.deframer_reset_coded(DF["S"], c["sync"], DF["nbytes"], c["min_score"], max_packets=DF["M"], puncture=c["name"])


def check_one_push(o, want, which=KEYS):
    """raw_push's guarded buffers against the reference's packets per stream: the first max_packets records, the canary in every row at or
    beyond a stream's count, in the guard rows and in every output that was not handed over"""
    S, M = DF["S"], DF["M"]
    assert o["count"].tolist() == [len(w) for w in want]
    for s in range(S):
        for j in range(M):
            for key in KEYS:
                v = o[key][s * M + j]
                if key in which and j < len(want[s]):
                    assert np.array_equal(v, np.asarray(want[s][j][key]).astype(v.dtype)), (s, j, key, v, want[s][j][key])
                else:
                    assert (v == CANARY[key]).all(), (s, j, key)
    for key in KEYS:
        assert (o[key][S * M:] == CANARY[key]).all(), key


@pytest.mark.parametrize("name", ["1/2", "3/4"])
def test_coded_deframer_decode_in_chunks_equals_the_unchunked_push_and_the_reference(name):
    c = deframer_case(name)
    S, M = DF["S"], DF["M"]
    per = min(M, DF["total"] // (DF["nsync"] + c["Nc"]) + 1)
    assert per == 4
    m = plain_modem()
    m.tune(viterbi_lds=0)
    whole = None
    for chunk in DF_CHUNKS:
        m.tune(viterbi_chunk_rows=chunk)
        reset(m, c)
        o = raw_push(m, c["z"], c["gain"], M, DF["nbytes"])
        assert "<global>" in m.last_kernel() and ("punct" in m.last_kernel()) == (name != "1/2"), m.last_kernel()
        assert m.viterbi_launches() == launches_of(S * per, chunk), (chunk, m.viterbi_launches())
        check_one_push(o, c["one"])
        whole = whole or o
        assert all(np.array_equal(o[key], whole[key]) for key in KEYS + ("count",)), chunk
    # nothing to decode: no decode launch, and the hunt's outputs are as before
    m.tune(viterbi_chunk_rows=1)
    reset(m, c)
    o = raw_push(m, c["z"], c["gain"], M, DF["nbytes"], which=("pos", "rot", "score"))
    assert m.viterbi_launches() == 0 and m.last_kernel() == "deframe_coded_hunt_kernel"
    check_one_push(o, c["one"], which=("pos", "rot", "score"))
    # in LDS the key does nothing
    m.tune(viterbi_lds=1)
    reset(m, c)
    o = raw_push(m, c["z"], c["gain"], M, DF["nbytes"])
    assert "<lds>" in m.last_kernel() and m.viterbi_launches() == 1
    check_one_push(o, c["one"])
    m.close()


@pytest.mark.parametrize("with_gain", [True, False])
@pytest.mark.parametrize("name", ["1/2", "3/4"])
def test_one_row_per_launch_over_three_pushes_with_a_packet_pending_across_an_edge(name, with_gain):
    c = deframer_case(name)
    m = plain_modem()
    m.tune(viterbi_lds=0, viterbi_chunk_rows=1)
    reset(m, c)
    got = push_coded(m, c["rows"], c["gains3"] if with_gain else None)
    assert "<global>" in m.last_kernel()
    per = min(DF["M"], DF["cuts"][-1] // (DF["nsync"] + c["Nc"]) + 1)
    assert m.viterbi_launches() == DF["S"] * per > DF["S"]
    want = c["want3"][with_gain]
    for s in range(DF["S"]):
        assert got[s] == want[s], (s, got[s][:1], want[s][:1])
    assert [len(g) for g in got] == list(DF["packets"])
    m.close()


# ------------------------------------------------------------------------------------------ 4. one context, many decodes, one synchronisation
@functools.lru_cache(maxsize=None)
def sequence_case():
    rng = np.random.default_rng(77)
    c = dict(a=random_soft(2, 70, 70), big=random_soft(9, 2054, 2054), b=random_soft(2, 70, 71), long=random_soft(5, 8200, 8200))
    c["punct"] = transmitted(3, 513, NAMED["5/6"], 513)
    c["key_big"] = rng.integers(0, 4, 2054).astype(np.uint8)
    c["key_punct"] = rng.integers(0, 4, c["punct"].shape[1]).astype(np.uint8)
    c["want"] = dict(a=viterbi_ref(c["a"]), big=viterbi_ref(c["big"], flip=c["key_big"], flags=OPEN_END), b=viterbi_ref(c["b"], flags=BOTH_OPEN),
                     punct=viterbi_punct_ref(c["punct"], 513, NAMED["5/6"], flip=c["key_punct"]), long=viterbi_ref(c["long"]))
    assert not same(c["want"]["a"], viterbi_ref(c["b"]))                     # "other data" is other data
    return c


def records(o, push):
    """a deframe_coded() result as push_all's records per stream"""
    h = {key: o[key].cpu().numpy() for key in KEYS + ("count",)}
    return [[rec(push, {key: h[key][s, j] for key in KEYS}) for j in range(h["count"][s])] for s in range(len(h["count"]))]


def test_small_large_small_decodes_and_coded_pushes_on_one_context_with_one_synchronisation():
    """what a streaming host runs: the scratch buffer serves every call, regrows in the middle, and nothing is looked at before the end"""
    import torch
    c, d = sequence_case(), deframer_case("1/2")
    dev = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("a", "big", "b", "long", "punct", "key_big", "key_punct")}
    rows = [torch.from_numpy(r).cuda() for r in d["rows"][:2]]
    gains = [torch.from_numpy(g).cuda() for g in d["gains3"][:2]]
    m = plain_modem()
    m.tune(viterbi_lds=0)
    torch.cuda.synchronize()                                 # the uploads are over; from here on only the library's own waits
    for trip in range(2):                                    # the second trip finds the buffer already large
        m.tune(viterbi_chunk_rows=None)
        reset(m, d)
        held, counts = {}, {}
        held["a"] = m.viterbi(dev["a"])
        counts["a"] = m.viterbi_launches()
        held["push0"] = m.deframe_coded(rows[0], gains[0])
        counts["push0"] = m.viterbi_launches()
        held["big"] = m.viterbi(dev["big"], flip=dev["key_big"], open_end=True)      # regrows the scratch on the first trip
        held["punct"] = m.viterbi(dev["punct"], flip=dev["key_punct"], nsteps=513, puncture="5/6")
        held["push1"] = m.deframe_coded(rows[1], gains[1])
        held["b"] = m.viterbi(dev["b"], open_start=True, open_end=True)
        m.tune(viterbi_chunk_rows=2)
        held["long"] = m.viterbi(dev["long"])
        counts["long"] = m.viterbi_launches()
        m.sync()
        assert counts == dict(a=1, push0=1, long=3), counts
        for k in ("a", "big", "punct", "b", "long"):
            got = {q: held[k][q].cpu().numpy() for q in ("bits", "info")}
            assert_equal(got, c["want"][k], (trip, k))
        want = d["want3"][True]
        for p in range(2):
            got = records(held["push%d" % p], p)
            assert got == [[r for r in w if r[0] == p] for w in want], (trip, p)
    m.close()
