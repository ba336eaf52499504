"""qpsk_multi_* (include/qpsk_hip.h, MULTI; qpsk_amd/csrc/multi.cpp) where test_abi.test_multi_job_against_the_oracle stops: that test, and
the multi tests of test_rx_ext_gpu / test_rx_data_gpu, feed ONE batch to every step, so a slot that returned the previous step's rows, a
copy-back from the wrong slot or context scratch leaking from one step into the next would all pass them.  Here every pipelined step
has a batch of its own in every timing mode and output mode, the shardings are degenerate, a kernel status appears while two slots are
in flight, and a begin() fails on one shard only.  Every comparison is bit for bit against the oracle or an exact return code."""
import os

import numpy as np
import pytest

from oracle.pyoracle import TIMING_FFT, TIMING_FIXED, TIMING_HIST
from sigutil import bits_equal, make_frames, random_frames
from test_rx_data_cpu import data_rule

pytestmark = pytest.mark.gpu

FS, RS = 19200.0, 2400.0
FIXED_INDEX = 6
QPSK_ERR_ARG, QPSK_ERR_HIP, QPSK_ERR_STATE, QPSK_ERR_RANGE = -2, -3, -5, -6
NTHR = min(16, os.cpu_count() or 1)
NSTEPS = 5
# timing mode -> (frame_size, frames, shards): 2048 is what the one-pass histogram route serves; 38 + 39, 25 + 25 + 25 and 100 + 100 + 101
# frames per shard: an odd shard in every mode
SHAPES = {TIMING_FIXED: (1024, 77, [0, 0]), TIMING_HIST: (2048, 75, [0, 0, 0]), TIMING_FFT: (1024, 301, [0, 0, 0])}
MODE_NAMES = {TIMING_FIXED: "fixed", TIMING_HIST: "hist", TIMING_FFT: "fft"}


def job(devices, L, mode):
    import qpsk_amd
    return qpsk_amd.MultiJob(devices, fs=FS, rs=RS, frame_size=L, timing_mode=mode, fixed_index=FIXED_INDEX)


def reference(oracle, x, mode):
    w = oracle.rx_batch(x, FS, RS, timing_mode=mode, fixed_index=FIXED_INDEX, want_costas=True, threads=NTHR)
    w["data"] = data_rule(w.pop("costas"))
    return w


def step_batch(taps, mode, F, L, k):
    """step k's batch: other symbols, another offset and another delay every step"""
    seed = 1000 * (k + 1) + mode
    if mode == TIMING_FIXED:
        x, _ = make_frames(F, L, 8, taps, FS, offset_hz=45.0 - 20.0 * k, base_seed=seed, noise=0.03)
        return x
    if mode == TIMING_FFT:
        x, _ = make_frames(F, L + 8, 8, taps, FS, offset_hz=20.0 + 5.0 * k, base_seed=seed, noise=0.05)
        return np.ascontiguousarray(x[:, (3 * k) % 8:(3 * k) % 8 + L])
    # histogram timing, as test_histogram_mode_in_one_pass_on_a_guessed_index builds its batches: clean frames, a few noise and tone
    # frames off the majority index; every other step delayed by three samples, so that the previous step's guess is wrong for every
    # clean frame and the fall-back list is full
    delay = 3 * (k & 1)
    x, _ = make_frames(F, L + 8, 8, taps, FS, offset_hz=40.0, base_seed=seed, noise=0.03)
    x = np.ascontiguousarray(x[:, delay:delay + L])
    x[1::29] = random_frames(len(x[1::29]), L, seed=seed + 1)
    rng, n = np.random.default_rng(seed), np.arange(L)
    for f in range(3, F, 31):
        z = np.exp(1j * rng.uniform(0.01, 0.5) * n) * rng.uniform(0.2, 3)
        x[f, :, 0], x[f, :, 1] = z.real, z.imag
    return x


@pytest.fixture(scope="module")
def stimulus(oracle):
    """mode -> NSTEPS (batch, the oracle's rows of it), built once and left unchanged"""
    taps = oracle.rrc_make(FS, RS, np.float32(0.35))
    memo = {}

    def get(mode):
        if mode not in memo:
            L, F, _ = SHAPES[mode]
            xs = [step_batch(taps, mode, F, L, k) for k in range(NSTEPS)]
            memo[mode] = [(x, reference(oracle, x, mode)) for x in xs]
        return memo[mode]
    return get


@pytest.fixture(scope="module")
def clean(oracle):
    """one clean 77-frame batch (38 + 39 on two shards, 25 + 26 + 26 on three) and the oracle's rows"""
    taps = oracle.rrc_make(FS, RS, np.float32(0.35))
    x, _ = make_frames(77, 1024, 8, taps, FS, offset_hz=45.0, base_seed=5, noise=0.03)
    return x, reference(oracle, x, TIMING_FIXED)


def assert_rows(got, want, what, sym_key="sym"):
    sym, freq, phase = got
    assert bits_equal(sym, want[sym_key]), "%s: symbols differ in frames %s" % (what, np.nonzero((sym != want[sym_key]).any(axis=1))[0][:8])
    assert bits_equal(freq, want["freq"]), "%s: freq differs" % (what,)
    assert bits_equal(phase, want["phase"]), "%s: phase differs" % (what,)


def one_step(mj, slot, want, what):
    out = mj.outputs()
    mj.begin(slot)
    mj.end(slot, *out)
    assert_rows(out, want, what)


# ---------------------------------------------------------------------------- 1. each step returns that step's rows
def run_distinct_steps(mj, steps, output):
    """begin(0); [new input]; begin(1); end(0); [new input]; begin(0); end(1); ... on the caller's own device buffers, every step's
    gathered rows against the oracle's rows of THAT step's batch"""
    import torch
    total = steps[0][0].shape[0]
    mj.load(total=total)
    shards = [mj.shard(r) for r in range(mj.L.qpsk_multi_shards(mj.h))]
    lent = []
    for r, sh in enumerate(shards):
        t = torch.empty((sh["count"], mj.frame_size, 2), dtype=torch.float32, device="cuda")
        mj.use_device_input(r, t)
        lent.append(t)

    def feed(x):
        # The shards' streams are non-blocking: nothing orders them against the stream torch copies on.  The device-wide
        # synchronisations do -- the first lets every kernel that still reads the tensors finish, the second lands the new frames
        # before the next begin() enqueues its kernel.
        torch.cuda.synchronize()
        for sh, t in zip(shards, lent):
            t.copy_(torch.from_numpy(x[sh["first"]:sh["first"] + sh["count"]]))
        torch.cuda.synchronize()

    if output == "packed":
        mj.set_packed(True)
    if output == "data":
        mj.set_data(True)
    pinned = None
    if output == "direct":
        pinned = [mj.pinned_outputs(), mj.pinned_outputs()]
        for slot in (0, 1):
            mj.set_direct(slot, *pinned[slot])

    def begin(k):
        if pinned:
            for a in pinned[k & 1]:
                a.view(np.uint8)[...] = 0xEE      # the slot's last results are gone: what end() finds is this step's DMA
        mj.begin(k & 1)

    def end(k):
        if pinned:
            mj.end(k & 1)
            got = tuple(a.copy() for a in pinned[k & 1])
        else:
            got = mj.outputs()
            for a in got:
                a.view(np.uint8)[...] = 0xEE
            mj.end(k & 1, *got)
        if output == "packed":
            got = (mj.unpack(got[0]),) + tuple(got[1:])
        assert_rows(got, steps[k][1], "step %d (slot %d)" % (k, k & 1), sym_key="data" if output == "data" else "sym")

    feed(steps[0][0])
    begin(0)
    for k in range(1, len(steps)):
        feed(steps[k][0])
        begin(k)
        end(k - 1)
    end(len(steps) - 1)


@pytest.mark.parametrize("output", ["staging", "packed", "direct", "data"])
@pytest.mark.parametrize("mode", [TIMING_FIXED, TIMING_HIST, TIMING_FFT], ids=lambda m: MODE_NAMES[m])
def test_every_step_returns_its_own_rows(stimulus, mode, output):
    """NSTEPS pipelined steps, a different batch each, in every timing mode and output mode (staging, packed, direct DMA into pinned arrays
    on both slots, data decisions).  TIMING_FIXED with QPSK_PIPE_G = 4 on every shard: rx_lean_kernel on batches that are neither whole
    workgroups nor even (39 frames), so both slots go through the context's one pad buffer (c->sympad) and the copy behind the launch.
    TIMING_FFT with the library's own choice.  TIMING_HIST three times on fresh jobs: the one-pass route forced (every second step's
    guess misses every clean frame: c->index, c->mislist and the guess are shared by the slots), off, and left to the library -- there
    the route a step takes depends on what the host reads from the previous step's statistics, so only the results are asserted.
    Data mode takes its indices from the two-launch estimate and keeps no books: one run."""
    L, F, devices = SHAPES[mode]
    steps = stimulus(mode)
    runs = [None]
    if mode == TIMING_HIST and output != "data":
        runs = [1, 0, None]
    for onepass in runs:
        mj = job(devices, L, mode)
        try:
            for r in range(len(devices)):
                if mode == TIMING_HIST:
                    mj.tune_shard(r, hist_onepass=onepass)
                if mode == TIMING_FIXED:
                    mj.tune_shard(r, pipe_g=4)
            run_distinct_steps(mj, steps, output)
            for r in range(len(devices)):
                if mode == TIMING_FIXED:
                    assert mj.last_kernel(r) == "rx_lean_kernel", (r, mj.last_kernel(r))
                if mode == TIMING_HIST:
                    st = mj.hist_state(r)
                    if output == "data":
                        assert st == [-1] * 5, (r, st)      # a data call neither reads nor updates the guess: no books at all
                    else:
                        assert st[1] == 0, (r, onepass, st)      # the miss count is back at 0 behind the last step
                        if onepass == 1:
                            assert "one pass" in mj.last_kernel(r), (r, mj.last_kernel(r))
                        if onepass == 0:
                            assert "one pass" not in mj.last_kernel(r), (r, mj.last_kernel(r))
        finally:
            mj.close()


# ---------------------------------------------------------------------------- 2. degenerate shardings and reloads
@pytest.mark.parametrize("total", [1, 2, 3])
def test_fewer_frames_than_shards(clean, total):
    """three shards, one to three frames: the [r F / N, (r + 1) F / N) split with its empty shards, the oracle's rows in both slots"""
    x, want = clean
    w = {k: v[:total] for k, v in want.items()}
    mj = job([0, 0, 0], 1024, TIMING_FIXED)
    mj.load(x[:total])
    for r in range(3):
        sh = mj.shard(r)
        assert (sh["first"], sh["count"]) == (r * total // 3, (r + 1) * total // 3 - r * total // 3), (r, sh)
    outs = [mj.outputs(), mj.outputs()]
    mj.begin(0)
    mj.begin(1)
    mj.end(0, *outs[0])
    mj.end(1, *outs[1])
    for slot in (0, 1):
        assert_rows(outs[slot], w, "slot %d" % slot)
    mj.close()


def test_a_load_drops_the_step_in_flight(clean):
    """load(A); begin(0); load(B) with another frame count: the load waits for the step and drops it -- end(0) has nothing to end, and
    the next step is B's"""
    import qpsk_amd
    x, want = clean
    a, b = x[:77], x[20:60]
    wb = {k: v[20:60] for k, v in want.items()}
    mj = job([0, 0], 1024, TIMING_FIXED)
    mj.load(a)
    mj.begin(0)
    mj.load(b)
    assert (mj.shard(0)["count"], mj.shard(1)["first"], mj.shard(1)["count"]) == (20, 20, 20)
    with pytest.raises(qpsk_amd.QpskError, match="error %d: .*nothing in flight" % QPSK_ERR_STATE):
        mj.end(0)
    one_step(mj, 0, wb, "B in slot 0")
    one_step(mj, 1, wb, "B in slot 1")
    mj.close()


# ---------------------------------------------------------------------------- 3. the verdict reaches every slot it may belong to
@pytest.mark.parametrize("code,err", [(2, QPSK_ERR_RANGE), (1, QPSK_ERR_HIP)])
def test_a_status_with_both_slots_in_flight_fails_both(clean, code, err):
    """a kernel status on shard 1's context while slots 0 and 1 are in flight: the status word does not say whose it is, so BOTH ends
    fail, with the same code and text (before the per-slot rule the first end() took the flag and the second returned QPSK_OK);
    once both have ended nothing is left behind"""
    import torch
    import qpsk_amd
    x, want = clean
    mj = job([0, 0], 1024, TIMING_FIXED)
    mj.load(x)
    out = mj.outputs()
    mj.begin(0)
    mj.begin(1)
    torch.cuda.synchronize()
    mj.inject_status(1, code)
    with pytest.raises(qpsk_amd.QpskError) as e0:
        mj.end(0, *out)
    assert str(e0.value).startswith("libqpsk_hip error %d: device 0: " % err), str(e0.value)
    with pytest.raises(qpsk_amd.QpskError) as e1:
        mj.end(1, *out)
    assert str(e1.value) == str(e0.value)
    for slot in (0, 1, 1, 0):
        one_step(mj, slot, want, "slot %d after the failed ends" % slot)
    mj.close()


def test_a_status_with_one_slot_in_flight_fails_that_slot_only(clean):
    import qpsk_amd
    x, want = clean
    mj = job([0, 0], 1024, TIMING_FIXED)
    mj.load(x)
    mj.begin(0)
    mj.inject_status(1, 2)
    with pytest.raises(qpsk_amd.QpskError, match="error %d: device 0: " % QPSK_ERR_RANGE):
        mj.end(0, *mj.outputs())
    one_step(mj, 1, want, "slot 1 behind the failed slot 0")
    one_step(mj, 0, want, "slot 0 again")
    mj.close()


def test_a_persistently_bad_input_fails_every_step(clean):
    """one NaN sample in a frame of shard 1 (the fence of test_nonfinite_input_is_an_error: the kernel returns and flags its results),
    six steps in the advertised schedule: EVERY end() fails with QPSK_ERR_RANGE, not the irregular ones that happen to find the flag
    still there; a load of the clean batch then runs clean"""
    import qpsk_amd
    x, want = clean
    xb = x.copy()
    xb[50, 300, 0] = np.float32("nan")
    mj = job([0, 0], 1024, TIMING_FIXED)
    mj.load(xb)
    assert mj.shard(1)["first"] <= 50
    out = mj.outputs()
    failed = []

    def end(k):
        try:
            mj.end(k & 1, *out)
            failed.append((k, None))
        except qpsk_amd.QpskError as e:
            failed.append((k, str(e)))

    mj.begin(0)
    for k in range(1, 6):
        mj.begin(k & 1)
        end(k - 1)
    end(5)
    assert [k for k, _ in failed] == list(range(6))
    for k, text in failed:
        assert text is not None and text.startswith("libqpsk_hip error %d: device 0: " % QPSK_ERR_RANGE), (k, text)
    mj.load(x)
    one_step(mj, 0, want, "the clean batch behind the bad one")
    mj.close()


# ---------------------------------------------------------------------------- 4. a failed begin() leaves the slot free on every shard
REFUSED = dict(pipe_layout_lo=0x2, pipe_g=8, pipe_v=2)      # two units on one wave for eight frames per workgroup: rx_route refuses, nothing is launched


def test_a_begin_that_fails_on_one_shard_disarms_the_others(clean):
    """the middle one of three shards refuses its geometry (QPSK_ERR_ARG before any launch) while the other slot is in flight: begin(0)
    returns that error, shards 0 and 2 -- which did enqueue -- are waited for and disarmed, end(0) has nothing in flight, a second failing
    begin(0) is again refused for ITS reason (not 'still in flight'), and with the tuning cleared the slot works; the other slot ends
    with the oracle's rows"""
    import torch
    import qpsk_amd
    x, want = clean
    # first: this combination is refused by a plain context at shard 1's shape
    m = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=1024, timing_mode=TIMING_FIXED, fixed_index=FIXED_INDEX)
    m.tune(**REFUSED)
    with pytest.raises(qpsk_amd.QpskError, match="error %d: .*do not match 8 frames per workgroup" % QPSK_ERR_ARG):
        m.rx_batch(torch.from_numpy(x[25:51]).cuda())
    m.close()

    mj = job([0, 0, 0], 1024, TIMING_FIXED)
    mj.load(x)
    assert (mj.shard(1)["first"], mj.shard(1)["count"]) == (25, 26)
    other = mj.outputs()
    mj.begin(1)
    mj.tune_shard(1, **REFUSED)
    for attempt in (0, 1):
        with pytest.raises(qpsk_amd.QpskError, match="error %d: device 0: .*do not match 8 frames per workgroup" % QPSK_ERR_ARG):
            mj.begin(0)
        with pytest.raises(qpsk_amd.QpskError, match="error %d: .*nothing in flight in slot 0" % QPSK_ERR_STATE):
            mj.end(0)
    with pytest.raises(qpsk_amd.QpskError, match="do not match"):
        mj.begin(0)
    mj.tune_shard(1, **{k: None for k in REFUSED})
    one_step(mj, 0, want, "slot 0 with the tuning cleared")      # straight after a failed begin(0): no end(0) in between
    mj.end(1, *other)
    assert_rows(other, want, "slot 1, in flight all along")
    one_step(mj, 1, want, "slot 1 again")
    mj.close()


# ---------------------------------------------------------------------------- 5. the caller's device
def test_the_callers_device_is_left_alone(clean):
    """create, load, use_device_input and set_acquisition select the shard's device on the CALLER's thread: they put the caller's back"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices: a job on the last one, the caller on device 0")
    x, want = clean
    last = torch.cuda.device_count() - 1
    torch.cuda.set_device(0)
    mj = job([last], 1024, TIMING_FIXED)
    assert torch.cuda.current_device() == 0
    mj.load(x)
    assert torch.cuda.current_device() == 0
    lent = torch.from_numpy(x).to("cuda:%d" % last)
    mj.use_device_input(0, lent)
    assert torch.cuda.current_device() == 0
    mj.set_acquisition(np.full(len(x), FIXED_INDEX, np.int32), None)
    assert torch.cuda.current_device() == 0
    one_step(mj, 0, want, "the job on device %d" % last)
    mj.close()
    assert torch.cuda.current_device() == 0
