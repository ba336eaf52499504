"""What the Reed-Solomon decoder's GPU tests cannot show on a device, shown on the scalar port of rs_decode_kernel and rs_encode_kernel
(rs_port.py) -- no GPU needed.

The port is run over every row test_rs_gpu.py decodes and encodes (test_rs_cpu.case / encoder_rows, rs_rows.directed_rows / edge_rows: the
GPU tests build their inputs with the same functions):

 1. it equals rs_decode_ref and rs_encode_ref in every output byte and all four info words, with the flags and without, so it stands for
    the kernels;
 2. no index leaves exp[], row[], syn[], lam[] or om[] -- on the device an overrun reads a neighbour's bytes and fails nothing;
 3. every seeded fault of rs_port.FAULTS and ENCODE_FAULTS changes an output or leaves a table on at least one set: the inputs are
    adequate.  A change to the kernels is repeated in the port and has to keep this file green;
 4. the faults that survive the 480 rows the suite had before the directed rows and the edge codes are held to survive them
    (SURVIVED_BEFORE): that is what the new rows are for;
 5. taking out any of the early exits between Berlekamp-Massey and the verdict changes no output of any row, as rs.hip's header says,
    and neither does any of the four changes rs_port.EQUIVALENT lists with the reason why none can;
 6. the port's LDS starts as other random bytes and the results are the same.
"""
import numpy as np
import pytest

from rs_port import BOUNDS, ENCODE_FAULTS, EQUIVALENT, EVENTS, EXITS, FAULTS, REMOVALS, generator, rs_port
from rs_rows import directed_codes, directed_have, directed_rows, edge_codes, edge_rows
from test_rs_cpu import RS_CODES, case, codebook_decode, encoder_rows, rs_decode_ref, rs_encode_ref, rs_generator_ref

_SETS, _BASE = {}, {}


def decode_sets(new=True):
    """[(what, n, k, dict(words, flags, erased, plain))]: the 20 patterns of every code of RS_CODES, and with new=True the directed rows and
    the edge codes' rows behind them"""
    if not _SETS:
        _SETS[False] = [("patterns of (%d, %d)" % c, c[0], c[1], case(*c)) for c in RS_CODES]
        _SETS[True] = (_SETS[False] + [("directed rows of (%d, %d)" % c, c[0], c[1], directed_rows(*c)) for c in directed_codes()] +
                       [("edge rows of (%d, %d)" % c, c[0], c[1], edge_rows(*c)) for c in edge_codes()])
    return _SETS[new]


def encode_sets(new=True):
    """[(what, n, k, data)]: the encoder test's blocks of 1 and 5 rows (its 70 are more of the same to a port that takes a row at a time),
    and with new=True the 5 rows of every edge code"""
    old = [("encoder rows of (%d, %d), R = %d" % (n, k, R), n, k, data) for n, k in RS_CODES for R, data in encoder_rows(n, k, (1, 5))]
    return old + ([("encoder rows of (%d, %d), R = 5" % (n, k), n, k, encoder_rows(n, k, (5,))[0][1]) for n, k in edge_codes()] if new else [])


def modes(c):
    return (("flags", c["flags"], c["erased"]), ("d_erase NULL", None, c["plain"]))


def differs(got, want):
    """None, or the first row whose bytes or info differ"""
    for i in range(len(want[0])):
        if not np.array_equal(got[1][i], want[1][i]):
            return "info of row %d: %s, the reference has %s" % (i, got[1][i].tolist(), want[1][i].tolist())
        if not np.array_equal(got[0][i], want[0][i]):
            return "bytes of row %d" % i
    return None


def baseline():
    """the unfaulted port over every set, once: {(what, mode): traces}; asserts 1. and 2. on the way"""
    if not _BASE:
        for what, n, k, c in decode_sets():
            for mode, fl, want in modes(c):
                port = rs_port()
                got = port.decode(c["words"], n - k, fl)
                assert differs(got, want) is None, (what, mode, differs(got, want))
                assert port.over_bounds() is None, (what, mode, port.over_bounds())
                _BASE[(what, mode)] = (port.traces, dict(port.hi))
    return _BASE


# ------------------------------------------------------------------------------------------ 1., 2. the port stands for the kernels
def test_the_port_equals_the_references_on_every_row_and_no_index_leaves_its_table():
    base = baseline()
    exits, events, hi = dict.fromkeys(EXITS, 0), dict.fromkeys(EVENTS, 0), dict.fromkeys(BOUNDS, -1)
    for traces, h in base.values():
        for t in traces:
            exits[t["exit"]] += 1
            for ev in t["events"]:
                events[ev] += 1
        hi = {name: max(hi[name], h[name]) for name in hi}
    old = [t for (what, _), (traces, _) in base.items() if what.startswith("patterns") for t in traces]
    print("of the %d rows of the patterns alone, %d decode with corrections; events among those:" % (len(old), sum(t["exit"] == "decoded" for t in old)),
          {ev: sum(t["exit"] == "decoded" and ev in t["events"] for t in old) for ev in EVENTS},
          "; left by the second syndromes:", sum(t["exit"] == "second syndromes" for t in old))
    print("rows per exit:", exits)
    print("rows per event:", events)
    print("highest index used:", hi, "of", BOUNDS)
    assert all(exits.values()) and all(events.values())
    # the rows press on the tables: the staged row's last byte, the last syndrome, Lambda_64 (f = nroots = 64) and exp[] to within a few entries
    assert hi["row"] == 255 and hi["syn"] == 63 and hi["om"] == 63 and hi["lam"] == 64 and hi["exp"] >= 505
    for what, n, k, data in encode_sets():
        port = rs_port()
        assert np.array_equal(port.encode(data, n - k), rs_encode_ref(data, n - k)), what
        assert port.over_bounds() is None, (what, port.over_bounds())


def test_the_directed_rows_hold_the_events_they_were_chosen_for():
    """rs_rows asserts its own caps when it builds; here they are printed, and the search's yield is on record"""
    have = directed_have()
    for tag in sorted(have):
        print("%3d  %s" % (have[tag], tag))
    assert sum(len(directed_rows(*c)["words"]) for c in directed_codes()) <= 400


def test_the_port_s_tables_and_generator_are_the_reference_s():
    for nroots in range(1, 65):
        g = generator(nroots)
        assert g == rs_generator_ref(nroots).tolist()
        assert all(g), nroots                                                       # EQUIVALENT["gnz ignored"] rests on this


# ------------------------------------------------------------------------------------------ 3., 4. the seeded faults
def killed_by(fault, new=True):
    """the first set on which a fault shows, and how; None where it survives them all"""
    if fault in ENCODE_FAULTS or fault in ("lane < nroots dropped from gn", "gnz ignored"):
        for what, n, k, data in encode_sets(new):
            port = rs_port(fault=fault)
            if not np.array_equal(port.encode(data, n - k), rs_encode_ref(data, n - k)) or port.over_bounds():
                return what, port.over_bounds() or "parity"
        return None
    for what, n, k, c in decode_sets(new):
        for mode, fl, want in modes(c):
            port = rs_port(fault=fault)
            d = differs(port.decode(c["words"], n - k, fl), want) or port.over_bounds()
            if d:
                return what, mode, d
    return None


@pytest.mark.parametrize("fault", FAULTS + ENCODE_FAULTS)
def test_every_seeded_fault_shows_on_the_rows_the_gpu_tests_decode(fault):
    found = killed_by(fault)
    print(fault, "->", found)
    assert found is not None, "%r changes no output of any set: the GPU tests would pass a kernel with it" % fault


SURVIVED_BEFORE = ("len forgets f", "no second syndromes", "the clean exit taken before the f > nroots test")


@pytest.mark.parametrize("fault", SURVIVED_BEFORE)
def test_the_faults_the_new_rows_are_for_survive_without_them(fault):
    assert killed_by(fault, new=False) is None


# ------------------------------------------------------------------------------------------ 5. what may change nothing
def rows_where(pick):
    """every set cut down to the rows whose unfaulted trace passes `pick`: a row that never reaches the changed line cannot differ"""
    base = baseline()
    for what, n, k, c in decode_sets():
        for mode, fl, want in modes(c):
            at = [i for i, t in enumerate(base[(what, mode)][0]) if pick(t)]
            if at:
                yield what, mode, n, k, c["words"][at], None if fl is None else fl[at], (want[0][at], want[1][at])


@pytest.mark.parametrize("remove", REMOVALS)
def test_nothing_rests_on_an_early_exit(remove):
    """every row on which the removed check fired, decoded without it: the later checks stop the row all the same"""
    seen = 0
    for what, mode, n, k, words, fl, want in rows_where(lambda t: t["exit"] == remove or remove in t["fired"]):
        port = rs_port(remove=remove)
        got = port.decode(words, n - k, fl)
        assert differs(got, want) is None, (remove, what, mode, differs(got, want))
        assert port.over_bounds() is None, (remove, what, mode, port.over_bounds())
        assert all(t["exit"] != remove for t in port.traces)
        seen += len(words)
    print(remove, "removed on", seen, "rows")
    assert seen >= 4


@pytest.mark.parametrize("n,k", [(6, 2), (10, 4), (34, 32)])
def test_nothing_rests_on_an_early_exit_on_random_words_either(n, k):
    """the property on words nobody chose: 150 random words with random flags per code, most of them far from any codeword"""
    rng = np.random.default_rng([n, k, 3])
    words = rng.integers(0, 256, (150, n), dtype=np.uint8)
    flags = (rng.random((150, n)) < rng.random((150, 1)) * (n - k + 1) / n).astype(np.uint8)
    want = rs_decode_ref(words, n - k, flags)
    fired = set()
    for remove in (None,) + REMOVALS:
        port = rs_port(remove=remove)
        assert differs(port.decode(words, n - k, flags), want) is None, (remove, differs(port.decode(words, n - k, flags), want))
        fired |= {name for t in port.traces for name in t["fired"]} | {t["exit"] for t in port.traces}
    assert "roots != deg" in fired                                              # where nearly every random word ends


def test_the_words_the_second_syndromes_alone_reject_against_the_codebook():
    """two words of the small codes that pass every check before the last (found by random search: about 1 damaged word in 2000 to 3000
    is one): the port leaves by the second syndromes, and the codebook -- every codeword of the code, enumerated -- says no codeword
    lies within the radius, so failing them is right and a decoder without the last check would hand out a non-codeword"""
    for n, k, word, flags in ((6, 2, [212, 240, 140, 110, 229, 193], [1, 1, 0, 0, 0, 0]), (8, 2, [153, 150, 33, 67, 88, 217, 119, 22], [0, 0, 1, 1, 1, 0, 1, 0])):
        word, flags = np.array(word, np.uint8), np.array(flags, np.uint8)
        port = rs_port()
        out, info = port.decode(word, n - k, flags)
        assert port.traces[0]["exit"] == "second syndromes" and port.traces[0]["fired"] == ()
        c, want = codebook_decode(word, flags, n, k)
        assert want[0] == -1 and tuple(info[0]) == want and np.array_equal(out[0], word)
        out, info = rs_port(fault="no second syndromes").decode(word, n - k, flags)
        assert info[0, 0] >= 0 and rs_decode_ref(out, n - k)[1][0, 3] == 0      # what it would hand out is no codeword


@pytest.mark.parametrize("change", sorted(EQUIVALENT))
def test_the_changes_left_out_of_the_fault_list_change_nothing(change):
    if change in ("lane < nroots dropped from gn", "gnz ignored"):
        assert killed_by(change) is None
        return
    reached = 0
    for what, mode, n, k, words, fl, want in rows_where(lambda t: t["deg"] is not None):
        if change == "chunk skip 64 c > n" and n % 64:
            continue
        port = rs_port(fault=change)
        assert differs(port.decode(words, n - k, fl), want) is None and port.over_bounds() is None, (change, what, mode)
        reached += len(words)
    assert reached >= 100


# ------------------------------------------------------------------------------------------ 6. the LDS a launch finds
def test_no_byte_the_staging_did_not_write_reaches_an_output():
    """other random bytes in the LDS, the rows of every set in another order (so each meets another wave's slice): the same results"""
    for what, n, k, c in decode_sets():
        order = np.roll(np.arange(len(c["words"])), 1)
        for mode, fl, want in modes(c):
            port = rs_port(seed=1)
            got = port.decode(c["words"][order], n - k, None if fl is None else fl[order])
            assert differs(got, (want[0][order], want[1][order])) is None, (what, mode)
