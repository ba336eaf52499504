"""ctypes binding of libqpsk_hip.so (include/qpsk_hip.h) for tests and bench.py.

Device buffers are torch tensors on the context's GPU; only their data_ptr() crosses the C ABI.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TAU = 2.0 * 3.14159265358979323846
TIMING_HIST, TIMING_FIXED, TIMING_FFT = 0, 1, 2
OUTER_POLARITY, OUTER_MSB_FIRST = 1, 2      # qpsk_outer_reset's flags
DISPERSAL_MSB_FIRST = 1                     # qpsk_dispersal_batch's
NTAPS = 127


class QpskError(RuntimeError):
    pass


class Params(C.Structure):
    """qpsk_params of include/qpsk_hip.h (the reference's #defines and main() literals)."""
    _fields_ = [("fs", C.c_double), ("rs", C.c_double), ("frame_size", C.c_int), ("rrc_alpha", C.c_float),
                ("loop_bw", C.c_float), ("min_freq", C.c_float), ("max_freq", C.c_float),
                ("timing_mode", C.c_int), ("fixed_index", C.c_int)]


def lib_path():
    """The built library; QPSK_HIP_LIB names another build of it (A/B timing of two source versions on one box)."""
    return os.environ.get("QPSK_HIP_LIB") or os.path.join(HERE, "libqpsk_hip.so")


def build(verbose=False):
    """Compile qpsk_amd/csrc for gfx950 into qpsk_amd/libqpsk_hip.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return lib_path()


_LIB = None

# every symbol include/qpsk_hip.h declares (tests check that the library exports all of them)
API_SYMBOLS = [
    "qpsk_last_error", "qpsk_version", "qpsk_device_count", "qpsk_params_default", "qpsk_ctx_create",
    "qpsk_ctx_destroy", "qpsk_ctx_sync", "qpsk_ctx_set_stream", "qpsk_ctx_set_tuning", "qpsk_ctx_cycles", "qpsk_ctx_nsym",
    "qpsk_ctx_last_kernel",
    "qpsk_ctx_get_taps", "qpsk_ctx_get_gains", "qpsk_ctx_set_taps", "qpsk_ctx_set_loop", "qpsk_rx_batch", "qpsk_rx_batch_pitched",
    "qpsk_rx_batch_bw", "qpsk_rrc_fir_batch", "qpsk_rrc_fir_batch_fast", "qpsk_timing_hist_batch", "qpsk_timing_scan_batch", "qpsk_timing_fft_batch", "qpsk_timing_fft_bin_batch", "qpsk_costas_batch", "qpsk_fft_batch",
    "qpsk_streams_reset", "qpsk_streams_set_loop_state", "qpsk_streams_get_loop_state", "qpsk_streams_rx_cplx",
    "qpsk_streams_rx_pcm", "qpsk_streams_rx_pcm_host", "qpsk_dev_alloc", "qpsk_dev_free", "qpsk_dev_upload", "qpsk_dev_download",
    "qpsk_selftest_sincos_hash", "qpsk_crc16_batch", "qpsk_interleave_batch", "qpsk_scramble_batch",
    "qpsk_tx_reset", "qpsk_tx_symbols", "qpsk_test_inject_status", "qpsk_test_hist_state", "qpsk_ctx_check",
    "qpsk_multi_create", "qpsk_multi_destroy", "qpsk_multi_shards", "qpsk_multi_load", "qpsk_multi_shard", "qpsk_multi_use_device_input",
    "qpsk_multi_rx_begin", "qpsk_multi_rx_end", "qpsk_multi_set_direct_output", "qpsk_host_alloc", "qpsk_host_free",
    "qpsk_multi_set_packed", "qpsk_pack_symbols", "qpsk_unpack_symbols_host",
    "qpsk_rx_batch_ext", "qpsk_rx_batch_bw_ext", "qpsk_multi_set_acquisition", "qpsk_carrier_est_batch",
    "qpsk_rx_batch_data", "qpsk_sync_batch", "qpsk_multi_set_data", "qpsk_deframer_reset", "qpsk_deframer_push",
    "qpsk_deframer_reset_coded", "qpsk_deframer_push_coded",
    "qpsk_soft_batch", "qpsk_conv_encode_batch", "qpsk_viterbi_batch",
    "qpsk_punct_ntx", "qpsk_conv_encode_punct_batch", "qpsk_viterbi_punct_batch", "qpsk_deframer_reset_coded_punct",
    "qpsk_test_viterbi_launches", "qpsk_test_deframer_advance", "qpsk_test_fir_runs",
    "qpsk_frame_len", "qpsk_frame_batch",
    "qpsk_ilv_stride", "qpsk_conv_encode_ilv_batch", "qpsk_viterbi_ilv_batch", "qpsk_frame_batch_ilv", "qpsk_deframer_reset_coded_ilv",
    "qpsk_rs_generator", "qpsk_rs_encode_batch", "qpsk_rs_decode_batch",
    "qpsk_rs_cross_encode_batch", "qpsk_rs_cross_decode_batch", "qpsk_rs_cross_place_batch",
    "qpsk_viterbi_stream_reset", "qpsk_viterbi_stream_emits", "qpsk_viterbi_stream_push", "qpsk_viterbi_stream_flush",
    "qpsk_conv_encode_stream_batch", "qpsk_test_viterbi_stream_advance",
    "qpsk_outer_reset", "qpsk_outer_max_words", "qpsk_outer_push", "qpsk_outer_interleave_batch", "qpsk_test_outer_advance",
    "qpsk_nodesync_reset", "qpsk_nodesync_shifts", "qpsk_nodesync_push", "qpsk_nodesync_set",
    "qpsk_outer_reset_group", "qpsk_dispersal_batch", "qpsk_dispersal_sequence",
    "qpsk_channel_twiddles", "qpsk_channel_reset", "qpsk_channel_push", "qpsk_synth_reset", "qpsk_synth_push",
    "qpsk_resample_reset", "qpsk_resample_need", "qpsk_resample_push",
]
# the named puncturing patterns of include/qpsk_hip.h (QPSK_PUNCT_*): rate -> (period, keep0, keep1), bit r of a mask = step r of the period
PUNCTURE = {"1/2": (1, 0x1, 0x1), "2/3": (2, 0x1, 0x3), "3/4": (3, 0x5, 0x3), "5/6": (5, 0x15, 0x0B), "7/8": (7, 0x51, 0x2F)}


def _pattern(puncture):
    """a key of PUNCTURE or a (period, keep0, keep1) tuple -> the three ints (the library checks them)"""
    if isinstance(puncture, str):
        if puncture not in PUNCTURE:
            raise ValueError("puncture must be one of %s or a (period, keep0, keep1) tuple" % sorted(PUNCTURE))
        puncture = PUNCTURE[puncture]
    period, keep0, keep1 = puncture
    return int(period), int(keep0), int(keep1)
# every symbol include/qpsk_dropin.h declares
DROPIN_SYMBOLS = [
    "qpsk_dropin_configure", "qpsk_dropin_set_device", "qpsk_dropin_shutdown", "rrc_fir", "rrc_make",
    "create_control_loop", "phase_detector", "update_gains", "advance_loop", "phase_wrap", "frequency_limit",
    "set_loop_bandwidth", "set_damping_factor", "set_alpha", "set_beta", "set_frequency", "set_phase",
    "set_max_freq", "set_min_freq", "get_loop_bandwidth", "get_damping_factor", "get_alpha", "get_beta",
    "get_frequency", "get_phase", "get_max_freq", "get_min_freq", "fft", "fftn", "ifft", "ifftn", "qpsk_demod",
    "rx_frame", "qpsk_dropin_costas_frame", "qpsk_dropin_symbols", "qpsk_dropin_offset_freq",
    "qpsk_dropin_timing_index",
]


def load():
    """Load the library; raises QpskError if it has not been built (no fallback of any kind)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise QpskError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback)" % p)
    # PyTorch ships its own libamdhip64; whichever HIP runtime is loaded first serves the whole process, and
    # torch.cuda stops working if the system one got in before it.  This plumbing always shares the process with
    # torch (device buffers are torch tensors), so let torch load its runtime first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(p)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.qpsk_last_error.restype = C.c_char_p
    L.qpsk_version.restype = C.c_char_p
    L.qpsk_params_default.argtypes = [C.POINTER(Params)]
    L.qpsk_ctx_create.argtypes = [C.POINTER(vp), i32, C.POINTER(Params), vp]
    L.qpsk_ctx_destroy.argtypes = [vp]
    L.qpsk_ctx_destroy.restype = None
    L.qpsk_ctx_sync.argtypes = [vp]
    L.qpsk_ctx_set_stream.argtypes = [vp, vp]
    L.qpsk_ctx_set_tuning.argtypes = [vp, C.c_char_p, i32]
    L.qpsk_ctx_cycles.argtypes = [vp]
    L.qpsk_ctx_nsym.argtypes = [vp]
    L.qpsk_ctx_last_kernel.argtypes = [vp]
    L.qpsk_ctx_last_kernel.restype = C.c_char_p
    L.qpsk_ctx_get_taps.argtypes = [vp, C.POINTER(f32)]
    L.qpsk_ctx_get_gains.argtypes = [vp, C.POINTER(f32), C.POINTER(f32)]
    L.qpsk_ctx_set_taps.argtypes = [vp, C.POINTER(f32)]
    L.qpsk_ctx_set_loop.argtypes = [vp, f32, f32, f32, f32]
    L.qpsk_rx_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.qpsk_rx_batch_pitched.argtypes = [vp, vp, C.c_longlong, i32, vp, vp, vp, vp, vp, vp]
    L.qpsk_rx_batch_bw.argtypes = [vp, vp, i32, C.POINTER(f32), i32, vp, vp, vp, vp]
    L.qpsk_rx_batch_ext.argtypes = [vp, vp, C.c_longlong, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.qpsk_rx_batch_bw_ext.argtypes = [vp, vp, i32, C.POINTER(f32), i32, vp, vp, vp, vp, vp, vp]
    L.qpsk_multi_set_acquisition.argtypes = [vp, vp, vp]
    L.qpsk_carrier_est_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, vp, vp, vp, vp]
    L.qpsk_rx_batch_data.argtypes = [vp, vp, C.c_longlong, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.qpsk_sync_batch.argtypes = [vp, vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.qpsk_multi_set_data.argtypes = [vp, i32]
    L.qpsk_deframer_reset.argtypes = [vp, i32, vp, i32, i32, i32, i32]
    L.qpsk_deframer_push.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.qpsk_deframer_reset_coded.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, f32]
    L.qpsk_deframer_push_coded.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.qpsk_soft_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, i32, f32, vp, vp, vp, i32, i32, vp, vp, vp]
    L.qpsk_conv_encode_batch.argtypes = [vp, vp, i32, i32, i32, vp]
    L.qpsk_viterbi_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, vp, i32, vp, vp]
    u32 = C.c_uint32
    L.qpsk_punct_ntx.argtypes = [i32, i32, u32, u32]
    L.qpsk_conv_encode_punct_batch.argtypes = [vp, vp, i32, i32, i32, i32, u32, u32, vp]
    L.qpsk_viterbi_punct_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, u32, u32, vp, i32, vp, vp]
    L.qpsk_deframer_reset_coded_punct.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, f32, i32, u32, u32]
    L.qpsk_frame_len.argtypes = [i32, i32, i32, i32, u32, u32]
    L.qpsk_frame_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, vp, i32, i32, i32, u32, u32, i32, i32, i32, vp, vp]
    L.qpsk_ilv_stride.argtypes = [i32, i32]
    L.qpsk_conv_encode_ilv_batch.argtypes = [vp, vp, i32, i32, i32, i32, u32, u32, i32, vp]
    L.qpsk_viterbi_ilv_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, u32, u32, i32, vp, i32, vp, vp]
    L.qpsk_frame_batch_ilv.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, vp, i32, i32, i32, u32, u32, i32, i32, i32, i32, vp, vp]
    L.qpsk_deframer_reset_coded_ilv.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, f32, i32, u32, u32, i32]
    L.qpsk_rs_generator.argtypes = [i32, vp]
    L.qpsk_rs_encode_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, vp, C.c_longlong]
    L.qpsk_rs_decode_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, vp, vp, C.c_longlong, vp]
    L.qpsk_rs_cross_encode_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, i32, i32]
    L.qpsk_rs_cross_decode_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, i32, i32, vp, vp, C.c_longlong, vp, vp]
    L.qpsk_rs_cross_place_batch.argtypes = [vp, vp, C.c_longlong, vp, vp, i32, i32, i32, i32, i32, vp, vp, C.c_longlong, vp]
    L.qpsk_rrc_fir_batch.argtypes = [vp, vp, vp, vp, i32, i32]
    L.qpsk_rrc_fir_batch_fast.argtypes = [vp, vp, vp, vp, i32, i32]
    L.qpsk_timing_hist_batch.argtypes = [vp, vp, i32, vp, vp]
    L.qpsk_timing_fft_batch.argtypes = [vp, vp, i32, vp, vp, vp]
    L.qpsk_timing_fft_bin_batch.argtypes = [vp, vp, i32, vp, vp, vp]
    L.qpsk_timing_scan_batch.argtypes = [vp, vp, i32, vp, vp]
    L.qpsk_costas_batch.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.qpsk_fft_batch.argtypes = [vp, vp, vp, i32, i32, i32]
    L.qpsk_streams_reset.argtypes = [vp, i32, C.c_double]
    L.qpsk_streams_set_loop_state.argtypes = [vp, C.POINTER(f32)]
    L.qpsk_streams_get_loop_state.argtypes = [vp, C.POINTER(f32)]
    L.qpsk_streams_rx_cplx.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.qpsk_streams_rx_pcm.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.qpsk_streams_rx_pcm_host.argtypes = [vp, vp, vp, vp, vp, vp]
    L.qpsk_selftest_sincos_hash.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_ulonglong)]
    L.qpsk_test_inject_status.argtypes = [vp, i32]
    L.qpsk_ctx_check.argtypes = [vp]
    L.qpsk_test_hist_state.argtypes = [vp, C.POINTER(i32)]
    L.qpsk_test_viterbi_launches.argtypes = [vp, C.POINTER(i32)]
    L.qpsk_test_deframer_advance.argtypes = [vp, C.c_longlong]
    L.qpsk_viterbi_stream_reset.argtypes = [vp, i32, i32, i32, i32, u32, u32]
    L.qpsk_viterbi_stream_emits.argtypes = [vp, i32]
    L.qpsk_viterbi_stream_push.argtypes = [vp, vp, C.c_longlong, i32, vp, C.c_longlong, vp, C.POINTER(i32)]
    L.qpsk_viterbi_stream_flush.argtypes = [vp, i32, vp, C.c_longlong, vp, C.POINTER(i32)]
    L.qpsk_conv_encode_stream_batch.argtypes = [vp, vp, i32, i32, i32, u32, u32, vp, vp, vp]
    L.qpsk_test_viterbi_stream_advance.argtypes = [vp, C.c_longlong]
    L.qpsk_outer_reset.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32]
    L.qpsk_outer_reset_group.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32]
    L.qpsk_dispersal_batch.argtypes = [vp, vp, C.c_longlong, i32, i32, i32, i32, vp, i32, vp, C.c_longlong]
    L.qpsk_dispersal_sequence.argtypes = [i32, i32, i32, vp]
    L.qpsk_channel_twiddles.argtypes = [i32, vp]
    L.qpsk_channel_reset.argtypes = [vp, i32, i32, vp, vp, i32]
    L.qpsk_channel_push.argtypes = [vp, vp, i32, vp, C.c_longlong]
    L.qpsk_synth_reset.argtypes = [vp, i32, i32, vp, vp, i32]
    L.qpsk_synth_push.argtypes = [vp, vp, C.c_longlong, i32, vp]
    L.qpsk_resample_reset.argtypes = [vp, i32, i32, i32, i32, vp]
    L.qpsk_resample_need.argtypes = [vp, i32]
    L.qpsk_resample_push.argtypes = [vp, vp, C.c_longlong, i32, i32, vp, C.c_longlong]
    L.qpsk_outer_max_words.argtypes = [vp, i32]
    L.qpsk_outer_push.argtypes = [vp, vp, C.c_longlong, i32, i32, vp, vp, C.c_longlong, vp, vp, vp]
    L.qpsk_outer_interleave_batch.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.qpsk_test_outer_advance.argtypes = [vp, C.c_longlong]
    L.qpsk_nodesync_reset.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32]
    L.qpsk_nodesync_shifts.argtypes = [i32, u32, u32]
    L.qpsk_nodesync_push.argtypes = [vp, vp, C.c_longlong, i32, vp, vp, C.c_longlong, vp]
    L.qpsk_nodesync_set.argtypes = [vp, vp]
    L.qpsk_test_fir_runs.argtypes = [vp, i32, i32, C.POINTER(i32)]
    L.qpsk_multi_create.argtypes = [C.POINTER(vp), C.POINTER(i32), i32, C.POINTER(Params)]
    L.qpsk_multi_destroy.argtypes = [vp]
    L.qpsk_multi_destroy.restype = None
    L.qpsk_multi_shards.argtypes = [vp]
    L.qpsk_multi_load.argtypes = [vp, C.c_longlong, vp]
    L.qpsk_multi_shard.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(vp), C.POINTER(vp)]
    L.qpsk_multi_use_device_input.argtypes = [vp, i32, vp]
    L.qpsk_multi_set_direct_output.argtypes = [vp, i32, vp, vp, vp]
    L.qpsk_multi_set_packed.argtypes = [vp, i32]
    L.qpsk_pack_symbols.argtypes = [vp, vp, C.c_longlong, i32, vp]
    L.qpsk_unpack_symbols_host.argtypes = [vp, C.c_longlong, i32, vp]
    L.qpsk_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.qpsk_host_free.argtypes = [vp]
    L.qpsk_multi_rx_begin.argtypes = [vp, i32]
    L.qpsk_multi_rx_end.argtypes = [vp, i32, vp, vp, vp]
    L.qpsk_crc16_batch.argtypes = [vp, vp, i32, i32, vp]
    L.qpsk_interleave_batch.argtypes = [vp, vp, i32, i32, i32]
    L.qpsk_scramble_batch.argtypes = [vp, vp, i32, i32]
    L.qpsk_tx_reset.argtypes = [vp, i32, C.c_double]
    L.qpsk_tx_symbols.argtypes = [vp, vp, i32, vp, vp]
    _LIB = L
    return L


def version():
    """qpsk_version() of the loaded library"""
    return load().qpsk_version().decode()


FRAME_UNCODED, FRAME_CODED = 0, 1      # QPSK_FRAME_UNCODED, QPSK_FRAME_CODED


def _coding(coded, puncture):
    """frame()'s coded / puncture -> qpsk_frame_batch's (coding, period, keep0, keep1); coded with no pattern is rate 1/2"""
    if not coded:
        return (FRAME_UNCODED, 1, 1, 1)
    return (FRAME_CODED,) + _pattern("1/2" if puncture is None else puncture)


def frame_len(nsync, nbytes, coded=True, puncture=None):
    """qpsk_frame_len: the dibits of one packet on air, sync word and body, as Modem.frame() builds it (coded, puncture as there); host
    only, needs no GPU"""
    L = load()
    rc = L.qpsk_frame_len(int(nsync), int(nbytes), *_coding(coded, puncture))
    if rc < 0:
        raise QpskError("libqpsk_hip error %d: %s" % (rc, L.qpsk_last_error().decode()))
    return rc


def ilv_stride(nbits, want):
    """qpsk_ilv_stride: the smallest interleaver stride s >= min(want, nbits - 1) coprime to nbits, the bits of a body on air (2 ntx);
    ilv_stride(n, n // 16) is a starting point against bursts.  Host only, needs no GPU"""
    L = load()
    rc = L.qpsk_ilv_stride(int(nbits), int(want))
    if rc < 0:
        raise QpskError("libqpsk_hip error %d: %s" % (rc, L.qpsk_last_error().decode()))
    return rc


def rs_generator(nroots):
    """qpsk_rs_generator: the nroots + 1 coefficients of the Reed-Solomon generator polynomial prod (x - alpha^i), i < nroots, over GF(256)
    modulo 0x11D, highest first, as a numpy uint8 array.  Host only, needs no GPU"""
    L = load()
    g = np.zeros(max(int(nroots), 0) + 1, np.uint8)
    rc = L.qpsk_rs_generator(int(nroots), g.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise QpskError("libqpsk_hip error %d: %s" % (rc, L.qpsk_last_error().decode()))
    return g


def dispersal_sequence(len=188, group=8, msb_first=False):      # noqa: A002 (the header's name)
    """qpsk_dispersal_sequence: the group * len - 1 bytes PR of DVB's energy dispersal (DVB TRANSPORT in include/qpsk_hip.h), as bytes;
    msb_first: a byte's first bit is its bit 7 (DVB's order: 03 F6 08 34 ...).  Host only, needs no GPU"""
    L = load()
    out = np.zeros(max(int(group) * int(len), 1), np.uint8)
    rc = L.qpsk_dispersal_sequence(int(len), int(group), DISPERSAL_MSB_FIRST if msb_first else 0, out.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise QpskError("libqpsk_hip error %d: %s" % (rc, L.qpsk_last_error().decode()))
    return out[:rc].tobytes()


def channel_twiddles(M):
    """qpsk_channel_twiddles: the (M / 2, 2) float32 table (cos, sin)(TAU j / M) of the channeliser's transform (CHANNELISER in
    include/qpsk_hip.h), part of its definition.  Host only, needs no GPU"""
    L = load()
    tw = np.zeros((max(int(M) // 2, 1), 2), np.float32)
    rc = L.qpsk_channel_twiddles(int(M), tw.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise QpskError("libqpsk_hip error %d: %s" % (rc, L.qpsk_last_error().decode()))
    return tw


def _kaiser_sinc(n, spacing, beta):
    """The n float64 taps of a Kaiser-windowed sinc with its nulls `spacing` taps apart (cut-off 1 / (2 spacing) cycles per tap), centred
    and made symmetric bit for bit; unscaled: the *_prototype functions scale and round"""
    t = (np.arange(n) - (n - 1) / 2.0) / float(spacing)
    h = np.sinc(t) * np.kaiser(n, float(beta))
    return 0.5 * (h + h[::-1])


def channel_prototype(M, P, beta=8.0, gain=1.0):
    """A prototype for Modem.channel_reset(): the M P taps of a Kaiser-windowed sinc with its cut-off at half the channel spacing
    (1 / (2 M) cycles per wideband sample), symmetric, unit gain at DC, float32.  A numpy convenience: the library designs no filter, and
    any finite taps do.  gain multiplies the float32 taps: Modem.synth_reset() wants the interpolation gain M, and gain=M is exact in
    float32, M being a power of two -- the synthesis prototype is then M times the analysis one tap for tap"""
    h = _kaiser_sinc(int(M) * int(P), int(M), beta)
    return np.float32(gain) * (h / h.sum()).astype(np.float32)


def resample_prototype(L, D, P, beta=10.0, gain=None):
    """A prototype for Modem.resample_reset(): the L P taps of a Kaiser-windowed sinc with its cut-off at 1 / (2 max(L, D)) cycles per
    interpolated sample -- half the LOWER of the two rates, so neither the images of the interpolation nor the aliases of the decimation
    pass -- symmetric, float32, every tap rounded once, their sum equal to gain (default: the interpolation gain L).  A numpy convenience:
    the library designs no filter, and any finite taps do.  The transition band is the window's main lobe: the stop band begins
    sqrt(1 + (beta / pi)^2) / (L P) cycles per interpolated sample beyond the cut-off (the Kaiser window's first null; 3.34 / (L P) at
    beta = 10), the pass band ends as far below it, and the stop band lies about beta / 0.1102 + 8.7 dB down (Kaiser's rule: 99 dB)"""
    h = _kaiser_sinc(int(L) * int(P), max(int(L), int(D)), beta)
    return (h * (float(L if gain is None else gain) / h.sum())).astype(np.float32)


def nodesync_shifts(puncture):
    """qpsk_nodesync_shifts: the delays (in dibits) a node sync has to try for a pattern, a key of PUNCTURE or a (period, keep0, keep1)
    tuple: nodesync_reset()'s nshift.  Host only, needs no GPU"""
    L = load()
    rc = L.qpsk_nodesync_shifts(*_pattern(puncture))
    if rc < 0:
        raise QpskError("libqpsk_hip error %d: %s" % (rc, L.qpsk_last_error().decode()))
    return rc


def _interleaved(interleave):
    """interleave= of the Modem calls: None or 1 is off (the existing entry points are called), an integer stride takes the ilv ones"""
    return interleave is not None and int(interleave) != 1


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Modem:
    """One qpsk_ctx: a configuration (taps, loop gains) bound to one GPU and one HIP stream."""

    def __init__(self, fs=9600.0, rs=2400.0, frame_size=512, rrc_alpha=0.35, loop_bw=np.float32(TAU / 100.0),
                 min_freq=-1.0, max_freq=1.0, timing_mode=TIMING_HIST, fixed_index=0, device=None, stream="torch"):
        import torch
        self.torch = torch
        self.L = load()
        if not torch.cuda.is_available():
            raise QpskError("no GPU visible to torch; libqpsk_hip has no CPU path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.dev = torch.device("cuda", self.device)
        self.params = Params(fs, rs, frame_size, rrc_alpha, loop_bw, min_freq, max_freq, timing_mode, fixed_index)
        if stream == "torch":
            s = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        elif stream is None:
            s = None
        else:
            s = C.c_void_p(int(stream))
        h = C.c_void_p()
        self._check(self.L.qpsk_ctx_create(C.byref(h), self.device, C.byref(self.params), s))
        self.h = h
        self.cycles = self.L.qpsk_ctx_cycles(h)
        self.nsym = self.L.qpsk_ctx_nsym(h)
        self.frame_size = frame_size
        self.nstreams = 0
        self._vs_streams = 0      # streams of the streaming Viterbi decoder (viterbi_stream_reset)
        self._outer = None        # (streams, n) of the outer link (outer_reset)
        self._ns_links = 0        # links of the node sync (nodesync_reset)
        self._channel = None      # (M, nsel) of the channeliser (channel_reset)
        self._synth = None        # (M, nsel) of the synthesis bank (synth_reset)
        self._resample = 0        # streams of the resampler (resample_reset)

    def _check(self, rc):
        if rc != 0:
            raise QpskError("libqpsk_hip error %d: %s" % (rc, self.L.qpsk_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.qpsk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self, data=None, sync=None, lag_min=0, lag_max=0, nout=0):
        """No arguments: wait for the context's work (qpsk_ctx_sync) and report a kernel's verdict.  With data and a sync word: the
        sync-word search of qpsk_sync_batch (see _sync_search)."""
        if data is None:
            self._check(self.L.qpsk_ctx_sync(self.h))
            return None
        return self._sync_search(data, sync, lag_min, lag_max, nout)

    def last_kernel(self):
        """Name of the kernel the last rx_batch*() (or rrc_fir(), ...) call launched (which geometry served that shape)."""
        return self.L.qpsk_ctx_last_kernel(self.h).decode()

    def tune(self, **kw):
        """Kernel-geometry selection (tests, measurements): m.tune(pipe_nf=3, pipe_wide=0); None = library's choice.
        Keys are the QPSK_* names of qpsk_ctx_set_tuning() in lower case without the prefix."""
        for k, v in kw.items():
            self._check(self.L.qpsk_ctx_set_tuning(self.h, ("QPSK_" + k.upper()).encode(), -1 if v is None else int(v)))

    def viterbi_launches(self):
        """Test hook: decode launches of the last viterbi() / deframe_coded() call (qpsk_test_viterbi_launches)."""
        n = C.c_int(-1)
        self._check(self.L.qpsk_test_viterbi_launches(self.h, C.byref(n)))
        return n.value

    def deframer_advance(self, delta):
        """Test hook: move both deframers' stream positions on by delta dibits (qpsk_test_deframer_advance)."""
        self._check(self.L.qpsk_test_deframer_advance(self.h, int(delta)))

    def fir_runs(self, nframes, length):
        """Test hook: (ntiles, parts, tpp) -- the runs of 512-output tiles rrc_fir_stream_kernel cuts this batch into on this device
        (qpsk_test_fir_runs); nothing is launched."""
        out = (C.c_int * 3)()
        self._check(self.L.qpsk_test_fir_runs(self.h, int(nframes), int(length), out))
        return tuple(out)

    def set_stream(self, stream):
        """Enqueue this context's work on another HIP stream (a torch.cuda.Stream or a raw handle; None = default)."""
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        self._check(self.L.qpsk_ctx_set_stream(self.h, s))

    # ---- configuration
    @property
    def taps(self):
        t = (C.c_float * NTAPS)()
        self._check(self.L.qpsk_ctx_get_taps(self.h, t))
        return np.array(t, np.float32)

    @property
    def gains(self):
        a, b = C.c_float(), C.c_float()
        self._check(self.L.qpsk_ctx_get_gains(self.h, C.byref(a), C.byref(b)))
        return np.float32(a.value), np.float32(b.value)

    def set_taps(self, taps):
        t = (C.c_float * NTAPS)(*[float(x) for x in taps])
        self._check(self.L.qpsk_ctx_set_taps(self.h, t))

    def set_loop(self, alpha, beta, min_freq, max_freq):
        self._check(self.L.qpsk_ctx_set_loop(self.h, alpha, beta, min_freq, max_freq))

    # ---- helpers
    def _dev(self, a, dtype):
        t = self.torch
        if isinstance(a, np.ndarray):
            a = t.from_numpy(np.ascontiguousarray(a))
        a = a.to(self.dev)
        assert a.dtype == dtype, (a.dtype, dtype)
        return a.contiguous()

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.dev)

    # ---- the hot path
    def rx_batch(self, frames, want_costas=False, out=None):
        """frames: (F, frame_size, 2) float32 (numpy or torch).  Returns dict of torch tensors."""
        t = self.torch
        x = self._dev(frames, t.float32)
        F = x.shape[0]
        assert x.shape[1] == self.frame_size and x.shape[2] == 2
        o = out or dict(sym=self.empty((F, self.nsym), t.uint8), freq=self.empty((F,), t.float32),
                        phase=self.empty((F,), t.float32), index=self.empty((F,), t.int32),
                        hz=self.empty((F,), t.float32),
                        costas=self.empty((F, self.nsym, 2), t.float32) if want_costas else None)
        self._check(self.L.qpsk_rx_batch(self.h, _ptr(x), F, _ptr(o["sym"]), _ptr(o["freq"]), _ptr(o["phase"]),
                                         _ptr(o.get("costas")), _ptr(o.get("index")), _ptr(o.get("hz"))))
        return o

    def rx_batch_raw(self, x, F, sym, freq, phase, pitch=0, index=None):
        """No allocation, no checks: the call bench.py times.  pitch: complex samples between frame starts (0 = packed);
        index: optional (F,) int32 tensor receiving the timing indices."""
        if pitch:
            rc = self.L.qpsk_rx_batch_pitched(self.h, _ptr(x), pitch, F, _ptr(sym), _ptr(freq), _ptr(phase), None, _ptr(index), None)
        else:
            rc = self.L.qpsk_rx_batch(self.h, _ptr(x), F, _ptr(sym), _ptr(freq), _ptr(phase), None, _ptr(index), None)
        if rc:
            self._check(rc)

    def rx_batch_bw(self, frames, loop_bws):
        t = self.torch
        x = self._dev(frames, t.float32)
        F, B = x.shape[0], len(loop_bws)
        bws = (C.c_float * B)(*[float(b) for b in loop_bws])
        o = dict(sym=self.empty((F, B, self.nsym), t.uint8), freq=self.empty((F, B), t.float32),
                 phase=self.empty((F, B), t.float32), index=self.empty((F,), t.int32))
        self._check(self.L.qpsk_rx_batch_bw(self.h, _ptr(x), F, bws, B, _ptr(o["sym"]), _ptr(o["freq"]),
                                            _ptr(o["phase"]), _ptr(o["index"])))
        return o

    def rx_batch_ext(self, frames, index=None, seed=None, want_costas=False, pitch=0):
        """rx_batch with the acquisition from outside (qpsk_rx_batch_ext): index (F,) int32 decimation offsets 0..7 in place of the
        context's timing estimate, seed (F, 2) float32 (phase, freq) each loop starts from (set_phase / set_frequency); None = the
        context's timing / (0, 0).  pitch: frames are (F, pitch, 2) with the first frame_size samples of each row used (0 = packed).
        An offset outside 0..7 or a bad seed is reported by the next synchronising call (sync())."""
        t = self.torch
        x = self._dev(frames, t.float32)
        F = x.shape[0]
        assert x.shape[1] == (pitch or self.frame_size) and x.shape[2] == 2
        ix = None if index is None else self._dev(index, t.int32)
        sd = None if seed is None else self._dev(seed, t.float32)
        assert ix is None or tuple(ix.shape) == (F,)
        assert sd is None or tuple(sd.shape) == (F, 2)
        o = dict(sym=self.empty((F, self.nsym), t.uint8), freq=self.empty((F,), t.float32),
                 phase=self.empty((F,), t.float32), index=self.empty((F,), t.int32), hz=self.empty((F,), t.float32),
                 costas=self.empty((F, self.nsym, 2), t.float32) if want_costas else None)
        self._check(self.L.qpsk_rx_batch_ext(self.h, _ptr(x), int(pitch), F, _ptr(ix), _ptr(sd), _ptr(o["sym"]), _ptr(o["freq"]),
                                             _ptr(o["phase"]), _ptr(o["costas"]), _ptr(o["index"]), _ptr(o["hz"])))
        o["_keep"] = (x, ix, sd)      # the inputs stay alive until the caller is done with the outputs (stream order)
        return o

    def rx_batch_data(self, frames, index=None, seed=None, want_sym=False, pitch=0):
        """rx_batch_ext with the data rule's decisions (qpsk_rx_batch_data): dict of torch tensors data (F, nsym) uint8 -- (z.im < 0) << 1 |
        (z.re < 0) of costas_frame[], the transmitter's dibits up to the loop's quarter-turn rotation -- and freq, phase, index, hz as
        rx_batch_ext; with want_sym also sym, the slicer's decisions.  index, seed, pitch as rx_batch_ext."""
        t = self.torch
        x = self._dev(frames, t.float32)
        F = x.shape[0]
        assert x.shape[1] == (pitch or self.frame_size) and x.shape[2] == 2
        ix = None if index is None else self._dev(index, t.int32)
        sd = None if seed is None else self._dev(seed, t.float32)
        assert ix is None or tuple(ix.shape) == (F,)
        assert sd is None or tuple(sd.shape) == (F, 2)
        o = dict(data=self.empty((F, self.nsym), t.uint8), sym=self.empty((F, self.nsym), t.uint8) if want_sym else None,
                 freq=self.empty((F,), t.float32), phase=self.empty((F,), t.float32), index=self.empty((F,), t.int32),
                 hz=self.empty((F,), t.float32))
        self._check(self.L.qpsk_rx_batch_data(self.h, _ptr(x), int(pitch), F, _ptr(ix), _ptr(sd), _ptr(o["data"]), _ptr(o["sym"]),
                                              _ptr(o["freq"]), _ptr(o["phase"]), _ptr(o["index"]), _ptr(o["hz"])))
        o["_keep"] = (x, ix, sd)
        return o

    def _sync_search(self, data, sync, lag_min, lag_max, nout):
        """Sync-word search (qpsk_sync_batch) over data (F, nsym) uint8 decisions: sync is a sequence of dibits (1..128 of them), lags
        lag_min..lag_max.  Dict of torch tensors out (F, nout) uint8 -- the payload behind the word, de-rotated into the transmitter's
        dibits -- lag, rot, score (F,) int32."""
        t = self.torch
        d = self._dev(data, t.uint8)
        F, N = d.shape
        sw = np.ascontiguousarray(np.asarray(sync, dtype=np.uint8))
        o = dict(out=self.empty((F, nout), t.uint8), lag=self.empty((F,), t.int32), rot=self.empty((F,), t.int32),
                 score=self.empty((F,), t.int32))
        self._check(self.L.qpsk_sync_batch(self.h, _ptr(d), F, N, sw.ctypes.data_as(C.c_void_p), len(sw), int(lag_min), int(lag_max),
                                           int(nout), _ptr(o["out"]), _ptr(o["lag"]), _ptr(o["rot"]), _ptr(o["score"])))
        o["_keep"] = (d,)
        return o

    def rx_batch_bw_ext(self, frames, loop_bws, index=None, seed=None):
        """rx_batch_bw with the acquisition from outside (qpsk_rx_batch_bw_ext): index (F,) int32 or None, seed (F, nbw, 2) or None"""
        t = self.torch
        x = self._dev(frames, t.float32)
        F, B = x.shape[0], len(loop_bws)
        bws = (C.c_float * B)(*[float(b) for b in loop_bws])
        ix = None if index is None else self._dev(index, t.int32)
        sd = None if seed is None else self._dev(seed, t.float32)
        assert ix is None or tuple(ix.shape) == (F,)
        assert sd is None or tuple(sd.shape) == (F, B, 2)
        o = dict(sym=self.empty((F, B, self.nsym), t.uint8), freq=self.empty((F, B), t.float32),
                 phase=self.empty((F, B), t.float32), index=self.empty((F,), t.int32))
        self._check(self.L.qpsk_rx_batch_bw_ext(self.h, _ptr(x), F, bws, B, _ptr(ix), _ptr(sd), _ptr(o["sym"]), _ptr(o["freq"]),
                                                _ptr(o["phase"]), _ptr(o["index"])))
        o["_keep"] = (x, ix, sd)
        return o

    def carrier_est(self, frames, n=1024, start=128, pitch=0, want_line=False):
        """Coarse carrier estimate from the fourth-power line (qpsk_carrier_est_batch) over samples start .. start + n - 1 of each frame:
        dict of torch tensors seed (F, 2) float32 = (0, freq), ready for rx_batch_ext(seed=...); freq (F,) float32 in rad/symbol; bin (F,)
        int32; with want_line also line (F, 2) float64, the spectral line X[bin].  pitch as rx_batch_ext.  A NaN / Inf sample inside the
        window is reported by the next synchronising call (sync())."""
        t = self.torch
        x = self._dev(frames, t.float32)
        F = x.shape[0]
        assert x.shape[1] == (pitch or self.frame_size) and x.shape[2] == 2
        o = dict(seed=self.empty((F, 2), t.float32), freq=self.empty((F,), t.float32), bin=self.empty((F,), t.int32))
        if want_line:
            o["line"] = self.empty((F, 2), t.float64)
        self._check(self.L.qpsk_carrier_est_batch(self.h, _ptr(x), int(pitch), F, int(start), int(n), _ptr(o["seed"]), _ptr(o["freq"]),
                                                  _ptr(o["bin"]), _ptr(o.get("line"))))
        o["_keep"] = (x,)      # the input stays alive until the caller is done with the outputs (stream order)
        return o

    SOFT_MODES = {"unit": 0, "llr": 1}      # QPSK_SOFT_UNIT, QPSK_SOFT_LLR

    def soft(self, costas, skip=0, mode="unit", scale=64.0, gain=None, lag=None, rot=None, first=0, nout=None, want_sums=False):
        """Soft decisions and signal quality (qpsk_soft_batch) from rows of costas_frame[]: costas (R, nsym, 2) float32, or the dict that
        rx_batch_ext(want_costas=True) or streams_rx_pcm() returns.  Dict of torch tensors soft (R, nout, 2) int8 -- one value per bit of
        each dibit, positive <=> the bit is 0 -- quality (R, 4) float32 = (amp, snr, lock, nvar) and, with want_sums, sums (R, 4) float64.
        skip leaves the first symbols out of the sums; mode "unit" puts the constellation at +-scale, "llr" gives log-likelihood ratios
        in steps of scale; gain (R,) float32 replaces the row's own gain; lag, rot (R,) int32 and first, nout place and de-rotate the
        payload as sync() found it (lag, rot: its outputs; first: its word's length); nout None = the rest of the row.  A lag that leaves
        the row, or a NaN / Inf sample, is reported by the next synchronising call (sync())."""
        return self._soft(costas, skip, mode, scale, gain, lag, rot, first, nout, want_sums, True)

    def quality(self, costas, skip=0):
        """soft() without the soft output: dict with quality (R, 4) float32 = (amp, snr, lock, nvar) per row"""
        return self._soft(costas, skip, "unit", 64.0, None, None, None, 0, 0, False, False)

    def _soft(self, costas, skip, mode, scale, gain, lag, rot, first, nout, want_sums, want_soft):
        t = self.torch
        if isinstance(costas, dict):
            costas = costas["costas"]
        z = self._dev(costas, t.float32)
        if z.dim() != 3 or z.shape[2] != 2:
            raise ValueError("soft() input must be (rows, nsym, 2) float32")
        R, N = z.shape[0], z.shape[1]
        g = None if gain is None else self._dev(gain, t.float32)
        lg = None if lag is None else self._dev(lag, t.int32)
        rt = None if rot is None else self._dev(rot, t.int32)
        for a in (g, lg, rt):
            assert a is None or tuple(a.shape) == (R,)
        if nout is None:
            nout = N - first
        o = dict(quality=self.empty((R, 4), t.float32))
        if want_soft:
            o["soft"] = self.empty((R, nout, 2), t.int8)
        if want_sums:
            o["sums"] = self.empty((R, 4), t.float64)
        self._check(self.L.qpsk_soft_batch(self.h, _ptr(z), 0, R, N, int(skip), self.SOFT_MODES[mode], float(scale), _ptr(g), _ptr(lg),
                                           _ptr(rt), int(first), int(nout), _ptr(o.get("soft")), _ptr(o["quality"]), _ptr(o.get("sums"))))
        o["_keep"] = (z, g, lg, rt)      # the inputs stay alive until the caller is done with the outputs (stream order)
        return o

    # ---- the K = 7, rate-1/2 convolutional code
    def punct_ntx(self, nsteps, puncture):
        """qpsk_punct_ntx: the transmitted dibits of nsteps trellis steps behind a puncturing pattern (a key of PUNCTURE or a (period,
        keep0, keep1) tuple); host only"""
        rc = self.L.qpsk_punct_ntx(int(nsteps), *_pattern(puncture))
        self._check(min(rc, 0))
        return rc

    def conv_encode(self, bits_packed, nbits, tail=True, puncture=None, interleave=None):
        """qpsk_conv_encode_batch: bits_packed (R, ceil(nbits / 8)) uint8, bit t in byte t >> 3 at position t & 7 -> (R, nsteps) uint8 coded
        dibits, nsteps = nbits + 6 with the tail (six zero bits that bring the encoder back to state 0).  With puncture (a key of PUNCTURE
        or a (period, keep0, keep1) tuple) qpsk_conv_encode_punct_batch: (R, punct_ntx(nsteps)) transmitted dibits.  With interleave (a
        stride of INTERLEAVING, coprime to the 2 ntx bits of a row; None or 1 = off) qpsk_conv_encode_ilv_batch: the same dibits, their
        bits spread over the row (no puncture = rate 1/2)"""
        t = self.torch
        b = self._dev(bits_packed, t.uint8)
        if b.dim() != 2 or b.shape[1] != (int(nbits) + 7) // 8:
            raise ValueError("conv_encode() input must be (rows, ceil(nbits / 8)) uint8")
        nsteps = int(nbits) + (6 if tail else 0)
        if _interleaved(interleave):
            pat = _pattern("1/2" if puncture is None else puncture)
            out = self.empty((b.shape[0], self.punct_ntx(nsteps, pat)), t.uint8)
            self._check(self.L.qpsk_conv_encode_ilv_batch(self.h, _ptr(b), b.shape[0], int(nbits), 1 if tail else 0, *pat, int(interleave),
                                                          _ptr(out)))
            return out
        if puncture is not None:
            pat = _pattern(puncture)
            out = self.empty((b.shape[0], self.punct_ntx(nsteps, pat)), t.uint8)
            self._check(self.L.qpsk_conv_encode_punct_batch(self.h, _ptr(b), b.shape[0], int(nbits), 1 if tail else 0, *pat, _ptr(out)))
            return out
        out = self.empty((b.shape[0], nsteps), t.uint8)
        self._check(self.L.qpsk_conv_encode_batch(self.h, _ptr(b), b.shape[0], int(nbits), 1 if tail else 0, _ptr(out)))
        return out

    def viterbi(self, soft, flip=None, open_start=False, open_end=False, pitch=0, nsteps=None, puncture=None, interleave=None):
        """qpsk_viterbi_batch on soft (R, nsteps, 2) int8 -- what soft() returns under "soft" -- or, with pitch, (R, pitch, 2) of which the
        first nsteps steps of each row are decoded.  flip (nsteps,) uint8: the scrambler's keystream dibits, undone on the soft values.
        Dict of torch tensors bits (R, ceil(nsteps / 8)) uint8, packed low bits first, tail bits included, and info (R, 4) int32 = (end
        metric, end state, state the trace-back arrives at, channel bit errors against the re-encoded path).
        With puncture (a key of PUNCTURE or a (period, keep0, keep1) tuple) qpsk_viterbi_punct_batch: soft (R, ntx, 2), or (R, pitch, 2),
        holds the TRANSMITTED symbols, flip is (ntx,), and nsteps must be given (ntx does not determine it).
        With interleave (a stride of INTERLEAVING; None or 1 = off) qpsk_viterbi_ilv_batch on the rows as they were on air, shapes as with
        puncture (no puncture = rate 1/2, and nsteps defaults to the row's length)."""
        t = self.torch
        if isinstance(soft, dict):
            soft = soft["soft"]
        q = self._dev(soft, t.int8)
        ilv = _interleaved(interleave)
        if ilv and puncture is None:
            puncture = "1/2"
            if nsteps is None and q.dim() == 3 and not pitch:
                nsteps = q.shape[1]
        if puncture is not None:
            pat = _pattern(puncture)
            if nsteps is None:
                raise ValueError("viterbi(puncture=...) needs nsteps: the transmitted length does not determine it")
            n = int(nsteps)
            ntx = self.punct_ntx(n, pat)
            if q.dim() != 3 or q.shape[2] != 2 or q.shape[1] != (pitch or ntx):
                raise ValueError("viterbi(puncture=...) input must be (rows, ntx = %d or pitch, 2) int8" % ntx)
            f = None if flip is None else self._dev(flip, t.uint8)
            if f is not None and tuple(f.shape) != (ntx,):
                raise ValueError("viterbi(puncture=...) flip must be (ntx = %d,) uint8" % ntx)
            R = q.shape[0]
            o = dict(bits=self.empty((R, (n + 7) // 8), t.uint8), info=self.empty((R, 4), t.int32))
            flags = (1 if open_start else 0) | (2 if open_end else 0)
            if ilv:
                self._check(self.L.qpsk_viterbi_ilv_batch(self.h, _ptr(q), int(pitch), R, n, *pat, int(interleave), _ptr(f), flags,
                                                          _ptr(o["bits"]), _ptr(o["info"])))
            else:
                self._check(self.L.qpsk_viterbi_punct_batch(self.h, _ptr(q), int(pitch), R, n, *pat, _ptr(f), flags, _ptr(o["bits"]),
                                                            _ptr(o["info"])))
            o["_keep"] = (q, f)
            return o
        if q.dim() != 3 or q.shape[2] != 2 or (pitch and q.shape[1] != pitch):
            raise ValueError("viterbi() input must be (rows, nsteps or pitch, 2) int8")
        R = q.shape[0]
        n = int(nsteps) if nsteps is not None else q.shape[1]
        f = None if flip is None else self._dev(flip, t.uint8)
        assert f is None or tuple(f.shape) == (n,)
        o = dict(bits=self.empty((R, (n + 7) // 8), t.uint8), info=self.empty((R, 4), t.int32))
        self._check(self.L.qpsk_viterbi_batch(self.h, _ptr(q), int(pitch), R, n, _ptr(f), (1 if open_start else 0) | (2 if open_end else 0),
                                              _ptr(o["bits"]), _ptr(o["info"])))
        o["_keep"] = (q, f)      # the inputs stay alive until the caller is done with the outputs (stream order)
        return o

    # ---- the streaming decoder (VITERBI STREAM in include/qpsk_hip.h)
    def viterbi_stream_reset(self, nstreams, depth=128, window=256, puncture=None):
        """qpsk_viterbi_stream_reset: nstreams decoders that carry their path from call to call and emit every bit once it is depth steps
        old, `window` bits per decision (both multiples of 64, depth + window <= 8192).  puncture: a key of PUNCTURE or a (period, keep0,
        keep1) tuple; None = rate 1/2."""
        pat = _pattern("1/2" if puncture is None else puncture)
        self._check(self.L.qpsk_viterbi_stream_reset(self.h, int(nstreams), int(depth), int(window), *pat))
        self._vs_streams = int(nstreams)

    def viterbi_stream_emits(self, ntx):
        """qpsk_viterbi_stream_emits: the bits per stream a viterbi_stream() of ntx transmitted dibits would emit now; host only"""
        rc = self.L.qpsk_viterbi_stream_emits(self.h, int(ntx))
        self._check(min(rc, 0))
        return rc

    def _viterbi_stream_out(self, nbits):
        t = self.torch
        return dict(bits=self.empty((self._vs_streams, (nbits + 7) // 8), t.uint8), info=self.empty((self._vs_streams, 4), t.int32))

    def viterbi_stream(self, soft, pitch=0, ntx=None):
        """qpsk_viterbi_stream_push: soft (S, ntx, 2) int8, the TRANSMITTED symbols of every stream (whole periods of the pattern) -- or,
        with pitch, (S, pitch, 2) of which the first ntx dibits of each row are pushed.  Dict of torch tensors bits (S, nbits / 8) uint8
        (this call's emitted bits, low bits first), nbits, info (S, 4) int32 = (channel errors, non-zero soft values, the state the last
        decision traced from or -1, the metric spread there)."""
        t = self.torch
        if isinstance(soft, dict):
            soft = soft["soft"]
        if not self._vs_streams:
            raise QpskError("viterbi_stream() before viterbi_stream_reset()")
        q = self._dev(soft, t.int8)
        if q.dim() != 3 or q.shape[0] != self._vs_streams or q.shape[2] != 2 or (pitch and q.shape[1] != pitch):
            raise ValueError("viterbi_stream() input must be (streams = %d, ntx or pitch, 2) int8" % self._vs_streams)
        ntx = q.shape[1] if ntx is None else int(ntx)
        o = self._viterbi_stream_out(self.viterbi_stream_emits(ntx))
        n = C.c_int32(-1)
        self._check(self.L.qpsk_viterbi_stream_push(self.h, _ptr(q), int(pitch), ntx, _ptr(o["bits"]), o["bits"].shape[1], _ptr(o["info"]),
                                                    C.byref(n)))
        o["nbits"] = n.value
        o["_keep"] = (q,)      # the input stays alive until the caller is done with the outputs (stream order)
        return o

    def viterbi_stream_flush(self, terminated=False):
        """qpsk_viterbi_stream_flush: the bits not yet emitted, traced from state 0 (terminated) or from the best state; the streams are
        then as after viterbi_stream_reset().  Dict as viterbi_stream()."""
        if not self._vs_streams:
            raise QpskError("viterbi_stream_flush() before viterbi_stream_reset()")
        o = self._viterbi_stream_out(8192)      # a flush emits fewer than depth + window <= 8192 bits
        n = C.c_int32(-1)
        self._check(self.L.qpsk_viterbi_stream_flush(self.h, 1 if terminated else 0, _ptr(o["bits"]), o["bits"].shape[1], _ptr(o["info"]),
                                                     C.byref(n)))
        o["nbits"] = n.value
        o["bits"] = o["bits"][:, :(n.value + 7) // 8]
        return o

    def viterbi_stream_advance(self, delta):
        """Test hook: move the streaming decoder's position counters on by delta steps (qpsk_test_viterbi_stream_advance)."""
        self._check(self.L.qpsk_test_viterbi_stream_advance(self.h, int(delta)))

    def conv_encode_stream(self, bits_packed, nbits, state=None, puncture=None):
        """qpsk_conv_encode_stream_batch: conv_encode() without a tail over a register that is carried: bits_packed (R, ceil(nbits / 8)),
        state (R,) uint8 = the register's low six bits before the row (None = 0) -> (dibits (R, ntx) uint8, state (R,) uint8 behind the
        row).  nbits covers whole periods of the pattern that send whole dibits."""
        t = self.torch
        b = self._dev(bits_packed, t.uint8)
        if b.dim() != 2 or b.shape[1] != (int(nbits) + 7) // 8:
            raise ValueError("conv_encode_stream() input must be (rows, ceil(nbits / 8)) uint8")
        pat = _pattern("1/2" if puncture is None else puncture)
        K = bin(pat[1]).count("1") + bin(pat[2]).count("1")
        st = None if state is None else self._dev(state, t.uint8)
        if st is not None and tuple(st.shape) != (b.shape[0],):
            raise ValueError("conv_encode_stream() state must be (rows,) uint8")
        out = self.empty((b.shape[0], max(int(nbits) // pat[0] * K // 2, 1)), t.uint8)
        nxt = self.empty((b.shape[0],), t.uint8)
        self._check(self.L.qpsk_conv_encode_stream_batch(self.h, _ptr(b), b.shape[0], int(nbits), *pat, _ptr(st), _ptr(nxt), _ptr(out)))
        return out, nxt

    # ---- the outer link of a continuous stream
    def outer_reset(self, nstreams, n, branches=1, sync=0x47, lock=2, drop=3, polarity=True, msb_first=False, group=0):
        """qpsk_outer_reset: nstreams receivers of words of n bytes behind viterbi_stream(): word sync on the byte `sync` (declared after
        `lock` words in a row, lost after `drop` misses in a row, 0 = never), polarity resolution, and a Forney deinterleaver of
        `branches` branches (a divisor of n).  msb_first: a byte's first bit is its bit 7 (DVB's order).  group: 0, or 3..16 with lock >=
        group = qpsk_outer_reset_group: every group-th word carries the complement of `sync` (DVB: 8), and outer()'s flags >> 4 is a
        word's place in its group."""
        flags = (OUTER_POLARITY if polarity else 0) | (OUTER_MSB_FIRST if msb_first else 0)
        if group:
            self._check(self.L.qpsk_outer_reset_group(self.h, int(nstreams), int(n), int(branches), int(sync), int(lock), int(drop), flags, int(group)))
        else:
            self._check(self.L.qpsk_outer_reset(self.h, int(nstreams), int(n), int(branches), int(sync), int(lock), int(drop), flags))
        self._outer = (int(nstreams), int(n))

    def outer_max_words(self, nbits):
        """qpsk_outer_max_words: the most words per stream an outer() of nbits can emit; host only"""
        rc = self.L.qpsk_outer_max_words(self.h, int(nbits))
        self._check(min(rc, 0))
        return rc

    def outer(self, bits, nbits=None, pitch=0, max_words=None):
        """qpsk_outer_push: bits (S, ceil(nbits / 8)) uint8, low bits first -- the `bits` of viterbi_stream() as it is (or its dict) -- or,
        with pitch, (S, pitch) of which the first nbits bits of each row are pushed; nbits None = every bit of a row.  Dict of torch
        tensors count (S,) int32 (the true number of words, also beyond max_words), words (S, max_words, n) uint8, pos (S, max_words)
        int64, flags (S, max_words) uint8 (bit 0: the sync byte is wrong, bit 1: the stream is inverted), info (S, 4) int32 = (locked, s,
        locks declared, locks lost); only the first min(count, max_words) entries of a stream are written."""
        t = self.torch
        if isinstance(bits, dict):
            bits, nbits = bits["bits"], (bits["nbits"] if nbits is None else nbits)
        if self._outer is None:
            raise QpskError("outer() before outer_reset()")
        S, n = self._outer
        b = self._dev(bits, t.uint8)
        if b.dim() != 2 or b.shape[0] != S or (pitch and b.shape[1] != pitch):
            raise ValueError("outer() input must be (streams = %d, ceil(nbits / 8) or pitch) uint8" % S)
        nbits = 8 * b.shape[1] if nbits is None else int(nbits)
        mw = self.outer_max_words(nbits) if max_words is None else int(max_words)
        o = dict(count=self.empty((S,), t.int32), words=self.empty((S, mw, n), t.uint8), pos=self.empty((S, mw), t.int64),
                 flags=self.empty((S, mw), t.uint8), info=self.empty((S, 4), t.int32))
        self._check(self.L.qpsk_outer_push(self.h, _ptr(b), b.shape[1], nbits, mw, _ptr(o["count"]), _ptr(o["words"]), n, _ptr(o["pos"]),
                                           _ptr(o["flags"]), _ptr(o["info"])))
        o["_keep"] = (b,)      # the input stays alive until the caller is done with the outputs (stream order)
        return o

    def outer_interleave(self, words, branches, history=None):
        """qpsk_outer_interleave_batch: words (R, nwords, n) uint8 -> (out (R, nwords, n), history (R, branches - 1, n)): out[c][q] =
        words[c - q % branches][q]; history = the last branches - 1 source words before the call, oldest first (None = zeros), and after
        it."""
        t = self.torch
        w = self._dev(words, t.uint8)
        if w.dim() != 3:
            raise ValueError("outer_interleave() input must be (rows, nwords, n) uint8")
        R, nw, n = w.shape
        I = int(branches)
        h = None if history is None else self._dev(history, t.uint8)
        if h is not None and tuple(h.shape) != (R, I - 1, n):
            raise ValueError("outer_interleave() history must be (rows, branches - 1, n) uint8")
        out = self.empty((R, nw, n), t.uint8)
        nxt = self.empty((R, max(I - 1, 0), n), t.uint8)
        self._check(self.L.qpsk_outer_interleave_batch(self.h, _ptr(w), R, nw, n, I, _ptr(h) if I > 1 else None, _ptr(nxt) if I > 1 else None,
                                                       _ptr(out)))
        return out, nxt

    def outer_advance(self, delta):
        """Test hook: move the outer link's position counter on by delta bits, a multiple of 8 (qpsk_test_outer_advance)."""
        self._check(self.L.qpsk_test_outer_advance(self.h, int(delta)))

    # ---- DVB's energy dispersal (DVB TRANSPORT in include/qpsk_hip.h)
    def dispersal(self, rows, group=8, flags=None, first=0, msb_first=False, pitch=0):
        """qpsk_dispersal_batch: rows (R, len) uint8 -- a view with its rows further apart is taken as it lies -- -> (R, len) uint8, every
        row xored with its part of the dispersal sequence, the first byte of a row of group index 0 inverted.  flags None: row r has
        the index (first + r) % group (the transmitter); otherwise flags holds R bytes, outer()'s `flags` over the same rows, and a
        row's index is flags >> 4 (a row whose index is >= group is copied).  pitch: the bytes between the OUTPUT's rows (0 = tight);
        the result is then a view of a (R, pitch) buffer, whose other bytes are not written"""
        t = self.torch
        d = rows if isinstance(rows, t.Tensor) and rows.dtype == t.uint8 and rows.is_cuda else self._dev(rows, t.uint8)
        if d.dim() != 2:
            raise ValueError("dispersal() rows must be (rows, len) uint8")
        R, n = d.shape
        if d.stride(1) != 1 or (R > 1 and d.stride(0) < n):
            d = d.contiguous()
        f = None if flags is None else self._dev(flags, t.uint8).reshape(-1)
        if f is not None and f.numel() != R:
            raise ValueError("dispersal() flags must hold one byte per row (%d)" % R)
        buf = self.empty((R, int(pitch) or n), t.uint8)
        self._check(self.L.qpsk_dispersal_batch(self.h, _ptr(d), d.stride(0) if R > 1 else n, R, n, int(group), DISPERSAL_MSB_FIRST if msb_first else 0,
                                                _ptr(f), int(first), _ptr(buf), int(pitch)))
        self._dispersal_keep = (d, f)      # the inputs stay alive until the stream has run the call
        return buf[:, :n]

    # ---- the node sync in front of the streaming decoder (NODE SYNC in include/qpsk_hip.h)
    def nodesync_reset(self, nlinks, nrot=2, nshift=1, span=4096, settle=1024, threshold=(1, 32), drop=2):
        """qpsk_nodesync_reset: nlinks node syncs in front of viterbi_stream(): nrot (1, 2 or 4) quarter-turn candidates times nshift
        (nodesync_shifts(puncture)) delays; a candidate is judged over `span` counted soft values, bad when errors / counted > threshold =
        (num, den); `settle` counted values are skipped behind a switch (the decoder's latency: the soft values of depth + window
        steps); a locked link moves on after `drop` bad spans in a row."""
        num, den = threshold
        self._check(self.L.qpsk_nodesync_reset(self.h, int(nlinks), int(nrot), int(nshift), int(span), int(settle), int(num), int(den), int(drop)))
        self._ns_links = int(nlinks)

    def nodesync(self, soft, vinfo=None, pitch=0, ntx=None):
        """qpsk_nodesync_push: soft (S, ntx, 2) int8 as soft() writes it -- or, with pitch, (S, pitch, 2) of which the first ntx dibits of
        each row are pushed; vinfo (S, 4) int32 = the info of the previous viterbi_stream() (or its dict; it stays on the device), None = no
        tick.  Dict of torch tensors soft (S, ntx, 2) int8, which goes into viterbi_stream() as it is, and info (S, 8) int32 = (r, h, locked,
        switches, verdict, run, err, cnt)."""
        t = self.torch
        if isinstance(soft, dict):
            soft = soft["soft"]
        if isinstance(vinfo, dict):
            vinfo = vinfo["info"]
        if not self._ns_links:
            raise QpskError("nodesync() before nodesync_reset()")
        S = self._ns_links
        q = self._dev(soft, t.int8)
        if q.dim() != 3 or q.shape[0] != S or q.shape[2] != 2 or (pitch and q.shape[1] != pitch):
            raise ValueError("nodesync() input must be (links = %d, ntx or pitch, 2) int8" % S)
        v = None if vinfo is None else self._dev(vinfo, t.int32)
        if v is not None and tuple(v.shape) != (S, 4):
            raise ValueError("nodesync() vinfo must be (links = %d, 4) int32" % S)
        ntx = q.shape[1] if ntx is None else int(ntx)
        o = dict(soft=self.empty((S, max(ntx, 0), 2), t.int8), info=self.empty((S, 8), t.int32))
        self._check(self.L.qpsk_nodesync_push(self.h, _ptr(q), int(pitch), ntx, _ptr(v), _ptr(o["soft"]), 0, _ptr(o["info"])))
        o["_keep"] = (q, v)      # the inputs stay alive until the caller is done with the outputs (stream order)
        return o

    def nodesync_set(self, cand=None):
        """qpsk_nodesync_set: put every link on candidate cand[l] (mod nrot * nshift; None = 0) with a fresh monitor; the carried history
        and the switch count stay."""
        if not self._ns_links:
            raise QpskError("nodesync_set() before nodesync_reset()")
        d = None if cand is None else self._dev(cand, self.torch.int32)
        if d is not None and tuple(d.shape) != (self._ns_links,):
            raise ValueError("nodesync_set() cand must be (links = %d,) int32" % self._ns_links)
        self._check(self.L.qpsk_nodesync_set(self.h, _ptr(d)))

    # ---- stages
    def rrc_fir(self, x, memory=None, fast=False):
        """x: (F, n, 2); memory: (F, 127, 2) updated in place (torch tensor) or None.  fast: the overlap-save filter
        (qpsk_rrc_fir_batch_fast: ~1e-6 of the peak from the exact one, not bit for bit)."""
        t = self.torch
        x = self._dev(x, t.float32)
        y = t.empty_like(x)
        fn = self.L.qpsk_rrc_fir_batch_fast if fast else self.L.qpsk_rrc_fir_batch
        self._check(fn(self.h, _ptr(memory), _ptr(x), _ptr(y), x.shape[0], x.shape[1]))
        return y

    def timing_hist(self, filtered, want_hist=False):
        t = self.torch
        y = self._dev(filtered, t.float32)
        idx = self.empty((y.shape[0],), t.int32)
        hist = self.empty((y.shape[0], 8), t.int32) if want_hist else None
        self._check(self.L.qpsk_timing_hist_batch(self.h, _ptr(y), y.shape[0], _ptr(idx), _ptr(hist)))
        return (idx, hist) if want_hist else idx

    def timing_scan(self, frames):
        """histogram timing estimate straight from unfiltered (F, frame_size, 2) frames -> (index (F,), hist (F, 8))"""
        t = self.torch
        x = self._dev(frames, t.float32)
        idx = self.empty((x.shape[0],), t.int32)
        hist = self.empty((x.shape[0], 8), t.int32)
        self._check(self.L.qpsk_timing_scan_batch(self.h, _ptr(x), x.shape[0], _ptr(idx), _ptr(hist)))
        return idx, hist

    def timing_fft(self, frames, want_internals=False):
        """FFT timing estimate of (F, frame_size, 2) frames -> index (F,) [, filtered (F, 512, 2), spectrum (F, 512) complex128]"""
        t = self.torch
        x = self._dev(frames, t.float32)
        F = x.shape[0]
        idx = self.empty((F,), t.int32)
        y = self.empty((F, 512, 2), t.float32) if want_internals else None
        X = self.empty((F, 512), t.complex128) if want_internals else None
        self._check(self.L.qpsk_timing_fft_batch(self.h, _ptr(x), F, _ptr(idx), _ptr(y), _ptr(X)))
        return (idx, y, X) if want_internals else idx

    def timing_fft_bin(self, frames):
        """the estimate as qpsk_rx_batch runs it (pruned transform) -> index (F,), filtered (F, 512, 2), bin (F,) complex128"""
        t = self.torch
        x = self._dev(frames, t.float32)
        F = x.shape[0]
        idx = self.empty((F,), t.int32)
        y = self.empty((F, 512, 2), t.float32)
        xk = self.empty((F,), t.complex128)
        self._check(self.L.qpsk_timing_fft_bin_batch(self.h, _ptr(x), F, _ptr(idx), _ptr(y), _ptr(xk)))
        return idx, y, xk

    def costas(self, d, state=None, want_costas=True):
        t = self.torch
        d = self._dev(d, t.float32)
        F, N = d.shape[0], d.shape[1]
        sym = self.empty((F, N), t.uint8)
        z = self.empty((F, N, 2), t.float32) if want_costas else None
        self._check(self.L.qpsk_costas_batch(self.h, _ptr(d), F, N, _ptr(state), _ptr(sym), _ptr(z)))
        return sym, z

    def fft(self, x, inverse=False):
        """x: (B, n) complex128 numpy/torch -> torch complex128"""
        t = self.torch
        if isinstance(x, np.ndarray):
            x = t.from_numpy(np.ascontiguousarray(x, dtype=np.complex128))
        x = x.to(self.dev).contiguous()
        out = t.empty_like(x)
        self._check(self.L.qpsk_fft_batch(self.h, _ptr(x), _ptr(out), x.shape[0], x.shape[1], int(inverse)))
        return out

    # ---- streams
    def streams_reset(self, nstreams, mixer_hz=1500.0):
        self._check(self.L.qpsk_streams_reset(self.h, nstreams, mixer_hz))
        self.nstreams = nstreams

    def _stream_out(self, want_costas):
        t, n = self.torch, self.nstreams
        return dict(sym=self.empty((n, self.nsym), t.uint8), freq=self.empty((n,), t.float32),
                    phase=self.empty((n,), t.float32), index=self.empty((n,), t.int32),
                    costas=self.empty((n, self.nsym, 2), t.float32) if want_costas else None)

    def streams_rx_cplx(self, blocks, want_costas=True):
        x = self._dev(blocks, self.torch.float32)
        o = self._stream_out(want_costas)
        self._check(self.L.qpsk_streams_rx_cplx(self.h, _ptr(x), _ptr(o["sym"]), _ptr(o["freq"]), _ptr(o["phase"]),
                                                _ptr(o["costas"]), _ptr(o["index"])))
        return o

    def streams_rx_pcm(self, pcm, want_costas=True):
        x = self._dev(pcm, self.torch.int16)
        o = self._stream_out(want_costas)
        self._check(self.L.qpsk_streams_rx_pcm(self.h, _ptr(x), _ptr(o["sym"]), _ptr(o["freq"]), _ptr(o["phase"]),
                                               _ptr(o["costas"]), _ptr(o["index"])))
        return o

    # ---- the polyphase channeliser in front of the streams (CHANNELISER in include/qpsk_hip.h)
    def channel_reset(self, M, P, proto, chan=None):
        """qpsk_channel_reset: M channels (a power of two, 2..4096), P taps per branch (1..32), proto the M P real taps (e.g.
        channel_prototype(M, P)); chan: the channel numbers of the output rows, any order, repeats allowed; None = all M in order.
        Zeroes the history"""
        h = np.ascontiguousarray(np.asarray(proto, dtype=np.float32).reshape(-1))
        if h.size != int(M) * int(P):
            raise ValueError("channel_reset() proto must hold M * P = %d taps" % (int(M) * int(P)))
        ch = None if chan is None else np.ascontiguousarray(np.asarray(chan, dtype=np.int32).reshape(-1))
        self._check(self.L.qpsk_channel_reset(self.h, int(M), int(P), h.ctypes.data_as(C.c_void_p),
                                              None if ch is None else ch.ctypes.data_as(C.c_void_p), 0 if ch is None else len(ch)))
        self._channel = (int(M), int(M) if ch is None else len(ch))

    def channel(self, x, pitch=0):
        """qpsk_channel_push: x (T * M, 2) float32, the next T * M wideband samples -> (nsel, T, 2) float32, row i = channel chan[i]:
        the blocks streams_rx_cplx() takes.  pitch: the complex samples between the OUTPUT's rows (0 = tight); the result is then a view
        of a (nsel, pitch, 2) buffer whose other samples are not written"""
        t = self.torch
        if self._channel is None:
            raise QpskError("channel() before channel_reset()")
        M, nsel = self._channel
        x = self._dev(x, t.float32)
        if x.dim() != 2 or x.shape[1] != 2 or x.shape[0] < M or x.shape[0] % M:
            raise ValueError("channel() input must be (T * %d, 2) float32" % M)
        T = x.shape[0] // M
        rows = int(pitch) if pitch else T
        buf = self.empty((nsel, rows, 2), t.float32)
        self._check(self.L.qpsk_channel_push(self.h, _ptr(x), T, _ptr(buf), int(pitch)))
        self._channel_keep = (x,)      # the input stays alive until the stream has run the call
        return buf[:, :T]

    # ---- the synthesis bank, the channeliser's transmit twin (SYNTHESIS BANK in include/qpsk_hip.h)
    def synth_reset(self, M, P, proto, chan=None):
        """qpsk_synth_reset: M channels (a power of two, 2..4096), P taps per branch (1..32), proto the M P real taps with the
        interpolation gain in them (e.g. channel_prototype(M, P, gain=M)); chan: the channels the input rows go to, any order, no
        repeats; None = all M in order.  Zeroes the history"""
        h = np.ascontiguousarray(np.asarray(proto, dtype=np.float32).reshape(-1))
        if h.size != int(M) * int(P):
            raise ValueError("synth_reset() proto must hold M * P = %d taps" % (int(M) * int(P)))
        ch = None if chan is None else np.ascontiguousarray(np.asarray(chan, dtype=np.int32).reshape(-1))
        self._check(self.L.qpsk_synth_reset(self.h, int(M), int(P), h.ctypes.data_as(C.c_void_p),
                                            None if ch is None else ch.ctypes.data_as(C.c_void_p), 0 if ch is None else len(ch)))
        self._synth = (int(M), int(M) if ch is None else len(ch))

    def synth(self, rows, pitch=0):
        """qpsk_synth_push: rows (nsel, T, 2) float32, the next T samples of every selected channel (row i goes to channel chan[i]) ->
        (T * M, 2) float32, the next T * M wideband samples: what channel() takes.  pitch: the complex samples between the INPUT's rows
        (0 = tight); rows is then a view (nsel, T, 2) of a (nsel, pitch, 2) float32 buffer on the device, read where it lies"""
        t = self.torch
        if self._synth is None:
            raise QpskError("synth() before synth_reset()")
        M, nsel = self._synth
        if pitch:
            c = rows
            if not isinstance(c, t.Tensor) or c.device != self.dev or c.dtype != t.float32 or c.dim() != 3 or c.stride() != (2 * int(pitch), 2, 1):
                raise ValueError("synth() with a pitch takes a float32 device view whose rows lie 2 * pitch floats apart")
        else:
            c = self._dev(rows, t.float32)
        if c.dim() != 3 or c.shape[0] != nsel or c.shape[1] < 1 or c.shape[2] != 2:
            raise ValueError("synth() input must be (%d, T, 2) float32" % nsel)
        T = c.shape[1]
        x = self.empty((T * M, 2), t.float32)
        self._check(self.L.qpsk_synth_push(self.h, _ptr(c), int(pitch), T, _ptr(x)))
        self._synth_keep = (c,)      # the input stays alive until the stream has run the call
        return x

    # ---- the rational resampler between the capture's rate and the modem's (RESAMPLER in include/qpsk_hip.h)
    def resample_reset(self, nstreams, L, D, P, proto):
        """qpsk_resample_reset: nstreams rows (1..65536) resampled by L / D (L 1..512, D 1..4096), P taps per branch (1..32), proto the
        L P real taps with the interpolation gain in them (e.g. resample_prototype(L, D, P)).  Zeroes the history and the position"""
        h = np.ascontiguousarray(np.asarray(proto, dtype=np.float32).reshape(-1))
        if h.size != int(L) * int(P):
            raise ValueError("resample_reset() proto must hold L * P = %d taps" % (int(L) * int(P)))
        self._check(self.L.qpsk_resample_reset(self.h, int(nstreams), int(L), int(D), int(P), h.ctypes.data_as(C.c_void_p)))
        self._resample = int(nstreams)

    def resample_need(self, nout):
        """qpsk_resample_need: the input samples per stream the NEXT resample() of nout outputs consumes (0 is possible when L > D)"""
        rc = self.L.qpsk_resample_need(self.h, int(nout))
        if rc < 0:
            self._check(rc)
        return rc

    def resample(self, rows, nout, pitch=0, out_pitch=0):
        """qpsk_resample_push: rows (nstreams, nin, 2) float32, the next nin samples of every stream, nin = resample_need(nout) (ValueError
        otherwise) -> (nstreams, nout, 2) float32, the next nout outputs.  pitch: the complex samples between the INPUT's rows (0 = tight);
        rows is then a view (nstreams, nin, 2) of a (nstreams, pitch, 2) float32 buffer on the device, read where it lies (what channel()
        returns with its pitch).  out_pitch: the same for the OUTPUT's rows; the result is then a view of a (nstreams, out_pitch, 2) buffer
        whose other samples are not written"""
        t = self.torch
        if not self._resample:
            raise QpskError("resample() before resample_reset()")
        S = self._resample
        if pitch:
            c = rows
            if not isinstance(c, t.Tensor) or c.device != self.dev or c.dtype != t.float32 or c.dim() != 3 or \
                    (c.shape[1] > 0 and (c.stride()[1:] != (2, 1) or (c.shape[0] > 1 and c.stride(0) != 2 * int(pitch)))):
                raise ValueError("resample() with a pitch takes a float32 device view whose rows lie 2 * pitch floats apart")
        else:
            c = self._dev(rows, t.float32)
        if c.dim() != 3 or c.shape[0] != S or c.shape[2] != 2:
            raise ValueError("resample() input must be (%d, nin, 2) float32" % S)
        need = self.resample_need(nout)
        if c.shape[1] != need:
            raise ValueError("resample() of %d outputs consumes %d samples per stream now, not %d" % (int(nout), need, c.shape[1]))
        buf = self.empty((S, int(out_pitch) if out_pitch else int(nout), 2), t.float32)
        self._check(self.L.qpsk_resample_push(self.h, _ptr(c) if need else None, int(pitch), need, int(nout), _ptr(buf), int(out_pitch)))
        self._resample_keep = (c,)      # the input stays alive until the stream has run the call
        return buf[:, :int(nout)]

    # ---- packets from continuous streams (qpsk_deframer_*)
    def deframer_reset(self, nstreams, sync, nbytes, min_score, max_packets=8):
        """One deframer state per stream (independent of the receive streams): sync is a sequence of 1..128 dibits, a packet is nbytes
        of payload and its CRC-16; a position whose best rotation matches min_score or more of the word's dibits starts a packet."""
        sw = np.ascontiguousarray(np.asarray(sync, dtype=np.uint8))
        self._check(self.L.qpsk_deframer_reset(self.h, int(nstreams), sw.ctypes.data_as(C.c_void_p), len(sw), int(min_score), int(nbytes),
                                               int(max_packets)))
        self.df_shape = (int(nstreams), int(nbytes), int(max_packets))

    def deframe(self, costas=None, data=None):
        """Push one row per stream: costas (nstreams, nsym, 2) float32 -- e.g. the dict streams_rx_pcm(..., want_costas=True) returns --
        or data (nstreams, nsym) uint8 dibits.  Dict of torch tensors for the packets completed by this push: count (nstreams,) int32
        (the true number; only the first max_packets rows are written), bytes (nstreams, max_packets, nbytes + 2) uint8, pos
        (nstreams, max_packets) int64, rot, score int32, crc_ok uint8."""
        t = self.torch
        if isinstance(costas, dict):
            costas = costas["costas"]
        if (costas is None) == (data is None):
            raise ValueError("deframe() takes exactly one of costas, data")
        x = self._dev(costas, t.float32) if costas is not None else self._dev(data, t.uint8)
        S, nb, M = self.df_shape
        if x.shape[0] != S or (costas is not None and (x.dim() != 3 or x.shape[2] != 2)) or (data is not None and x.dim() != 2):
            raise ValueError("deframe() input must be (%d, nsym, 2) float32 or (%d, nsym) uint8" % (S, S))
        o = dict(count=self.empty((S,), t.int32), bytes=self.torch.zeros((S, M, nb + 2), dtype=t.uint8, device=self.dev),
                 pos=t.zeros((S, M), dtype=t.int64, device=self.dev), rot=t.zeros((S, M), dtype=t.int32, device=self.dev),
                 score=t.zeros((S, M), dtype=t.int32, device=self.dev), crc_ok=t.zeros((S, M), dtype=t.uint8, device=self.dev))
        self._check(self.L.qpsk_deframer_push(self.h, _ptr(x) if costas is not None else None, _ptr(x) if data is not None else None,
                                              x.shape[1], _ptr(o["count"]), _ptr(o["bytes"]), _ptr(o["pos"]), _ptr(o["rot"]),
                                              _ptr(o["score"]), _ptr(o["crc_ok"])))
        o["_keep"] = (x,)
        return o

    def deframer_reset_coded(self, nstreams, sync, nbytes, min_score, max_packets=8, mode="unit", scale=64.0, puncture=None, interleave=None):
        """deframer_reset() for packets whose body carries the K = 7 rate-1/2 code: [sync][scrambled conv_encode(payload + CRC-16, tail)].
        mode, scale: soft()'s, for the gain of a push that brings none of its own.  Replaces an uncoded deframer of the context.
        With puncture (a key of PUNCTURE or a (period, keep0, keep1) tuple) qpsk_deframer_reset_coded_punct: the body is
        conv_encode(..., puncture=...); deframe_coded() is the push of both.  With interleave (a stride of INTERLEAVING; None or 1 = off)
        qpsk_deframer_reset_coded_ilv: the body frame(..., interleave=...) sends; a refused stride leaves the deframer as it was."""
        sw = np.ascontiguousarray(np.asarray(sync, dtype=np.uint8))
        if _interleaved(interleave):
            self._check(self.L.qpsk_deframer_reset_coded_ilv(self.h, int(nstreams), sw.ctypes.data_as(C.c_void_p), len(sw), int(min_score),
                                                             int(nbytes), int(max_packets), self.SOFT_MODES[mode], float(scale),
                                                             *_pattern("1/2" if puncture is None else puncture), int(interleave)))
            self.df_shape = (int(nstreams), int(nbytes), int(max_packets))
            return
        if puncture is not None:
            self._check(self.L.qpsk_deframer_reset_coded_punct(self.h, int(nstreams), sw.ctypes.data_as(C.c_void_p), len(sw), int(min_score),
                                                               int(nbytes), int(max_packets), self.SOFT_MODES[mode], float(scale),
                                                               *_pattern(puncture)))
            self.df_shape = (int(nstreams), int(nbytes), int(max_packets))
            return
        self._check(self.L.qpsk_deframer_reset_coded(self.h, int(nstreams), sw.ctypes.data_as(C.c_void_p), len(sw), int(min_score), int(nbytes),
                                                     int(max_packets), self.SOFT_MODES[mode], float(scale)))
        self.df_shape = (int(nstreams), int(nbytes), int(max_packets))

    def deframe_coded(self, costas, gain=None):
        """Push one row per stream: costas (nstreams, nsym, 2) float32, or the dict streams_rx_pcm(..., want_costas=True) returns; gain
        (nstreams,) float32 = this push's soft gain per stream, None = each row's own (soft()'s rule with skip 0).  Dict of torch tensors
        for the packets completed by this push: count, bytes, pos, rot, score, crc_ok as deframe(), and info (nstreams, max_packets, 4)
        int32 = the decoder's (end metric, end state, start state, channel bit errors)."""
        t = self.torch
        if isinstance(costas, dict):
            costas = costas["costas"]
        x = self._dev(costas, t.float32)
        S, nb, M = self.df_shape
        if x.dim() != 3 or x.shape[0] != S or x.shape[2] != 2:
            raise ValueError("deframe_coded() input must be (%d, nsym, 2) float32" % S)
        g = None if gain is None else self._dev(gain, t.float32)
        if g is not None and tuple(g.shape) != (S,):
            raise ValueError("deframe_coded() gain must be (%d,) float32" % S)
        z = lambda shape, dt: t.zeros(shape, dtype=dt, device=self.dev)      # noqa: E731
        o = dict(count=self.empty((S,), t.int32), bytes=z((S, M, nb + 2), t.uint8), pos=z((S, M), t.int64), rot=z((S, M), t.int32),
                 score=z((S, M), t.int32), crc_ok=z((S, M), t.uint8), info=z((S, M, 4), t.int32))
        self._check(self.L.qpsk_deframer_push_coded(self.h, _ptr(x), x.shape[1], _ptr(g), _ptr(o["count"]), _ptr(o["bytes"]), _ptr(o["pos"]),
                                                    _ptr(o["rot"]), _ptr(o["score"]), _ptr(o["crc_ok"]), _ptr(o["info"])))
        o["_keep"] = (x, g)
        return o

    # ---- packets onto the air (qpsk_frame_batch), the transmit twin of the deframers
    def frame(self, payloads, sync, coded=True, puncture=None, per_row=1, lead=0, gap=0, row_len=None, interleave=None):
        """qpsk_frame_batch: payloads (nrows * per_row, nbytes) or (nrows, per_row, nbytes) uint8 -> dict of torch tensors dibits (nrows,
        row_len) uint8 -- per row per_row packets [sync][scrambled body], the first at column lead, gap idle columns between two, idle fill
        (the scrambler's keystream from column 0) everywhere else: rows for tx_symbols() -- and crc (nrows * per_row,) int16, the CRC-16
        sent (view it as uint16, as crc16() does).  sync: 1..128 dibits.  coded=False: the body deframe() receives; coded=True: the K = 7
        code, rate 1/2 (deframer_reset_coded) or, with puncture (a key of PUNCTURE or a (period, keep0, keep1) tuple), the punctured
        body.  row_len None = the exact fit.  interleave: a stride of INTERLEAVING for the coded body (None or 1 = off), which
        qpsk_frame_batch_ilv spreads over the body on air; deframer_reset_coded(..., interleave=...) receives it."""
        t = self.torch
        p = self._dev(payloads, t.uint8)
        per_row, lead, gap = int(per_row), int(lead), int(gap)
        if p.dim() == 3 and p.shape[1] == per_row:
            p = p.reshape(-1, p.shape[2])
        if p.dim() != 2 or per_row < 1 or p.shape[0] < 1 or p.shape[0] % per_row:
            raise ValueError("frame() payloads must be (nrows * per_row, nbytes) or (nrows, per_row, nbytes) uint8")
        npk, nbytes = p.shape
        sw = np.ascontiguousarray(np.asarray(sync, dtype=np.uint8))
        code = _coding(coded, puncture)
        if row_len is None:
            P = self.L.qpsk_frame_len(len(sw), nbytes, *code)
            self._check(min(P, 0))
            row_len = lead + per_row * P + (per_row - 1) * gap
        o = dict(dibits=self.empty((npk // per_row, int(row_len)), t.uint8), crc=self.empty((npk,), t.int16))
        if _interleaved(interleave):
            self._check(self.L.qpsk_frame_batch_ilv(self.h, _ptr(p), 0, npk // per_row, per_row, nbytes, sw.ctypes.data_as(C.c_void_p), len(sw),
                                                    *code, int(interleave), lead, gap, int(row_len), _ptr(o["dibits"]), _ptr(o["crc"])))
        else:
            self._check(self.L.qpsk_frame_batch(self.h, _ptr(p), 0, npk // per_row, per_row, nbytes, sw.ctypes.data_as(C.c_void_p), len(sw),
                                                *code, lead, gap, int(row_len), _ptr(o["dibits"]), _ptr(o["crc"])))
        o["_keep"] = (p,)      # the input stays alive until the caller is done with the outputs (stream order)
        return o

    # ---- the Reed-Solomon outer code (qpsk_rs_*)
    def rs_encode(self, data, nroots, pitch=0):
        """qpsk_rs_encode_batch: data (R, k) uint8 -> (R, k + nroots) uint8, the data and then the parity of the (k + nroots, k) code over
        GF(256).  pitch: the bytes between the OUTPUT's rows (0 = tight); the result is then a view of a (R, pitch) buffer, whose other
        bytes are not written"""
        t = self.torch
        d = self._dev(data, t.uint8)
        if d.dim() != 2:
            raise ValueError("rs_encode() data must be (rows, k) uint8")
        R, k = d.shape
        n = k + int(nroots)
        buf = self.empty((R, int(pitch) or n), t.uint8)
        self._check(self.L.qpsk_rs_encode_batch(self.h, _ptr(d), 0, R, k, int(nroots), _ptr(buf), int(pitch)))
        self._rs_keep = (d,)      # the input stays alive until the stream has run the call
        return buf[:, :n]

    def rs_decode(self, words, nroots, erasures=None, pitch=0, n=None, inplace=False):
        """qpsk_rs_decode_batch: words (R, n) uint8, or with pitch (R, pitch) of which the first n bytes of each row are the codeword --
        the deframers' bytes reshaped to (S * M, nbytes + 2) with pitch = nbytes + 2, n = nbytes.  erasures (R, n) uint8, non-zero =
        that byte is erased, or None.  -> (words (R, n) uint8, info (R, 4) int32 = (bytes changed or -1, erasures, errors or -1, the
        row came in with zero syndromes)).  A row that cannot be decoded comes back as it was with info[:, 0] = -1.  inplace: the
        corrected rows are written over words (a device tensor) and the first result is a view of it"""
        t = self.torch
        w = self._dev(words, t.uint8)
        if w.dim() != 2 or (pitch and w.shape[1] != pitch):
            raise ValueError("rs_decode() words must be (rows, n or pitch) uint8")
        R = w.shape[0]
        n = int(n) if n is not None else w.shape[1]
        e = None if erasures is None else self._dev(erasures, t.uint8)
        if e is not None and tuple(e.shape) != (R, n):
            raise ValueError("rs_decode() erasures must be (%d, %d) uint8" % (R, n))
        if inplace and (not isinstance(words, t.Tensor) or w.data_ptr() != words.data_ptr()):
            raise ValueError("rs_decode(inplace=True) needs a contiguous uint8 tensor on the modem's device")
        out = w if inplace else self.empty((R, n), t.uint8)
        info = self.empty((R, 4), t.int32)
        self._check(self.L.qpsk_rs_decode_batch(self.h, _ptr(w), int(pitch), R, n, int(nroots), _ptr(e), _ptr(out), int(pitch) if inplace else 0,
                                                _ptr(info)))
        self._rs_keep = (w, e)
        return out[:, :n], info

    # ---- the packet erasure code (qpsk_rs_cross_*): Reed-Solomon across the packets of a group
    def rs_cross_encode(self, groups, nroots, skip=0):
        """qpsk_rs_cross_encode_batch: groups (G, n, len) uint8, n = k + nroots packets each -- the k data packets filled in, the first
        skip bytes of every packet the caller's header.  The parity packets' bytes [skip, len) are written IN PLACE so that every byte
        column is a codeword of the (n, k) code; -> the device tensor (groups itself when it is a contiguous uint8 tensor on the modem's
        device).  groups.reshape(G * n, len) is then frame()'s payloads"""
        t = self.torch
        g = self._dev(groups, t.uint8)
        if g.dim() != 3:
            raise ValueError("rs_cross_encode() groups must be (G, n, len) uint8")
        G, n, ln = g.shape
        self._check(self.L.qpsk_rs_cross_encode_batch(self.h, _ptr(g), 0, G, n - int(nroots), int(nroots), ln, int(skip)))
        return g

    def rs_cross_decode(self, groups, have, nroots, skip=0, inplace=False):
        """qpsk_rs_cross_decode_batch: groups (G, n, len) uint8, have (G, n) uint8 (zero = that packet is missing) -> (groups (G, n, len)
        uint8, info (G, 4) int32 = (columns failed, missing packets, bytes changed, 1 if no column failed)).  A column that cannot be
        completed comes back as it was.  inplace: the result is written over groups (a device tensor) and the first result is groups"""
        t = self.torch
        g = self._dev(groups, t.uint8)
        if g.dim() != 3:
            raise ValueError("rs_cross_decode() groups must be (G, n, len) uint8")
        G, n, ln = g.shape
        h = self._dev(have, t.uint8)
        if tuple(h.shape) != (G, n):
            raise ValueError("rs_cross_decode() have must be (%d, %d) uint8" % (G, n))
        if inplace and (not isinstance(groups, t.Tensor) or g.data_ptr() != groups.data_ptr()):
            raise ValueError("rs_cross_decode(inplace=True) needs a contiguous uint8 tensor on the modem's device")
        out = g if inplace else self.empty((G, n, ln), t.uint8)
        info = self.empty((G, 4), t.int32)
        self._check(self.L.qpsk_rs_cross_decode_batch(self.h, _ptr(g), 0, G, n, int(nroots), ln, int(skip), _ptr(h), _ptr(out), 0, _ptr(info),
                                                      None))
        self._rs_keep = (g, h)
        return out, info

    def rs_cross_place(self, bytes, count, crc_ok, n, ngroups, base=None, groups=None, have=None):      # noqa: A002 (the header's name)
        """qpsk_rs_cross_place_batch: bytes (S, M, row) uint8, count (S,) int32 and crc_ok (S, M) uint8 as deframe() / deframe_coded()
        return them; byte 0 of a packet is its sequence number q.  A packet with crc_ok set and d = (q - base[s]) & 255 < ngroups * n goes to
        groups[s, d // n, d % n] and sets have[s, d]; the later of two with one d wins.  base (S,) int32 or None = 0.  groups (S, ngroups,
        n, len) and have (S, ngroups * n) are device tensors to accumulate into -- the first len <= row bytes of a packet are taken, so
        len = nbytes leaves the deframers' two CRC bytes behind -- or None: zeroed buffers with len = row.  -> (groups, have)"""
        t = self.torch
        b = self._dev(bytes, t.uint8)
        if b.dim() != 3:
            raise ValueError("rs_cross_place() bytes must be (S, max_packets, row) uint8")
        S, M, row = b.shape
        n, ngroups = int(n), int(ngroups)
        cnt, ok = self._dev(count, t.int32), self._dev(crc_ok, t.uint8)
        if tuple(cnt.shape) != (S,) or tuple(ok.shape) != (S, M):
            raise ValueError("rs_cross_place() count must be (%d,) int32 and crc_ok (%d, %d) uint8" % (S, S, M))
        bs = None if base is None else self._dev(base, t.int32)
        if bs is not None and tuple(bs.shape) != (S,):
            raise ValueError("rs_cross_place() base must be (%d,) int32" % S)
        if groups is None:
            groups = t.zeros((S, max(ngroups, 0), max(n, 0), row), dtype=t.uint8, device=self.dev)
        if have is None:
            have = t.zeros((S, max(ngroups * n, 0)), dtype=t.uint8, device=self.dev)
        for name, x, shape in (("groups", groups, (S, ngroups, n)), ("have", have, (S, ngroups * n))):
            if not isinstance(x, t.Tensor) or x.dtype != t.uint8 or not x.is_contiguous() or x.device != self.dev or tuple(x.shape[:len(shape)]) != shape:
                raise ValueError("rs_cross_place() %s must be a contiguous uint8 tensor %s on the modem's device" % (name, shape))
        if groups.dim() != 4 or groups.shape[3] > row:
            raise ValueError("rs_cross_place() groups must be (S, ngroups, n, len) with len <= %d" % row)
        self._check(self.L.qpsk_rs_cross_place_batch(self.h, _ptr(b), row, _ptr(cnt), _ptr(ok), S, M, groups.shape[3], n, ngroups, _ptr(bs),
                                                     _ptr(groups), 0, _ptr(have)))
        self._rs_keep = (b, cnt, ok, bs)
        return groups, have

    def streams_loop_state(self):
        a = (C.c_float * (2 * self.nstreams))()
        self._check(self.L.qpsk_streams_get_loop_state(self.h, a))
        return np.array(a, np.float32).reshape(-1, 2)

    # ---- bit-level stages (algorithms/ of the reference)
    # ---- transmitters (qpsk.c:225-285)
    def tx_reset(self, nstreams, tx_hz=1550.0):
        self._check(self.L.qpsk_tx_reset(self.h, nstreams, tx_hz))
        self.ntx = nstreams

    def tx_symbols(self, symbols, want_pcm=True, want_baseband=False):
        """symbols: (ntx, nsym) uint8 dibits -> dict(pcm (ntx, nsym*CYCLES) int16, baseband (ntx, nsym*CYCLES, 2))"""
        t = self.torch
        d = self._dev(symbols, t.uint8)
        if d.dim() != 2 or d.shape[0] != getattr(self, "ntx", 0):
            raise ValueError("symbols must be (ntx, nsym) after tx_reset(ntx)")
        n = d.shape[1] * self.cycles
        pcm = self.empty((d.shape[0], n), t.int16) if want_pcm else None
        bb = self.empty((d.shape[0], n, 2), t.float32) if want_baseband else None
        self._check(self.L.qpsk_tx_symbols(self.h, _ptr(d), d.shape[1], _ptr(pcm), _ptr(bb)))
        return dict(pcm=pcm, baseband=bb)

    def crc16(self, packets):
        """packets: (P, nbytes) uint8 -> (P,) uint16 (torch int16 view returned as numpy uint16)"""
        t = self.torch
        d = self._dev(packets, t.uint8)
        out = self.empty((d.shape[0],), t.int16)
        self._check(self.L.qpsk_crc16_batch(self.h, _ptr(d), d.shape[0], d.shape[1], _ptr(out)))
        return out.cpu().numpy().view(np.uint16)

    def interleave(self, packets, direction):
        d = self._dev(packets, self.torch.uint8).clone()
        self._check(self.L.qpsk_interleave_batch(self.h, _ptr(d), d.shape[0], d.shape[1], int(direction)))
        return d

    def scramble(self, symbols):
        d = self._dev(symbols, self.torch.uint8).clone()
        self._check(self.L.qpsk_scramble_batch(self.h, _ptr(d), d.shape[0], d.shape[1]))
        return d

    def sincos_hash(self, first, count):
        h = C.c_ulonglong()
        self._check(self.L.qpsk_selftest_sincos_hash(self.h, first, count, C.byref(h)))
        return h.value


class MultiJob:
    """qpsk_multi of include/qpsk_hip.h: a batch sharded over several devices (repeats allowed), one context + one host thread + two
    streams per shard, results gathered into host arrays.  Plumbing for the tests and bench.py's `gather` key."""

    def __init__(self, devices, **params):
        kw = dict(fs=9600.0, rs=2400.0, frame_size=512, rrc_alpha=0.35, loop_bw=np.float32(TAU / 100.0), min_freq=-1.0, max_freq=1.0,
                  timing_mode=TIMING_HIST, fixed_index=0)
        kw.update(params)
        self.L = load()
        self.params = Params(kw["fs"], kw["rs"], kw["frame_size"], kw["rrc_alpha"], kw["loop_bw"], kw["min_freq"], kw["max_freq"],
                             kw["timing_mode"], kw["fixed_index"])
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        self._check(self.L.qpsk_multi_create(C.byref(h), devs, len(devices), C.byref(self.params)))
        self.h = h
        self.frame_size = kw["frame_size"]
        self.total = 0
        self.nsym = None

    def _check(self, rc):
        if rc != 0:
            raise QpskError("libqpsk_hip error %d: %s" % (rc, self.L.qpsk_last_error().decode()))

    def load(self, frames_host=None, total=None):
        """frames_host: (F, frame_size, 2) float32 numpy array uploaded shard by shard, or None with `total` (device buffers left empty)"""
        if frames_host is not None:
            x = np.ascontiguousarray(frames_host, np.float32)
            total = x.shape[0]
            self._check(self.L.qpsk_multi_load(self.h, total, x.ctypes.data_as(C.c_void_p)))
        else:
            self._check(self.L.qpsk_multi_load(self.h, int(total), None))
        self.total = int(total)
        ctx = C.c_void_p()
        self._check(self.L.qpsk_multi_shard(self.h, 0, None, None, None, C.byref(ctx), None))
        self.nsym = self.L.qpsk_ctx_nsym(ctx)

    def shard(self, r):
        dev, first, count, ctx, d_in = C.c_int32(), C.c_longlong(), C.c_longlong(), C.c_void_p(), C.c_void_p()
        self._check(self.L.qpsk_multi_shard(self.h, r, C.byref(dev), C.byref(first), C.byref(count), C.byref(ctx), C.byref(d_in)))
        return dict(device=dev.value, first=first.value, count=count.value, ctx=ctx, d_in=d_in.value)

    def tune_shard(self, r, **kw):
        """Modem.tune() on shard r's context: tune_shard(1, hist_onepass=1, pipe_g=4); None = the library's choice"""
        ctx = self.shard(r)["ctx"]
        for k, v in kw.items():
            self._check(self.L.qpsk_ctx_set_tuning(ctx, ("QPSK_" + k.upper()).encode(), -1 if v is None else int(v)))

    def inject_status(self, r, code):
        """Test hook: a kernel status code into the status word of shard r's context (qpsk_test_inject_status)"""
        self._check(self.L.qpsk_test_inject_status(self.shard(r)["ctx"], int(code)))

    def hist_state(self, r):
        """Test hook: qpsk_test_hist_state of shard r's context -> [guess, missed, majority, frames, off the majority] (synchronises)"""
        st = (C.c_int32 * 5)()
        self._check(self.L.qpsk_test_hist_state(self.shard(r)["ctx"], st))
        return list(st)

    def last_kernel(self, r):
        """Name of the receive kernel shard r's last begin() launched"""
        return self.L.qpsk_ctx_last_kernel(self.shard(r)["ctx"]).decode()

    def use_device_input(self, r, tensor):
        self._check(self.L.qpsk_multi_use_device_input(self.h, r, C.c_void_p(tensor.data_ptr())))

    def begin(self, slot):
        self._check(self.L.qpsk_multi_rx_begin(self.h, slot))

    def end(self, slot, sym=None, freq=None, phase=None):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
        self._check(self.L.qpsk_multi_rx_end(self.h, slot, p(sym), p(freq), p(phase)))

    def set_acquisition(self, index=None, seed=None):
        """qpsk_multi_set_acquisition: index (total,) int32 and / or seed (total, 2) float32 host arrays for every later begin(); both
        None = back to the contexts' timing.  A later load() clears it."""
        ix = None if index is None else np.ascontiguousarray(index, np.int32)
        sd = None if seed is None else np.ascontiguousarray(seed, np.float32)
        assert ix is None or ix.shape == (self.total,)
        assert sd is None or sd.shape == (self.total, 2)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
        self._check(self.L.qpsk_multi_set_acquisition(self.h, p(ix), p(sd)))

    def set_packed(self, on):
        self._check(self.L.qpsk_multi_set_packed(self.h, int(bool(on))))
        self.packed = bool(on)

    def set_data(self, on):
        """qpsk_multi_set_data: while on, the gathered rows are qpsk_rx_batch_data's decisions instead of the slicer's"""
        self._check(self.L.qpsk_multi_set_data(self.h, int(bool(on))))
        self.data = bool(on)

    def unpack(self, packed):
        out = np.empty((packed.shape[0], self.nsym), np.uint8)
        self._check(self.L.qpsk_unpack_symbols_host(packed.ctypes.data_as(C.c_void_p), packed.shape[0], self.nsym, out.ctypes.data_as(C.c_void_p)))
        return out

    def pinned_outputs(self):
        """(sym, freq, phase) numpy views of page-locked memory (qpsk_host_alloc) for direct mode; kept alive by this object"""
        out = []
        cols = (self.nsym + 3) // 4 if getattr(self, "packed", False) else self.nsym
        for shape, dt in (((self.total, cols), np.uint8), ((self.total,), np.float32), ((self.total,), np.float32)):
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            p = C.c_void_p()
            self._check(self.L.qpsk_host_alloc(C.byref(p), nbytes))
            self._pinned = getattr(self, "_pinned", []) + [p]
            buf = (C.c_uint8 * nbytes).from_address(p.value)
            out.append(np.frombuffer(buf, dtype=dt).reshape(shape))
        return tuple(out)

    def set_direct(self, slot, sym=None, freq=None, phase=None):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)      # noqa: E731
        self._check(self.L.qpsk_multi_set_direct_output(self.h, slot, p(sym), p(freq), p(phase)))

    def outputs(self):
        cols = (self.nsym + 3) // 4 if getattr(self, "packed", False) else self.nsym
        return (np.empty((self.total, cols), np.uint8), np.empty(self.total, np.float32), np.empty(self.total, np.float32))

    def close(self):
        if getattr(self, "h", None):
            self.L.qpsk_multi_destroy(self.h)
            self.h = None
            for p in getattr(self, "_pinned", []):
                self.L.qpsk_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass

