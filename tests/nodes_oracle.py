"""The oracle's restatements of the graph's nodes (oracle/rdsp_oracle.c: the two integer analysers, the float and the
Teensy fixed-point biquad cascades) as the tests call them: every orc_* binding of these objects stated once, and the small
drivers that run one channel through them.  A plain module like engine_sources_model.py; test_spectrum, test_audio_nodes,
test_firmware_tables, test_firmware_kat, test_boundary_c and golden/make_golden.py import from here."""
import ctypes as C

import numpy as np

F32P, I16P, I32P, U16P = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int32), C.POINTER(C.c_uint16)


class OrcBiquad(C.Structure):
    _fields_ = [("n_stages", C.c_int), ("coef", C.c_float * 20), ("state", C.c_float * 16)]


class OrcTeensyBiquad(C.Structure):
    _fields_ = [("chained", C.c_int * 4), ("coef", (C.c_int32 * 5) * 4), ("x1", C.c_int16 * 4), ("x2", C.c_int16 * 4),
                ("y1", C.c_int16 * 4), ("y2", C.c_int16 * 4), ("sum", C.c_int32 * 4)]


_BQ, _TBQ = C.POINTER(OrcBiquad), C.POINTER(OrcTeensyBiquad)
# name: (restype, argtypes); restype None leaves ctypes' int
_ORC = {
    "orc_fft256iq_create": (C.c_void_p, [C.c_int, C.c_int]),
    "orc_fft256iq_destroy": (None, [C.c_void_p]),
    "orc_fft256iq_update": (C.c_int, [C.c_void_p, I16P, I16P]),
    "orc_fft256iq_output": (U16P, [C.c_void_p]),
    "orc_fft256iq_averageTogether": (None, [C.c_void_p, C.c_int]),
    "orc_fft256iq_windowFunction": (None, [C.c_void_p, C.c_int]),
    "orc_fft256iq_windowFunction_table": (None, [C.c_void_p, I16P]),
    "orc_fft256iq_read": (C.c_float, [C.c_void_p, C.c_uint]),
    "orc_fft256iq_read_range": (C.c_float, [C.c_void_p, C.c_uint, C.c_uint]),
    "orc_cfft_radix4_q15_256": (None, [I16P]),
    "orc_cfft_radix4_q15_n": (None, [I16P, C.c_int]),
    "orc_window_q15": (None, [C.c_int, I16P]),
    "orc_window_q15_n": (None, [C.c_int, C.c_int, I16P]),
    "orc_twiddle_q15_4096": (None, [I16P]),
    "orc_sqrt_guess_table": (U16P, None),
    "orc_sqrt_uint32": (C.c_uint32, [C.c_uint32]),
    "orc_sqrt_uint32_approx": (C.c_uint32, [C.c_uint32]),
    "orc_fft1024_create": (C.c_void_p, [C.c_int]),
    "orc_fft1024_destroy": (None, [C.c_void_p]),
    "orc_fft1024_update": (C.c_int, [C.c_void_p, I16P]),
    "orc_fft1024_output": (U16P, [C.c_void_p]),
    "orc_fft1024_windowFunction_table": (None, [C.c_void_p, I16P]),
    "orc_design_butter_bp8": (None, [C.c_double, C.c_double, C.c_double, F32P]),
    "orc_biquad_design": (None, [C.c_int, C.c_double, C.c_double, C.c_double, F32P]),
    "orc_set_audio_iir": (None, [C.c_void_p, C.c_int, C.c_double, C.c_double]),
    "orc_chain_iir_coeffs": (F32P, [C.c_void_p]),
    "orc_biquad_init": (None, [_BQ, C.c_int, F32P]),
    "orc_biquad_run": (None, [_BQ, F32P, C.c_int]),
    "orc_biquad_set_stage": (None, [_BQ, C.c_int, F32P]),
    "orc_float_to_q15": (None, [F32P, I16P, C.c_uint32]),
    "orc_teensy_biquad_init": (None, [_TBQ]),
    "orc_teensy_biquad_setCoefficients_int": (None, [_TBQ, C.c_int, I32P]),
    "orc_teensy_biquad_setCoefficients": (None, [_TBQ, C.c_int, C.POINTER(C.c_double)]),
    "orc_teensy_biquad_design": (None, [C.c_int, C.c_float, C.c_float, C.c_float, I32P]),
    "orc_teensy_biquad_update": (None, [_TBQ, I16P, C.c_int]),
}


def _bind(lib):
    """the oracle library with the bindings above (again: any binding a test changed for itself is back)"""
    for name, (res, args) in _ORC.items():
        fn = getattr(lib, name)
        if res is not None:
            fn.restype = res
        if args is not None:
            fn.argtypes = args
    return lib


def _olib(oracle):
    return _bind(oracle.load())


def oracle_spectra(lib, iq, naverage, window):
    """iq int16 [n, 2] (n multiple of 128) -> list of uint16[256] spectra, in order.  window: an id, or an int16
    table handed over the way the reference does (windowFunction(const int16_t *), FFTIQ.h:93)."""
    if isinstance(window, np.ndarray):
        s = lib.orc_fft256iq_create(naverage, 0)
        lib.orc_fft256iq_windowFunction_table(s, np.ascontiguousarray(window, np.int16).ctypes.data_as(I16P))
    else:
        s = lib.orc_fft256iq_create(naverage, window)
    outs = []
    i = np.ascontiguousarray(iq[:, 0])
    q = np.ascontiguousarray(iq[:, 1])
    for b in range(len(iq) // 128):
        if lib.orc_fft256iq_update(s, i[b * 128:].ctypes.data_as(I16P), q[b * 128:].ctypes.data_as(I16P)):
            outs.append(np.ctypeslib.as_array(lib.orc_fft256iq_output(s), (256,)).copy())
    lib.orc_fft256iq_destroy(s)
    return outs


def oracle_fft1024(lib, x, window):
    s = lib.orc_fft1024_create(window)
    outs = []
    for b in range(len(x) // 128):
        blk = np.ascontiguousarray(x[b * 128:(b + 1) * 128], np.int16)
        if lib.orc_fft1024_update(s, blk.ctypes.data_as(I16P)):
            outs.append(np.ctypeslib.as_array(lib.orc_fft1024_output(s), (512,)).copy())
    lib.orc_fft1024_destroy(s)
    return np.stack(outs) if outs else np.zeros((0, 512), np.uint16)


def oracle_biquad(lib, coef20, x):
    """float DF1 cascade of the oracle over a float array (fresh state)"""
    b = OrcBiquad()
    _bind(lib)
    c = np.ascontiguousarray(coef20, np.float32)
    lib.orc_biquad_init(C.byref(b), 4, c.ctypes.data_as(F32P))
    y = np.ascontiguousarray(x, np.float32).copy()
    lib.orc_biquad_run(C.byref(b), y.ctypes.data_as(F32P), len(y))
    return y


class TeensyBiquadOracle:
    """the oracle's restatement of the Teensy library's AudioFilterBiquad (fixed point), one channel"""
    KIND = {"lowpass": 0, "highpass": 1, "bandpass": 2, "notch": 3}

    def __init__(self, lib, fs=44100.0):
        self.lib, self.fs, self.o = _bind(lib), fs, OrcTeensyBiquad()
        lib.orc_teensy_biquad_init(C.byref(self.o))

    def set(self, stage, kind, f, q):
        c5 = np.zeros(5, np.int32)
        self.lib.orc_teensy_biquad_design(self.KIND[kind], f, q, self.fs, c5.ctypes.data_as(I32P))
        self.lib.orc_teensy_biquad_setCoefficients_int(C.byref(self.o), stage, c5.ctypes.data_as(I32P))
        return c5

    def setCoefficients(self, stage, c5):
        c = np.ascontiguousarray(c5, np.float64)
        self.lib.orc_teensy_biquad_setCoefficients(C.byref(self.o), stage, c.ctypes.data_as(C.POINTER(C.c_double)))

    def update(self, x):
        """x int16 [n] (n a multiple of 128): block by block like the audio interrupt; returns the filtered int16"""
        y = np.ascontiguousarray(x, np.int16).copy()
        for b in range(len(y) // 128):
            blk = y[b * 128:(b + 1) * 128]
            self.lib.orc_teensy_biquad_update(C.byref(self.o), blk.ctypes.data_as(I16P), 128)
        return y
