"""AudioAnalyzeFFT256IQ (analyze_fft256iq.h:52-110) batched over channels: the IQ
panadapter spectrum analyser on the GPU (integer q15 path, bit-exact against the CPU restatement kept with the tests)."""
import ctypes as C

import numpy as np
import torch

from . import _lib

# the table names of analyze_fft256iq.h:30-50 -> RDSP_WINDOW_* (include/rdsp.h)
WINDOW_IDS = {"none": 0, "Hanning": 1, "BlackmanHarris": 2, "BlackmanNuttall": 3, "Bartlett": 4, "Blackman": 5,
              "Flattop": 6, "Nuttall": 7, "Welch": 8, "Hamming": 9, "Cosine": 10, "Tukey": 11}
WINDOWS = {"none": 0, **{f"AudioWindow{k}256": v for k, v in WINDOW_IDS.items() if v}}


def window_q15(window_id, n=256):
    """The q15 table the Teensy Audio library holds under that name (int16 [n])."""
    w = np.zeros(n, np.int16)
    _lib.load().rdsp_window_q15_n(int(window_id), int(n), w.ctypes.data_as(C.POINTER(C.c_int16)))
    return w


class _Analyzer(_lib.Handle):
    """What the two integer analysers share.  A subclass gives the symbol prefix (rdsp_<prefix>_*), the bins of an output
    row, the taps of a window table, its window names, and `_input`: what update() checks of its input and passes on."""
    _prefix = _bins = _taps = _windows = None

    def _fn(self, name):
        return getattr(self.lib, f"rdsp_{self._prefix}_{name}")

    def _open(self, n_channels, *settings):
        self.n_channels = n_channels
        self.output = None      # uint16 [n_channels, bins] of the latest completed spectrum
        self._flag = False
        self._destroy = f"rdsp_{self._prefix}_destroy"
        self._create(f"rdsp_{self._prefix}_create", n_channels, *settings)

    def averageTogether(self, n):   # FFTIQ.h:88-91; INO:148 (the 1024-point analyser of the library ignores it)
        _lib.check(self._fn("averageTogether")(self.h, int(n)))

    def windowFunction(self, window):
        """FFTIQ.h:93-95: a table name, an int16 array of q15 taps (the reference's own argument) or None."""
        if window is None or isinstance(window, str):
            _lib.check(self._fn("windowFunction")(self.h, self._windows[window or "none"]))
            return
        w = np.ascontiguousarray(window, dtype=np.int16)
        assert w.shape == (self._taps,)
        _lib.check(self._fn("windowFunction_table")(self.h, w.ctypes.data_as(C.POINTER(C.c_int16))))

    def update(self, x, stream=None):
        """x: the int16 cuda tensor the class describes; returns uint16-valued int16-storage tensor [n_channels, n_out, bins]
        (viewed as uint16 via .cpu().numpy().view('uint16'))."""
        nb, layout = self._input(x)
        n_out = self._fn("outputs_for")(self.h, nb)
        out = torch.zeros((self.n_channels, max(n_out, 1), self._bins), dtype=torch.int16, device=x.device)
        got = C.c_int()
        _lib.check(self._fn("update")(self.h, C.c_void_p(x.data_ptr()), *layout, nb, C.c_void_p(out.data_ptr()), out.shape[1],
                                      C.byref(got), _lib.stream_ptr(stream)))
        out = out[:, :got.value]
        if got.value:
            self.output = out[:, -1]
            self._flag = True
        return out

    def available(self):  # FFTIQ.h:62-68
        f, self._flag = self._flag, False
        return f

    def _row(self, channel):
        return np.ascontiguousarray(self.output[channel].cpu().numpy().view(np.uint16))

    def read(self, channel, binFirst, binLast=None):  # FFTIQ.h:70-73 and :75-86
        if self.output is None:
            return 0.0
        row = self._row(channel).ctypes.data_as(C.POINTER(C.c_uint16))
        if binLast is None:
            return float(self._fn("read")(row, int(binFirst)))
        return float(self._fn("read_range")(row, int(binFirst), int(binLast)))


class AnalyzeFFT256IQ(_Analyzer):
    """`AnalyzeFFT256IQ(n)` is the reference's constructor (FFTIQ.h:55-58): BlackmanNuttall256, naverage 8.
    update(iq): int16 cuda tensor [n_channels, n_blocks*128, 2]."""
    _prefix, _bins, _taps, _windows = "spectrum", 256, 256, WINDOWS

    def __init__(self, n_channels, naverage=8, window="AudioWindowBlackmanNuttall256", device=0):
        self._open(n_channels, device, naverage, WINDOWS[window])

    def _input(self, iq):
        assert iq.is_cuda and iq.dtype == torch.int16 and iq.is_contiguous() and iq.shape[0] == self.n_channels
        return iq.shape[1] // 128, (iq.stride(0) // 2,)
