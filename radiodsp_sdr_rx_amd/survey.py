"""Band survey: Welch-averaged power spectra of shared IQ source rows and the station finder -- a ctypes mirror of the
rdsp_survey_* entry points of include/rdsp.h, which has the definition.  The rows are those Engine.update_sources() takes, in
the same four formats; find_stations() turns a spectrum row into the station_hz that Engine.tune() wants."""
import ctypes as C

import numpy as np

from ._lib import Handle, check, load, stream_ptr
from .engine import SRC_F32, SRC_S8, SRC_S16, SRC_U8, _src_dtype  # noqa: F401

_F32P, _F64P = C.POINTER(C.c_float), C.POINTER(C.c_double)


def window(fft_n):
    """the float32 taps every frame is multiplied by: the periodic 4-term Blackman-Harris window over its sum (host only)"""
    w = np.zeros(int(fft_n) if fft_n in (1024, 4096) else 1, np.float32)
    check(load().rdsp_survey_window(int(fft_n), w.ctypes.data_as(_F32P)))
    return w


def rows_between(fft_n, navg, pairs_before, pairs):
    """rows per source that `pairs` pairs complete behind `pairs_before` pairs (host only)"""
    r = load().rdsp_survey_rows_between(int(fft_n), int(navg), int(pairs_before), int(pairs))
    if r < 0:
        check(r)
    return r


def bin_hz(fft_n, P, Q, j):
    """Hz from the band centre of index j of a row, the band at 44100 P / Q Hz"""
    return float(load().rdsp_survey_bin_hz(int(fft_n), int(P), int(Q), int(j)))


def find_stations(row, P, Q, min_db_over_floor=20.0, min_spacing_hz=1000.0, max_out=64):
    """row: one spectrum row (float32 [fft_n], host) -> (station_hz float64 [n], power float32 [n]), strongest first (host only)"""
    row = np.ascontiguousarray(row, np.float32)
    assert row.ndim == 1
    hz, pw = np.zeros(max(int(max_out), 1), np.float64), np.zeros(max(int(max_out), 1), np.float32)
    n = load().rdsp_survey_find_stations(row.ctypes.data_as(_F32P), row.size, int(P), int(Q), float(min_db_over_floor),
                                         float(min_spacing_hz), int(max_out), hz.ctypes.data_as(_F64P), pw.ctypes.data_as(_F32P))
    if n < 0:
        check(n)
    return hz[:n].copy(), pw[:n].copy()


class Survey(Handle):
    _destroy = "rdsp_survey_destroy"

    def __init__(self, n_sources, fft_n=4096, navg=8, fmt=SRC_S16, max_pairs_per_call=1 << 22, device=0):
        self._create("rdsp_survey_create", int(n_sources), int(device), int(fft_n), int(navg), int(fmt), int(max_pairs_per_call))
        self.n_sources, self.fft_n, self.navg, self.fmt = int(n_sources), int(fft_n), int(navg), int(fmt)

    def reset(self, stream=None):
        check(self.lib.rdsp_survey_reset(self.h, stream_ptr(stream)))

    def rows_for(self, pairs):
        """rows per source the NEXT update of `pairs` pairs completes"""
        return int(self.lib.rdsp_survey_rows_for(self.h, int(pairs)))

    def axis_hz(self, P, Q):
        """Hz from the band centre of every index of a row, the band at 44100 P / Q Hz"""
        return np.array([bin_hz(self.fft_n, P, Q, j) for j in range(self.fft_n)])

    def update(self, d_src, pairs=None, out=None, stream=None):
        """d_src: torch [n_sources, n, 2] in the survey's format on its device, possibly a view into a longer buffer (rows any
        whole number of pairs apart); the first `pairs` (default n) pairs of every row are taken.  Returns float32
        [n_sources, rows, fft_n], rows = rows_for(pairs), a view of `out` if one is given (float32 [n_sources, >= rows, fft_n])."""
        import torch
        nsrc, n, two = d_src.shape
        pairs = n if pairs is None else int(pairs)
        assert d_src.dtype == _src_dtype(self.fmt), f"the survey's format {self.fmt} takes {_src_dtype(self.fmt)} rows, not {d_src.dtype}"
        assert nsrc == self.n_sources and two == 2 and 0 <= pairs <= n
        assert n == 0 or (d_src.stride(2) == 1 and d_src.stride(1) == 2 and d_src.stride(0) % 2 == 0)
        rows = self.rows_for(pairs)
        if out is None:
            out = torch.empty((nsrc, rows, self.fft_n), dtype=torch.float32, device=d_src.device)
        assert out.dtype == torch.float32 and out.shape[0] == nsrc and out.shape[1] >= rows and out.shape[2] == self.fft_n
        assert out.stride(2) == 1 and (out.shape[1] == 0 or out.stride(1) == self.fft_n)
        stride = d_src.stride(0) // 2 if nsrc > 1 else max(n, pairs)
        rows_stride = out.stride(0) if nsrc > 1 and out.shape[1] > 0 else out.shape[1] * self.fft_n
        got = C.c_int()
        check(self.lib.rdsp_survey_update(self.h, C.c_void_p(d_src.data_ptr()), stride, pairs, C.c_void_p(out.data_ptr()), rows_stride,
                                          C.byref(got), stream_ptr(stream)))
        assert got.value == rows
        return out[:, :rows]
