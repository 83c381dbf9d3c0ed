"""Channelizer: a wide IQ source split once into M sub-bands at D2 x 44100 Hz that all its receivers share -- a ctypes mirror
of the rdsp_channelizer_* entry points of include/rdsp.h, which has the definition.  The source rows are those
Engine.update_sources() takes, in the same four formats; the sub-band rows are SRC_F32 sources of an Engine at the integer rate
D2, and place() says which row and which residual frequency a station gets."""
import ctypes as C

import numpy as np

from ._lib import Handle, check, load, stream_ptr
from .engine import SRC_F32, SRC_S8, SRC_S16, SRC_U8, _src_dtype  # noqa: F401

_F32P = C.POINTER(C.c_float)
SUBBANDS = (8, 16, 32, 64)


def rate(P, Q, D2):
    """(P1, Q1): P / (Q D2) in lowest terms, the ratio of the source rate to the sub-band rate (host only)"""
    p1, q1 = C.c_int(), C.c_int()
    check(load().rdsp_channelizer_rate(int(P), int(Q), int(D2), C.byref(p1), C.byref(q1)))
    return p1.value, q1.value


def taps(P, Q, D2):
    """the float32 prototype, [16 ceil(P1 / Q1) Q1]: branch r is taps[r::Q1] (host only)"""
    P1, Q1 = rate(P, Q, D2)
    h = np.zeros(16 * -(-P1 // Q1) * Q1, np.float32)
    check(load().rdsp_channelizer_taps(int(P), int(Q), int(D2), h.ctypes.data_as(_F32P)))
    return h


def twiddles(M):
    """float32 [M, 2]: (cos, sin) of 2 pi m / M as the kernel uses them (host only)"""
    t = np.zeros((int(M) if M in SUBBANDS else 1, 2), np.float32)
    check(load().rdsp_channelizer_twiddles(int(M), t.ctypes.data_as(_F32P)))
    return t


def place(P, Q, M, station_hz):
    """a station (Hz from the band centre) -> (subband, residual_hz): the sub-band nearest to it and where it lies in that row.
    An array of stations gives (int array, float64 array), element for element what the scalar call gives (host only)"""
    if np.ndim(station_hz) == 0:
        k, r = C.c_int(), C.c_double()
        check(load().rdsp_channelizer_place(int(P), int(Q), int(M), float(station_hz), C.byref(k), C.byref(r)))
        return k.value, r.value
    st = np.asarray(station_hz, np.float64)
    k0, _ = place(P, Q, M, 0.0)                                # the scalar call's checks of P, Q and M
    assert k0 == 0
    fs = (float(P) * 44100.0) / float(Q)
    if not np.all(np.abs(st) < fs / 2.0):                       # NaN compares false
        place(P, Q, M, float(st.reshape(-1)[np.argmax(~(np.abs(st.reshape(-1)) < fs / 2.0))]))   # raises with the library's text
    spacing = fs / float(M)
    x = st / spacing
    kk = np.trunc(x)
    kk = kk + np.sign(x) * (np.abs(x - kk) >= 0.5)              # half away from zero; x - trunc(x) is exact
    return np.mod(kk.astype(np.int64), int(M)).astype(np.int64), st - kk * spacing


class Channelizer(Handle):
    _destroy = "rdsp_channelizer_destroy"

    def __init__(self, n_sources, P, Q, M, D2, fmt=SRC_S16, max_blocks_per_call=64, device=0):
        self._create("rdsp_channelizer_create", int(n_sources), int(device), int(P), int(Q), int(M), int(D2), int(fmt), int(max_blocks_per_call))
        self.n_sources, self.M, self.D2, self.fmt = int(n_sources), int(M), int(D2), int(fmt)
        p, q = C.c_int(), C.c_int()
        check(self.lib.rdsp_channelizer_source_rate(self.h, C.byref(p), C.byref(q)))
        self.P, self.Q = p.value, q.value

    def reset(self, stream=None):
        check(self.lib.rdsp_channelizer_reset(self.h, stream_ptr(stream)))

    def source_pairs(self, n_blocks):
        """pairs of every source row the NEXT update(..., n_blocks) consumes"""
        return int(self.lib.rdsp_channelizer_source_pairs(self.h, int(n_blocks)))

    def place(self, station_hz):
        return place(self.P, self.Q, self.M, station_hz)

    def update(self, d_src, n_blocks, out=None, stream=None):
        """d_src: torch [n_sources, n, 2] in the channelizer's format on its device, possibly a view into a longer buffer (rows
        any whole number of pairs apart); the first source_pairs(n_blocks) pairs of every row are taken.  Returns float32
        [n_sources M, n_blocks 128 D2, 2], row src M + k sub-band k of source src: a view of `out` if one is given (float32
        [n_sources M, >= n_blocks 128 D2, 2], rows an even number of pairs apart), which an Engine takes as SRC_F32 rows."""
        import torch
        nsrc, n, two = d_src.shape
        n_blocks, need = int(n_blocks), self.source_pairs(n_blocks)
        assert d_src.dtype == _src_dtype(self.fmt), f"the channelizer's format {self.fmt} takes {_src_dtype(self.fmt)} rows, not {d_src.dtype}"
        assert nsrc == self.n_sources and two == 2 and n >= need, "d_src holds fewer pairs than source_pairs(n_blocks)"
        assert n == 0 or (d_src.stride(2) == 1 and d_src.stride(1) == 2 and d_src.stride(0) % 2 == 0)
        n_out, rows = n_blocks * 128 * self.D2, nsrc * self.M
        if out is None:
            out = torch.empty((rows, n_out, 2), dtype=torch.float32, device=d_src.device)
        assert out.dtype == torch.float32 and out.shape[0] == rows and out.shape[1] >= n_out and out.shape[2] == 2
        assert out.shape[1] == 0 or (out.stride(2) == 1 and out.stride(1) == 2 and out.stride(0) % 2 == 0)
        stride = d_src.stride(0) // 2 if nsrc > 1 else max(n, need)
        check(self.lib.rdsp_channelizer_update(self.h, C.c_void_p(d_src.data_ptr()), stride, n_blocks, C.c_void_p(out.data_ptr()),
                                               out.stride(0) // 2, stream_ptr(stream)))
        return out[:, :n_out]
