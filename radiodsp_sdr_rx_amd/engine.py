"""`AudioSDR SDR;` of the reference sketch (RadioDSP_SDR_RX.ino:54) for many receivers on one GPU: a ctypes mirror of
the rdsp_engine_* entry points of include/rdsp.h.  Method names, argument meaning and numbering are the engine's
(INO:117-139, RDSP_controls.h:149-423); the arithmetic is csrc/rdsp_engine.hip's (its stage files rdsp_engine_front / _hilbert / _tail.hip)."""
import ctypes as C

import numpy as np

from ._lib import Handle, check, load, stream_ptr

LSBmode, USBmode, CW_LSBmode, CW_USBmode, AMmode, SAMmode = range(6)      # as the compiled tuningMode() passes them
NFMmode = 7                                                              # RDSP_ENGINE_MODE_NFM: this build's own, behind enable_fm()
audioAM, audioCW, audio2100, audio2700, audio3100, audioNone = 0, 1, 3, 6, 8, 10
AGCoff, AGCfast, AGCmedium, AGCslow = range(4)
SRC_S16, SRC_U8, SRC_S8, SRC_F32 = range(4)                              # RDSP_SRC_*: what the source rows hold
DCS_ANY, DCS_INVERTED = 0xFFFF, 0x8000                                   # RDSP_DCS_*: set_dcs_codes
NOISE_OFF, NOISE_MEASURE, NOISE_GATE = range(3)                          # RDSP_NOISE_*: set_noise_squelch
_F32P = C.POINTER(C.c_float)


def _src_dtype(fmt):
    import torch
    return (torch.int16, torch.uint8, torch.int8, torch.float32)[fmt]


class Engine(Handle):
    _destroy = "rdsp_engine_destroy"

    def __init__(self, n_channels, max_blocks_per_call=64, device=0, tables=None):
        self._create("rdsp_engine_create", n_channels, device, max_blocks_per_call)
        self.n_channels, self.max_blocks = n_channels, max_blocks_per_call
        self._last_blocks = 0   # of the last update made through this object: read_voice's and pack_voice's default
        if tables is not None:
            self.load_tables(*tables)

    def load_tables(self, biquad_sets, hilbert64):
        b = np.ascontiguousarray(biquad_sets, np.float32).reshape(-1)
        h = np.ascontiguousarray(hilbert64, np.float32).reshape(-1)
        assert b.size == 300 and h.size == 64
        check(self.lib.rdsp_engine_load_tables(self.h, b.ctypes.data_as(_F32P), h.ctypes.data_as(_F32P)))

    def sketch_setup(self):
        """INO:120-139 in the sketch's order"""
        self.enableAGC(); self.setAGCmode(AGCmedium); self.disableALSfilter(); self.disableNoiseBlanker()
        self.setInputGain(1.0); self.setOutputGain(0.5); self.setIQgainBalance(1.020)
        self.enableAudioFilter(); self.setAudioFilter(audio2700)
        return self.setDemodMode(LSBmode)

    def setDemodMode(self, mode):
        return float(self.lib.rdsp_engine_setDemodMode(self.h, int(mode)))

    def update(self, d_iq, out=None, stream=None):
        """d_iq: torch int16 [n_channels, n, 2] on the engine's device, n a multiple of 128 -> int16 [n_channels, n, 2]"""
        import torch
        nch, n, two = d_iq.shape
        assert nch == self.n_channels and two == 2 and n % 128 == 0 and d_iq.dtype == torch.int16 and d_iq.is_contiguous()
        if out is None:
            out = torch.empty_like(d_iq)
        check(self.lib.rdsp_engine_update(self.h, d_iq.data_ptr(), n, n // 128, out.data_ptr(), n, stream_ptr(stream)))
        self._last_blocks = n // 128
        return out

    def set_sources(self, n_sources, source_of_channel):
        """receiver ch listens to source row source_of_channel[ch] of the rows update_sources() takes"""
        assert len(source_of_channel) == self.n_channels
        a = (C.c_int * self.n_channels)(*[int(x) for x in source_of_channel])
        check(self.lib.rdsp_engine_set_sources(self.h, int(n_sources), a))
        self.n_sources = int(n_sources)

    def set_source_decimation(self, D, gain=1.0):
        """the source rows are at D x 44100 Hz (D = 1 ... 64): update_sources() tunes, low-passes (16 D taps, times gain) and
        decimates by D.  After set_sources()."""
        check(self.lib.rdsp_engine_set_source_decimation(self.h, int(D), float(gain)))

    def source_decimation(self):
        return int(self.lib.rdsp_engine_source_decimation(self.h))

    def set_source_rate(self, P, Q, gain=1.0):
        """the source rows are at 44100 P / Q Hz (P / Q reduced first; then 1 <= Q <= 441, Q <= P <= 64 Q): update_sources()
        tunes, low-passes and resamples by Q / P.  Q = 1 after reduction is set_source_decimation(P, gain).  After
        set_sources()."""
        check(self.lib.rdsp_engine_set_source_rate(self.h, int(P), int(Q), float(gain)))

    def source_rate(self):
        """(P, Q) in lowest terms; (D, 1) for an integer rate"""
        p, q = C.c_int(), C.c_int()
        check(self.lib.rdsp_engine_source_rate(self.h, C.byref(p), C.byref(q)))
        return p.value, q.value

    def source_pairs(self, n_blocks):
        """pairs of every source row the NEXT update_sources(..., n_blocks=n_blocks) consumes"""
        return int(self.lib.rdsp_engine_source_pairs(self.h, int(n_blocks)))

    def set_source_format(self, fmt):
        """the source rows are SRC_S16 (default), SRC_U8 (offset binary, .cu8), SRC_S8 (.cs8) or SRC_F32 (full scale +-1.0): one
        format per engine, read in place by update_sources().  A setting (kept by reset and the rate setters); another format
        begins another stream (source histories and frac zeroed, phases kept).  After set_sources()."""
        check(self.lib.rdsp_engine_set_source_format(self.h, int(fmt)))

    def source_format(self):
        return int(self.lib.rdsp_engine_source_format(self.h))

    def tune(self, first_channel, station_hz):
        """receivers first_channel ... get the stations station_hz (Hz from their source stream's centre, |f| < D x 22050)"""
        st = np.ascontiguousarray(np.atleast_1d(station_hz), np.float64)
        check(self.lib.rdsp_engine_tune(self.h, int(first_channel), st.size, st.ctypes.data_as(C.POINTER(C.c_double))))

    def update_sources(self, d_src, out=None, stream=None, n_blocks=None):
        """d_src: torch int16 (uint8 / int8 / float32 under the matching set_source_format) [n_sources, n D, 2] on the engine's
        device, n a multiple of 128, D the source decimation ->
        int16 [n_channels, n, 2]: every receiver tuned to its station in its source row (and for D > 1 low-passed and
        decimated), then update().  With n_blocks: n = n_blocks x 128 outputs from the first source_pairs(n_blocks) pairs of
        every row of d_src, which may be a view into a longer buffer (rows any whole number of pairs apart); required with a
        rational rate (set_source_rate)."""
        nsrc, n_in, two = d_src.shape
        import torch
        fmt = self.source_format()
        dtype = _src_dtype(fmt)
        assert d_src.dtype == dtype, f"the engine's source format {fmt} takes {dtype} rows, not {d_src.dtype}"
        if n_blocks is not None:
            n_blocks, need = int(n_blocks), self.source_pairs(n_blocks)
            assert two == 2 and n_in >= need, "d_src holds fewer pairs than source_pairs(n_blocks)"
            assert d_src.stride(2) == 1 and d_src.stride(1) == 2 and d_src.stride(0) % 2 == 0
            stride = d_src.stride(0) // 2 if nsrc > 1 else max(n_in, need)
        else:
            D = self.source_decimation()                     # 0 while the rate is rational
            assert D >= 1, "a rational source rate is set: pass n_blocks"
            n = n_in // D
            assert two == 2 and n_in == n * D and n % 128 == 0 and d_src.is_contiguous()
            n_blocks, stride = n // 128, n_in
        assert nsrc >= getattr(self, "n_sources", 0), "fewer source rows than set_sources named"
        n = n_blocks * 128
        if out is None:
            out = torch.empty((self.n_channels, n, 2), dtype=torch.int16, device=d_src.device)
        check(self.lib.rdsp_engine_update_source_samples(self.h, d_src.data_ptr(), stride, n_blocks, out.data_ptr(), n, stream_ptr(stream)))
        self._last_blocks = n_blocks
        return out

    def enable_meter(self):
        """the signal meter from the next update on (include/rdsp.h, "signal meter and squelch"); again: a no-op.  Takes no
        stream and waits for the device."""
        check(self.lib.rdsp_engine_enable_meter(self.h))

    def meter_enabled(self):
        return bool(self.lib.rdsp_engine_meter_enabled(self.h))

    def set_meter(self, attack=0.5, decay=0.0625):
        """the level's coefficients of the selected group, each in (0, 1]"""
        check(self.lib.rdsp_engine_set_meter(self.h, float(attack), float(decay)))

    def set_squelch(self, open_ms, close_ms, hang_blocks=0):
        """the selected group's gate: opens at a level >= open_ms, stays open while >= close_ms and for hang_blocks blocks
        after; mean squares of the demodulated audio (ms_of_db gives them from dB re a full-scale sine)"""
        check(self.lib.rdsp_engine_set_squelch(self.h, float(open_ms), float(close_ms), int(hang_blocks)))

    def disable_squelch(self):
        check(self.lib.rdsp_engine_disable_squelch(self.h))

    def read_meter(self, n_blocks, stream=None):
        """the last call's records -> (level float32, peak float32, open uint8), each [n_channels, n_blocks] on the device"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        level, peak = (torch.empty((self.n_channels, n), dtype=torch.float32, device=dev) for _ in range(2))
        gate = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        check(self.lib.rdsp_engine_read_meter(self.h, n, level.data_ptr(), n, peak.data_ptr(), n, gate.data_ptr(), n, stream_ptr(stream)))
        return level, peak, gate

    def active(self, stream=None):
        """the receivers whose gate was open in a block of the last call -> (int32 tensor on the device, ascending, count)"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        lst = torch.empty(self.n_channels, dtype=torch.int32, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        check(self.lib.rdsp_engine_active(self.h, lst.data_ptr(), cnt.data_ptr(), stream_ptr(stream)))
        if stream is not None:   # the count is read on the host: wait for the caller's stream, whichever form it came in
            (stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(stream)).synchronize()
        n = int(cnt.item())
        return lst[:n], n

    def meter(self):
        """[n_channels, 4] on the host: level, the last block's mean square, the last block's peak, open"""
        o = np.zeros((self.n_channels, 4), np.float32)
        check(self.lib.rdsp_engine_get_meter(self.h, o.ctypes.data_as(_F32P), None))
        return o

    def read_demod(self, n_blocks, stream=None):
        """the last call's demodulated float rows (behind the IF filter and the detector, in front of the audio filter, AGC
        and ALS: what the meter measures) -> float32 [n_channels, n_blocks x 128] on the device.  Works without the meter."""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks) * 128
        out = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        check(self.lib.rdsp_engine_read_demod(self.h, int(n_blocks), out.data_ptr(), n, stream_ptr(stream)))
        return out

    def pack_active(self, lr, n_blocks=None, capacity=None, stream=None):
        """the open blocks of the last call, dense and mono (include/rdsp.h, "packed audio of the open receivers"): lr is the
        tensor update() returned or filled -> (audio int16 [written, 128], records int32 [written, 2] = channel, block inside
        the call, both on the device; needed).  n_blocks: the call's first so many blocks (default: all of lr's); capacity:
        room for so many blocks (default: a sizing call first, then exactly `needed`)."""
        import torch
        assert lr.dtype == torch.int16 and lr.dim() == 3 and lr.shape[0] == self.n_channels and lr.shape[2] == 2
        assert lr.stride(2) == 1 and lr.stride(1) == 2 and (lr.stride(0) % 2 == 0 or self.n_channels == 1)
        stride = lr.stride(0) // 2 if self.n_channels > 1 else lr.shape[1]
        n = lr.shape[1] // 128 if n_blocks is None else int(n_blocks)
        cnt = torch.empty(2, dtype=torch.int32, device=lr.device)
        s = stream_ptr(stream)

        def counts():   # read on the host: wait for the caller's stream, whichever form it came in, as active() does
            if stream is not None:
                (stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(stream)).synchronize()
            return [int(v) for v in cnt.tolist()]
        if capacity is None:
            check(self.lib.rdsp_engine_pack_active(self.h, lr.data_ptr(), stride, n, None, None, 0, cnt.data_ptr(), s))
            capacity = counts()[0]
        capacity = int(capacity)
        audio = torch.empty((capacity, 128), dtype=torch.int16, device=lr.device)
        records = torch.empty((capacity, 2), dtype=torch.int32, device=lr.device)
        check(self.lib.rdsp_engine_pack_active(self.h, lr.data_ptr(), stride, n, audio.data_ptr() if capacity else None,
                                               records.data_ptr() if capacity else None, capacity, cnt.data_ptr(), s))
        needed, written = counts()
        return audio[:written], records[:written], needed

    def enable_voice(self, R):
        """voice-rate audio from the next update on (include/rdsp.h, "voice-rate audio"): the left words of every receiver's
        output row, behind the gate, low-passed and decimated by R = 2 or 4 on the device.  One R per engine; the same R again:
        a no-op.  Takes no stream and waits for the device; does not need the meter."""
        check(self.lib.rdsp_engine_enable_voice(self.h, int(R)))

    @property
    def voice_rate(self):
        """R, or 0 while the stage is off"""
        return int(self.lib.rdsp_engine_voice_rate(self.h))

    def read_voice(self, n_blocks=None, stream=None):
        """the last call's voice rows -> int16 [n_channels, n_blocks x 128 / R] on the device (default: the blocks of the last
        update() or update_sources() of this object)"""
        import torch
        R = self.voice_rate
        if n_blocks is None:
            n_blocks = self._last_blocks
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks) * 128 // max(R, 1)
        out = torch.empty((self.n_channels, n), dtype=torch.int16, device=dev)
        check(self.lib.rdsp_engine_read_voice(self.h, int(n_blocks), out.data_ptr(), n, stream_ptr(stream)))
        return out

    def pack_voice(self, n_blocks=None, capacity=None, stream=None):
        """the open blocks of the last call's voice rows, dense (include/rdsp.h, "voice-rate audio"): pack_active for blocks
        of 128 / R words -> (audio int16 [written, 128 // R], records int32 [written, 2] = channel, block inside the call, both
        on the device; needed).  Needs the meter and the stage.  n_blocks: the call's first so many blocks (default: all);
        capacity: room for so many blocks (default: a sizing call first, then exactly `needed`)."""
        import torch
        R = self.voice_rate
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = self._last_blocks if n_blocks is None else int(n_blocks)
        cnt = torch.empty(2, dtype=torch.int32, device=dev)
        s = stream_ptr(stream)

        def counts():   # read on the host: wait for the caller's stream, whichever form it came in, as active() does
            if stream is not None:
                (stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(stream)).synchronize()
            return [int(v) for v in cnt.tolist()]
        if capacity is None:
            check(self.lib.rdsp_engine_pack_voice(self.h, n, None, None, 0, cnt.data_ptr(), s))
            capacity = counts()[0]
        capacity = int(capacity)
        audio = torch.empty((capacity, 128 // max(R, 1)), dtype=torch.int16, device=dev)
        records = torch.empty((capacity, 2), dtype=torch.int32, device=dev)
        check(self.lib.rdsp_engine_pack_voice(self.h, n, audio.data_ptr() if capacity else None, records.data_ptr() if capacity else None,
                                              capacity, cnt.data_ptr(), s))
        needed, written = counts()
        return audio[:written], records[:written], needed

    def enable_fm(self):
        """narrow-band FM from now on (include/rdsp.h, "narrow-band FM"): setDemodMode(NFMmode) puts the selected group(s) into
        it, and their meter becomes a carrier squelch.  Again: a no-op.  Takes no stream and waits for the device."""
        check(self.lib.rdsp_engine_enable_fm(self.h))

    @property
    def fm_enabled(self):
        return bool(self.lib.rdsp_engine_fm_enabled(self.h))

    def set_fm(self, W=2, deviation_hz=5000.0, tau_us=750.0):
        """the selected group's detector: channel filter W = 2 (wide) or 3 (narrow), the deviation that reads +-1.0
        (1000 ... 7500 Hz), the de-emphasis time constant (0: none, or 25 ... 1000 us)"""
        check(self.lib.rdsp_engine_set_fm(self.h, int(W), float(deviation_hz), float(tau_us)))

    def read_fm_level(self, n_blocks, stream=None):
        """the last call's level rows (the magnitude behind the channel filter, 1.0 = a full-scale carrier: what an NFM group's
        meter measures) -> float32 [n_channels, n_blocks x 128] on the device; zeros for receivers not in NFM"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks) * 128
        out = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        check(self.lib.rdsp_engine_read_fm_level(self.h, int(n_blocks), out.data_ptr(), n, stream_ptr(stream)))
        return out

    def enable_tone(self):
        """the CTCSS tone squelch from the next update on (include/rdsp.h, "tone squelch"): every NFM group runs a correlator per
        receiver at the receiver's tone and, with the meter on, closes the blocks that do not carry it.  After enable_fm();
        again: a no-op.  Takes no stream and waits for the device; does not need the meter."""
        check(self.lib.rdsp_engine_enable_tone(self.h))

    @property
    def tone_enabled(self):
        return bool(self.lib.rdsp_engine_tone_enabled(self.h))

    def set_tones(self, first_channel, tone_hz):
        """receivers first_channel ... get the tones tone_hz (Hz: 0 for none, or 60 ... 300); may precede enable_tone()"""
        t = np.ascontiguousarray(np.atleast_1d(tone_hz), np.float32)
        check(self.lib.rdsp_engine_set_tones(self.h, int(first_channel), t.size, t.ctypes.data_as(_F32P)))

    def set_tone_squelch(self, K=128, on_amp=0.04, off_amp=0.025):
        """the selected group's detector: windows of K blocks (4 ... 512); the tone is there from an amplitude of on_amp on the
        demodulated tap (1.0: the peak deviation) and until it falls below off_amp"""
        check(self.lib.rdsp_engine_set_tone_squelch(self.h, int(K), float(on_amp), float(off_amp)))

    def read_tone(self, n_blocks, stream=None):
        """the last call's records -> (a2 float32: the squared tone amplitude of the last completed window, tone uint8), each
        [n_channels, n_blocks] on the device; zeros for receivers the detector did not run on"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        a2 = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        tone = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        check(self.lib.rdsp_engine_read_tone(self.h, n, a2.data_ptr(), n, tone.data_ptr(), n, stream_ptr(stream)))
        return a2, tone

    def enable_tone_search(self):
        """the CTCSS tone search from the next update on (include/rdsp.h, "tone search"): every NFM group with a search window
        (set_tone_search) runs a bank of correlators per receiver, one per tone of the bank, and records which tone the channel
        carries.  It only measures.  After enable_fm(); independent of enable_tone(); again: a no-op.  Takes no stream and waits
        for the device."""
        check(self.lib.rdsp_engine_enable_tone_search(self.h))

    @property
    def tone_search_enabled(self):
        return bool(self.lib.rdsp_engine_tone_search_enabled(self.h))

    def set_tone_bank(self, hz):
        """the engine's bank: 1 ... 64 tones of 60 ... 300 Hz, strictly ascending (default: standard_tones()); may precede
        enable_tone_search()"""
        t = np.ascontiguousarray(np.atleast_1d(hz), np.float32)
        check(self.lib.rdsp_engine_set_tone_bank(self.h, t.ctypes.data_as(_F32P), t.size))

    def tone_bank(self):
        """the bank in force: float32 [n_tones]"""
        o = np.zeros(64, np.float32)
        n = self.lib.rdsp_engine_tone_bank(self.h, o.ctypes.data_as(_F32P))
        check(min(n, 0))
        return o[:n].copy()

    def set_tone_search(self, K=128, min_amp=0.04, ratio=4.0):
        """the selected group's search: windows of K blocks (0: off, or 4 ... 512); a tone is found when its amplitude behind the
        decimator is at least min_amp (1.0: the peak deviation) and its power at least ratio times that of the strongest tone
        that is not its neighbour in the bank"""
        check(self.lib.rdsp_engine_set_tone_search(self.h, int(K), float(min_amp), float(ratio)))

    def read_tone_search(self, n_blocks, stream=None):
        """the last call's records -> (best uint8: the index in the bank of the tone the last completed window found, 255: none;
        a2 float32: the strongest tone's squared amplitude; next float32: the largest power outside its neighbourhood), each
        [n_channels, n_blocks] on the device; 255 / 0 / 0 for receivers the search did not run on"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        best = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        a2 = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        nxt = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        check(self.lib.rdsp_engine_read_tone_search(self.h, n, best.data_ptr(), n, a2.data_ptr(), n, nxt.data_ptr(), n, stream_ptr(stream)))
        return best, a2, nxt

    def read_tone_spectrum(self, stream=None):
        """the last completed window's powers, one per tone of the bank -> float32 [n_channels, n_tones] on the device"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = len(self.tone_bank())
        out = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        check(self.lib.rdsp_engine_read_tone_spectrum(self.h, 0, self.n_channels, out.data_ptr(), n, stream_ptr(stream)))
        return out

    def enable_dcs(self):
        """the DCS code squelch from the next update on (include/rdsp.h, "code squelch"): every NFM group runs one more kernel
        that recovers the 134.4 bit/s code under the audio and, with the meter on, closes the blocks that do not carry the
        receiver's code.  After enable_fm(); independent of enable_tone() and enable_tone_search(); again: a no-op.  Takes no
        stream and waits for the device."""
        check(self.lib.rdsp_engine_enable_dcs(self.h))

    @property
    def dcs_enabled(self):
        return bool(self.lib.rdsp_engine_dcs_enabled(self.h))

    def set_dcs_codes(self, first_channel, codes):
        """receivers first_channel ... get the codes (0: none; 1 ... 511, the octal digits read as a number: 0o023; | DCS_INVERTED:
        inverted polarity; DCS_ANY: any valid code, read out); may precede enable_dcs()"""
        c = np.ascontiguousarray(np.atleast_1d(codes), np.uint16)
        check(self.lib.rdsp_engine_set_dcs_codes(self.h, int(first_channel), c.size, c.ctypes.data_as(C.POINTER(C.c_uint16))))

    def set_dcs_squelch(self, K=64, max_err=1, on_hits=16, off_hits=12):
        """the selected group's detector: windows of K blocks (8 ... 512); a word matches within max_err bits (0 ... 3); the code
        is there from on_hits matches in a window and until a window has fewer than off_hits"""
        check(self.lib.rdsp_engine_set_dcs_squelch(self.h, int(K), int(max_err), int(on_hits), int(off_hits)))

    def read_dcs(self, n_blocks, stream=None):
        """the last call's records -> (dcs uint8: the decision, hits uint8: the last completed window's matches, word int32: its
        matched word, the smallest rotation; dcs_code_of_word names it), each [n_channels, n_blocks] on the device; zeros for
        receivers the detector did not run on"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        dcs = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        hits = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        word = torch.empty((self.n_channels, n), dtype=torch.int32, device=dev)
        check(self.lib.rdsp_engine_read_dcs(self.h, n, dcs.data_ptr(), n, hits.data_ptr(), n, word.data_ptr(), n, stream_ptr(stream)))
        return dcs, hits, word

    def enable_noise(self):
        """the noise squelch from the next update on (include/rdsp.h, "noise squelch"): every NFM group whose mode
        (set_noise_squelch) is above 0 runs one more kernel that reads the discriminator's noise above the voice band and, at
        mode 2 with the meter on, closes the blocks of an empty channel.  After enable_fm(); again: a no-op.  Takes no stream
        and waits for the device; does not need the meter."""
        check(self.lib.rdsp_engine_enable_noise(self.h))

    @property
    def noise_enabled(self):
        return bool(self.lib.rdsp_engine_noise_enabled(self.h))

    def set_noise_squelch(self, mode=NOISE_GATE, open_n=0.01, close_n=0.025, hang_blocks=8, fall=0.75, rise=0.125):
        """the selected group's detector: mode NOISE_OFF, NOISE_MEASURE or NOISE_GATE; the gate opens when the level N of the
        noise reading (a mean square on the demodulated tap, 1.0: the peak deviation) is at most open_n and stays open until it
        is above close_n for more than hang_blocks blocks; N follows a falling reading with `fall`, a rising one with `rise`"""
        check(self.lib.rdsp_engine_set_noise_squelch(self.h, int(mode), float(open_n), float(close_n), int(hang_blocks), float(fall), float(rise)))

    def read_noise(self, n_blocks, stream=None):
        """the last call's records -> (noise float32: the level N, nopen uint8: the noise gate), each [n_channels, n_blocks] on the
        device; zeros for receivers the detector did not run on"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        noise = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        nopen = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        check(self.lib.rdsp_engine_read_noise(self.h, n, noise.data_ptr(), n, nopen.data_ptr(), n, stream_ptr(stream)))
        return noise, nopen

    def enable_dtmf(self):
        """the DTMF decoder from the next update on (include/rdsp.h, "DTMF decoder"): every NFM group with a frame length
        (set_dtmf) runs one more kernel that correlates the demodulated tap against the eight DTMF tones and reads the keys sent.
        It only measures.  After enable_fm(); independent of the other detectors; again: a no-op.  Takes no stream and waits for
        the device."""
        check(self.lib.rdsp_engine_enable_dtmf(self.h))

    @property
    def dtmf_enabled(self):
        return bool(self.lib.rdsp_engine_dtmf_enabled(self.h))

    def set_dtmf(self, K=4, min_amp=0.015, ratio=4.0, twist=16.0, share=0.5, on_frames=2, off_frames=2):
        """the selected group's decoder: frames of K blocks (0: off, or 4 ... 32); a frame carries a key when both groups'
        strongest tones have an amplitude of at least min_amp (1.0: the peak deviation), `ratio` times the power of their
        group's second, at most `twist` times each other's power, and together at least `share` of the frame's energy; a digit
        is emitted after on_frames equal frames and released after off_frames others"""
        check(self.lib.rdsp_engine_set_dtmf(self.h, int(K), float(min_amp), float(ratio), float(twist), float(share), int(on_frames), int(off_frames)))

    def read_dtmf(self, n_blocks, stream=None):
        """the last call's records -> (key uint8: the key held after each block, 255: none; new uint8: the key emitted by a frame
        that ended with the block, else 255; lo, hi float32: the two groups' largest powers of the last completed frame), each
        [n_channels, n_blocks] on the device; 255 / 255 / 0 / 0 for receivers the decoder did not run on"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        key = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        new = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        lo = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        hi = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        check(self.lib.rdsp_engine_read_dtmf(self.h, n, key.data_ptr(), n, new.data_ptr(), n, lo.data_ptr(), n, hi.data_ptr(), n, stream_ptr(stream)))
        return key, new, lo, hi

    def read_dtmf_digits(self, stream=None):
        """every receiver's digit count and ring -> (n_digits int32 [n_channels], ring int32 [n_channels, 16]) on the device
        (the words are uint32: view them so); ring[k mod 16] of digit k is sym | (t_blocks & 0xFFFFFF) << 8"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        count = torch.empty((self.n_channels,), dtype=torch.int32, device=dev)
        ring = torch.empty((self.n_channels, 16), dtype=torch.int32, device=dev)
        check(self.lib.rdsp_engine_read_dtmf_digits(self.h, 0, self.n_channels, count.data_ptr(), ring.data_ptr(), stream_ptr(stream)))
        return count, ring

    def enable_afsk(self):
        """the AFSK 1200 packet decoder from the next update on (include/rdsp.h, "AFSK 1200 packet decoder"): every NFM group
        with the decoder on (set_afsk) runs one more kernel that demodulates Bell 202 on the demodulated tap, recovers the bit
        clock, unstuffs HDLC and keeps the frames whose check sequence holds.  It only measures.  After enable_fm(); independent
        of the other detectors; again: a no-op.  Takes no stream and waits for the device."""
        check(self.lib.rdsp_engine_enable_afsk(self.h))

    @property
    def afsk_enabled(self):
        return bool(self.lib.rdsp_engine_afsk_enabled(self.h))

    def set_afsk(self, on=1, space_gain=1.0, pull=2, min_bytes=17):
        """the selected group's decoder: on 0 or 1; the space correlator's power counts space_gain times (1.0 for a sender
        that pre-emphasises, afsk_space_gain(tau_us) for a flat one); a transition pulls the bit clock by 2^-pull of its error;
        frames below min_bytes bytes (FCS included) are not looked at"""
        check(self.lib.rdsp_engine_set_afsk(self.h, int(on), float(space_gain), int(pull), int(min_bytes)))

    def read_afsk(self, n_blocks, stream=None):
        """the last call's records -> (sync uint8: inside a frame at the block's end; new uint8, bad uint8: the frames emitted
        and refused by their check sequence in the block; lvl float32: the two correlators' power), each [n_channels, n_blocks]
        on the device; zeros for receivers the decoder did not run on"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        sync = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        new = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        bad = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        lvl = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        check(self.lib.rdsp_engine_read_afsk(self.h, n, sync.data_ptr(), n, new.data_ptr(), n, bad.data_ptr(), n, lvl.data_ptr(), n, stream_ptr(stream)))
        return sync, new, bad, lvl

    def read_afsk_ring(self, stream=None):
        """every receiver's frame count and ring -> (n_frames int32 [n_channels], ring int32 [n_channels, 4, 84]) on the device
        (the words are uint32: view them so); slot k mod 4 of frame k is len, t_blocks and the bytes in 82 little-endian words"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        count = torch.empty((self.n_channels,), dtype=torch.int32, device=dev)
        ring = torch.empty((self.n_channels, 4, 84), dtype=torch.int32, device=dev)
        check(self.lib.rdsp_engine_read_afsk_frames(self.h, 0, self.n_channels, count.data_ptr(), ring.data_ptr(), stream_ptr(stream)))
        return count, ring

    def read_afsk_frames(self, stream=None):
        """the frames the rings hold -> a list of (channel, t_blocks, bytes), oldest first per channel: the last four at most
        (FCS checked and removed; ax25.parse reads the addresses).  Waits for the stream."""
        count, ring = (v.cpu().numpy().view("uint32") for v in self.read_afsk_ring(stream))
        out = []
        for c in count.nonzero()[0]:
            n = int(count[c])
            for k in range(max(0, n - 4), n):
                slot = ring[c, k % 4]
                out.append((int(c), int(slot[1]), slot[2:].astype("<u4").tobytes()[:int(slot[0])]))
        return out

    def enable_pocsag(self):
        """the POCSAG pager decoder from the next update on (include/rdsp.h, "POCSAG pager decoder"): every NFM group with a
        paging baud rate (set_pocsag) runs one more kernel that slices the demodulated tap behind a matched filter, recovers the
        bit clock, frames batches on the sync word, corrects every codeword by BCH(31,21) and keeps the messages.  It only
        measures.  After enable_fm(); set a paging channel with set_fm(W=2, deviation_hz=7500, tau_us=0).  Independent of the
        other detectors; again: a no-op.  Takes no stream and waits for the device."""
        check(self.lib.rdsp_engine_enable_pocsag(self.h))

    @property
    def pocsag_enabled(self):
        return bool(self.lib.rdsp_engine_pocsag_enabled(self.h))

    def set_pocsag(self, baud=1200, invert=2, pull=3, sync_errs=2, fix_addr=1, fix_data=2):
        """the selected group's decoder: baud 0 (off), 512, 1200 or 2400; invert 0, 1 or 2: the polarity as sent, inverted, or
        either; a transition pulls the bit clock by 2^-pull of its error; a sync word matches within sync_errs bits; address and
        idle words are accepted with up to fix_addr corrected bits, message words with up to fix_data"""
        check(self.lib.rdsp_engine_set_pocsag(self.h, int(baud), int(invert), int(pull), int(sync_errs), int(fix_addr), int(fix_data)))

    def read_pocsag(self, n_blocks, stream=None):
        """the last call's records -> (sync uint8: in sync at the block's end; new uint8: the messages closed in the block; bad
        uint8: its uncorrectable codewords; lvl float32: the matched filter's mean magnitude; dc float32: the tap's mean), each
        [n_channels, n_blocks] on the device; zeros for receivers the decoder did not run on"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        n = int(n_blocks)
        sync = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        new = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        bad = torch.empty((self.n_channels, n), dtype=torch.uint8, device=dev)
        lvl = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        dc = torch.empty((self.n_channels, n), dtype=torch.float32, device=dev)
        check(self.lib.rdsp_engine_read_pocsag(self.h, n, sync.data_ptr(), n, new.data_ptr(), n, bad.data_ptr(), n, lvl.data_ptr(), n, dc.data_ptr(), n,
                                               stream_ptr(stream)))
        return sync, new, bad, lvl, dc

    def read_pocsag_ring(self, stream=None):
        """every receiver's message count and ring -> (n_msgs int32 [n_channels], ring int32 [n_channels, 4, 84]) on the device
        (the words are uint32: view them so); slot k mod 4 of message k is n_cw | flags << 8 | polarity << 16, t_blocks, address
        | function << 21, corrected bits | uncorrectable words << 16 and the words"""
        import torch
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        count = torch.empty((self.n_channels,), dtype=torch.int32, device=dev)
        ring = torch.empty((self.n_channels, 4, 84), dtype=torch.int32, device=dev)
        check(self.lib.rdsp_engine_read_pocsag_messages(self.h, 0, self.n_channels, count.data_ptr(), ring.data_ptr(), stream_ptr(stream)))
        return count, ring

    def read_pocsag_messages(self, stream=None):
        """the messages the rings hold -> a list of (channel, pocsag.Message), oldest first per channel: the last four at most
        (pocsag.numeric and pocsag.alpha read the words).  Waits for the stream."""
        from . import pocsag
        count, ring = (v.cpu().numpy().view("uint32") for v in self.read_pocsag_ring(stream))
        out = []
        for c in count.nonzero()[0]:
            n = int(count[c])
            for k in range(max(0, n - 4), n):
                out.append((int(c), pocsag.from_slot(ring[c, k % 4])))
        return out

    def gather_events(self, capacity_events=None, capacity_words=None, stream=None):
        """the digits, frames and messages the decoders emitted in the last update, dense (include/rdsp.h "Decoder events") ->
        (records int32 [written_events, 4] = channel, kind | n_words << 8, seq, offset; words int32 [written_words], both on the
        device (view them as uint32); counts, an events.Counts of needed_events, written_events, needed_words, written_words and
        lost).  capacity_events, capacity_words: room for so many (default: a sizing call first, then exactly `needed`).  Waits
        for the stream."""
        import torch
        from . import events
        dev = torch.device("cuda", self.lib.rdsp_engine_device(self.h))
        cnt = torch.empty(5, dtype=torch.int32, device=dev)
        s = stream_ptr(stream)

        def counts():   # read on the host: wait for the caller's stream, whichever form it came in, as active() does
            if stream is not None:
                (stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(stream)).synchronize()
            return events.Counts(*[int(v) for v in cnt.tolist()])
        if capacity_events is None or capacity_words is None:
            check(self.lib.rdsp_engine_gather_events(self.h, None, 0, None, 0, cnt.data_ptr(), s))
            need = counts()
            capacity_events = need.needed_events if capacity_events is None else capacity_events
            capacity_words = need.needed_words if capacity_words is None else capacity_words
        ce, cw = int(capacity_events), int(capacity_words)
        records = torch.empty((ce, 4), dtype=torch.int32, device=dev)
        words = torch.empty((cw,), dtype=torch.int32, device=dev)
        check(self.lib.rdsp_engine_gather_events(self.h, records.data_ptr() if ce else None, ce, words.data_ptr() if cw else None, cw, cnt.data_ptr(), s))
        got = counts()
        return records[:got.written_events], words[:got.written_words], got

    def events(self, stream=None):
        """the last update's events -> a list of events.Event(channel, kind, seq, t_blocks, value), by channel, then kind (DTMF,
        AFSK, POCSAG), then seq: value is the key's character, the frame's bytes or a pocsag.Message.  Waits for the stream."""
        from . import events
        records, words, _ = self.gather_events(stream=stream)
        return events.parse(records.cpu().numpy(), words.cpu().numpy())

    def set_groups(self, first_channels):
        """groups of consecutive channels with settings of their own: first_channels[g] = group g's first channel"""
        a = (C.c_int * len(first_channels))(*[int(x) for x in first_channels])
        check(self.lib.rdsp_engine_set_groups(self.h, len(first_channels), a))

    def select_group(self, group):
        """the group the setters address from now on; -1: all"""
        check(self.lib.rdsp_engine_select_group(self.h, int(group)))

    def save_state(self, first_channel, n_channels):
        n = self.lib.rdsp_engine_state_bytes(self.h, n_channels)
        buf = np.zeros(n, np.uint8)
        check(self.lib.rdsp_engine_save_state(self.h, first_channel, n_channels, buf.ctypes.data_as(C.c_void_p), n, None))
        return buf

    def load_state(self, first_channel, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        check(self.lib.rdsp_engine_load_state(self.h, first_channel, blob.ctypes.data_as(C.c_void_p), blob.size, None))

    def scalars(self):
        o = np.zeros((self.n_channels, 8), np.float32)
        check(self.lib.rdsp_engine_get_scalars(self.h, o.ctypes.data_as(_F32P), None))
        return o

    def agc_curve(self):
        return np.ctypeslib.as_array(self.lib.rdsp_engine_agc_curve(self.h), (130,)).copy()

    def sine_table(self):
        return np.ctypeslib.as_array(self.lib.rdsp_engine_sine_table(self.h), (257,)).copy()

    def tune_table(self):
        """the tuning pass's phasor table: [1024][4] = cos, sin of 2 pi k / 1024, steps to entry k + 1"""
        return np.ctypeslib.as_array(self.lib.rdsp_engine_tune_table(), (1024, 4)).copy()

    def reset(self):
        check(self.lib.rdsp_engine_reset(self.h, None))


def ddc_taps(D, gain=1.0):
    """the prototype low-pass of set_source_decimation(D, gain): 16 D float32 taps (host only, no GPU)"""
    o = np.zeros(16 * int(D), np.float32)
    check(load().rdsp_engine_ddc_taps(int(D), float(gain), o.ctypes.data_as(_F32P)))
    return o


def voice_taps(R):
    """the taps of enable_voice(R): 16 R int32, the prototype of ddc_taps(R) times 2^18, rounded (host only, no GPU)"""
    o = np.zeros(16 * int(R) if int(R) in (2, 4) else 1, np.int32)
    check(load().rdsp_engine_voice_taps(int(R), o.ctypes.data_as(C.POINTER(C.c_int32))))
    return o


def fm_atan2(y, x):
    """the discriminator's arctangent, csrc/rdsp_fm.h's fm_atan2 (host only, no GPU)"""
    return float(load().rdsp_engine_fm_atan2(float(y), float(x)))


def fm_constants(deviation_hz=5000.0, tau_us=750.0):
    """(k, a) of set_fm's deviation and time constant as float32: the discriminator's scale and the de-emphasis coefficient
    (host only, no GPU)"""
    o = np.zeros(2, np.float32)
    check(load().rdsp_engine_fm_constants(float(deviation_hz), float(tau_us), o.ctypes.data_as(_F32P)))
    return o[0], o[1]


def tone_gain(tone_hz, tau_us=750.0):
    """the magnitude of the NFM de-emphasis at tone_hz (1.0 for tau_us == 0): a tone at d Hz of deviation reads
    d / deviation_hz x tone_gain on the demodulated tap (host only, no GPU)"""
    g = float(load().rdsp_engine_tone_gain(float(tone_hz), float(tau_us)))
    if g == 0.0:
        check(-1)
    return g


def standard_tones():
    """the 50 standard CTCSS tones, 67.0 ... 254.1 Hz, ascending: the tone search's default bank (host only, no GPU)"""
    o = np.zeros(50, np.float32)
    assert load().rdsp_engine_tone_standard(o.ctypes.data_as(_F32P)) == 50
    return o


def tone_search_gain(tone_hz, tau_us=750.0):
    """what the tone search's decimator (a boxcar of 32 samples) and the NFM de-emphasis leave of a tone at tone_hz: sqrt(a2) of
    a tone at d Hz of deviation reads d / deviation_hz x tone_search_gain (host only, no GPU)"""
    g = float(load().rdsp_engine_tone_search_gain(float(tone_hz), float(tau_us)))
    if g == 0.0:
        check(-1)
    return g


def dcs_codeword(code):
    """the 23-bit word of DCS code 0 ... 511 (0o023 -> 0x763813), sent LSB first (host only, no GPU)"""
    w = int(load().rdsp_dcs_codeword(int(code)))
    if w == 0:
        check(-1)
    return w


def standard_dcs_codes():
    """the 104 standard DCS codes 0o023 ... 0o754, ascending: uint16 [104] (host only, no GPU)"""
    o = np.zeros(104, np.uint16)
    assert load().rdsp_dcs_standard(o.ctypes.data_as(C.POINTER(C.c_uint16))) == 104
    return o


def dcs_code_of_word(word):
    """(code, inverted) of a word read_dcs reported: the lowest standard code whose word is a rotation of it -- the
    normal-polarity reading, since every standard code's inverted word is another standard code's (host only, no GPU)"""
    code, inv = C.c_int(0), C.c_int(0)
    check(load().rdsp_dcs_code_of_word(int(word) & 0xFFFFFFFF, C.byref(code), C.byref(inv)))
    return code.value, bool(inv.value)


def noise_taps(tau_us=750.0):
    """the 65 float32 taps of the noise squelch for a group whose set_fm has tau_us: a 4500 ... 8000 Hz band-pass with the
    inverse of the de-emphasis folded in (host only, no GPU)"""
    o = np.zeros(65, np.float32)
    check(load().rdsp_engine_noise_taps(float(tau_us), o.ctypes.data_as(_F32P)))
    return o


def dtmf_key(sym):
    """the key of a DTMF symbol 0 ... 15, "123A456B789C*0#D"[sym]; "" for anything else (host only, no GPU)"""
    return load().rdsp_engine_dtmf_key(int(sym)).decode("ascii").rstrip("\0")


def dtmf_gain(hz, tau_us=750.0):
    """what the DTMF decoder's decimator (a boxcar of 4 samples) and the NFM de-emphasis leave of a tone at hz: the square root
    of its power reads d / deviation_hz x dtmf_gain for a tone at d Hz of deviation (host only, no GPU)"""
    g = float(load().rdsp_engine_dtmf_gain(float(hz), float(tau_us)))
    if g == 0.0:
        check(-1)
    return g


def afsk_space_gain(tau_us=750.0):
    """the AFSK decoder's space_gain for a sender that does not pre-emphasise: (dtmf_gain(1200) / dtmf_gain(2200))^2 behind a
    de-emphasis of tau_us (host only, no GPU)"""
    g = float(load().rdsp_engine_afsk_space_gain(float(tau_us)))
    if g == 0.0:
        check(-1)
    return g


def afsk_fcs(data):
    """the X-25 frame check sequence of AX.25 over `data`; a frame carries it low byte first (host only, no GPU)"""
    data = bytes(data)
    return int(load().rdsp_engine_afsk_fcs(data, len(data)))


def pocsag_bch_table():
    """the POCSAG decoder's correction table: 1024 uint16 by syndrome, b1 | b2 << 5 | ne << 10, 0xFFFF for no pattern of weight
    <= 2 (host only, no GPU)"""
    import numpy as np
    p = load().rdsp_engine_pocsag_bch_table()
    return np.array([p[k] for k in range(1024)], np.uint16)


def pocsag_codeword(data21):
    """the POCSAG codeword of 21 data bits: BCH(31,21) and even parity (host only, no GPU)"""
    return int(load().rdsp_engine_pocsag_codeword(int(data21) & 0x1FFFFF))


def rate_taps(P, Q, gain=1.0):
    """the prototype low-pass of set_source_rate(P, Q, gain): 16 ceil(P / Q) Q float32 taps, P / Q in lowest terms (host only,
    no GPU); branch r is taps[r::Q]"""
    import math
    g = math.gcd(int(P), int(Q)) if int(P) > 0 and int(Q) > 0 else 1
    p, q = int(P) // g, int(Q) // g
    o = np.zeros(16 * (-(-p // q)) * q if 0 < q <= 441 and q <= p <= 64 * q else 1, np.float32)
    check(load().rdsp_engine_rate_taps(int(P), int(Q), float(gain), o.ctypes.data_as(_F32P)))
    return o


def rate_of_hz(fs_hz):
    """(P, Q) with fs_hz = 44100 P / Q for an integer-Hz rate inside the limits of set_source_rate; RdspError otherwise"""
    p, q = C.c_int(), C.c_int()
    check(load().rdsp_engine_rate_of_hz(float(fs_hz), C.byref(p), C.byref(q)))
    return p.value, q.value


def pack_runs(records, first_block=0):
    """the records of a pack_active (host int32 [n, 2]: channel, block inside the call) merged into runs of consecutive blocks
    of one receiver -> int64 [m, 4]: channel, absolute first block (first_block + block), number of blocks, index of the run's
    first packed block; host only.  Records that are not strictly ascending in (channel, block) are refused."""
    rec = np.ascontiguousarray(records, np.int32).reshape(-1, 2)
    run_t = np.dtype([("channel", np.int32), ("n_blocks", np.int32), ("record", np.int32), ("block", np.int64)], align=True)   # rdsp_pack_run_t
    runs = np.zeros(max(len(rec), 1), run_t)
    n = load().rdsp_pack_runs(rec.ctypes.data, len(rec), int(first_block), runs.ctypes.data, len(rec))
    if n < 0:
        check(n)
    r = runs[:n]
    return np.stack([r["channel"], r["block"], r["n_blocks"], r["record"]], 1).astype(np.int64).reshape(-1, 4)


def ms_of_db(db):
    """the mean square of a sine at db dB re full scale (amplitude 1.0): 0.5 x 10^(db / 10); host only"""
    return 0.5 * 10.0 ** (float(db) / 10.0)


def db_of_ms(ms):
    """ms_of_db's inverse: 10 log10(2 ms), -inf for 0; host only"""
    import math
    return 10.0 * math.log10(2.0 * float(ms)) if ms > 0 else -math.inf


def _setter(name):
    def f(self, *a):
        check(getattr(self.lib, "rdsp_engine_" + name)(self.h, *a))
    f.__name__ = name
    return f


for _n in ("enableAGC", "setAGCmode", "enableALSfilter", "disableALSfilter", "setALSfilterNotch", "setALSfilterPeak",
           "setALSfilterAdaptive", "enableNoiseBlanker", "disableNoiseBlanker", "setInputGain", "setOutputGain",
           "setIQgainBalance", "enableAudioFilter", "setAudioFilter", "setMute"):
    setattr(Engine, _n, _setter(_n))


class PreProcessor(Handle):
    """`AudioSDRpreProcessor preProcessor;` (INO:53): rdsp_preproc_* of include/rdsp.h"""
    _destroy = "rdsp_preproc_destroy"

    def __init__(self, n_channels, device=0):
        self._create("rdsp_preproc_create", n_channels, device)
        self.n_channels = n_channels

    def startAutoI2SerrorDetection(self):
        check(self.lib.rdsp_preproc_startAutoI2SerrorDetection(self.h))

    def swapIQ(self, on):
        check(self.lib.rdsp_preproc_swapIQ(self.h, int(bool(on))))

    def reset(self):
        """state as constructed (not detecting until startAutoI2SerrorDetection); swapIQ kept"""
        check(self.lib.rdsp_preproc_reset(self.h, None))

    def update(self, d_iq, out=None, stream=None):
        import torch
        nch, n, two = d_iq.shape
        assert nch == self.n_channels and two == 2 and n % 128 == 0 and d_iq.dtype == torch.int16 and d_iq.is_contiguous()
        if out is None:
            out = torch.empty_like(d_iq)
        check(self.lib.rdsp_preproc_update(self.h, d_iq.data_ptr(), n, n // 128, out.data_ptr(), n, stream_ptr(stream)))
        return out

    def state(self):
        o = np.zeros((self.n_channels, 4), np.int16)
        check(self.lib.rdsp_preproc_get_state(self.h, o.ctypes.data_as(C.POINTER(C.c_int16)), None))
        return o
