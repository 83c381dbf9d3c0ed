"""rdsp_survey_t on the GPU at its edges (include/rdsp.h "survey"; kernel csrc/rdsp_survey.hip), behind the six cases of
tests/test_survey.py: the noise floor against a float32 reference, and the schedule and the launch shape at the settings those
cases never reach.  tests/survey_model.py is the model; docs/engine.md lists what each test pins.

The floor.  The bound of survey_model.survey_rows scales with a frame's norm: beside a carrier it admits -99.7 dB (N = 1024)
and -98.2 dB (N = 4096) of the peak at every bin, and a kernel that had lost 40 dB of dynamic range would pass it.
test_gpu_floor_against_the_float32_reference holds the kernel's far-bin maximum on survey_model.two_tone to that of
survey_model.survey_rows_f32 (scipy's complex64 transform on the same float32 windowed frames) on the same input plus
12 dB: the factor 4 in amplitude that chain twiddles good to about 4 ulp can cost over exact ones.  Measured on an MI355X,
dB relative to the peak (weak tone at -100 dB / at -120 dB / the -100 dB pair run backwards):
    N = 1024: -147.9 / -147.4 / -137.1, the reference -150.2 / -150.4 / -146.6: 2.3, 3.0 and 9.5 dB over it;
    N = 4096: -149.4 / -150.4 / -137.6, the reference -155.1 / -156.0 / -148.3: 5.7, 5.6 and 10.7 dB over it.
The mirrored pair is the worst case of both and the chains are what it costs: rdsp_fft.h's plan run thread by thread on the
host reads -136.5 and -138.4 dB on it with the chain twiddles and -148.6 and -144.3 dB with every twiddle rounded from double.

The schedule.  Every row of every test lies inside the bound of survey_rows of the float64 model, and where a twin took the
same stream in one call, the rows are the twin's bits: navg = 1 (no partial sums, no prefetch), navg = 8 across calls of
H + 3 pairs (the part buffers flip with every call), navg = 256 (the limit), a launch whose first unit continues part_in
while its last writes part_out, 300 units in one launch, 67 and 4096 sources, and drawn sessions with a reset in mid-row."""
import functools

import numpy as np
import pytest

import survey_model as M
from engine_sources_model import DTYPE, FL, S8, S16, U8
from test_survey import _odd_view

pytestmark = pytest.mark.gpu
NSRC = 3
SENTINEL = -7.0


def _rows_of(fmt, n_sources, n, seed):
    """[n_sources, n, 2] elements of format fmt drawn over the whole range, the rails mixed in; every source its own draw"""
    r = np.random.default_rng(seed)
    if fmt == FL:
        x = r.uniform(-1.0, 1.0, (n_sources, n, 2)).astype(np.float32)
        rails = np.array([-1.0, 1.0, 1.5, -2.0, 0.0], np.float32)
    else:
        info = np.iinfo(DTYPE[fmt])
        x = r.integers(info.min, info.max + 1, (n_sources, n, 2)).astype(DTYPE[fmt])
        rails = np.array([info.min, info.max], DTYPE[fmt])
    at = r.random((n_sources, n, 2)) < 0.02
    x[at] = rails[r.integers(0, len(rails), int(at.sum()))]
    return x


def _survey(n_sources, N, navg, fmt, max_pairs):
    from radiodsp_sdr_rx_amd.survey import Survey
    return Survey(n_sources, N, navg, fmt, max_pairs)


def _walk(sv, d, cuts, T=0, at=0, spare=0):
    """the calls of `cuts` pairs walking through d from pair `at` on, the object having seen T pairs since its reset: rows_for
    before every call is the model's schedule, and with `spare`, `out` has that many more rows, which keep their sentinel
    -> the rows of all calls [sources, rows, N] on the device"""
    import torch
    N, outs = sv.fft_n, []
    for pairs in cuts:
        want = sv.rows_for(pairs)
        assert want == M.rows_between(N, sv.navg, T, pairs), (T, pairs)
        out = torch.full((sv.n_sources, want + spare, N), SENTINEL, dtype=torch.float32, device="cuda") if spare else None
        rows = sv.update(d[:, at:at + pairs], pairs=pairs, out=out)
        assert rows.shape == (sv.n_sources, want, N)
        if spare:
            assert bool((out[:, want:] == SENTINEL).all()), (T, pairs)
        outs.append(rows)
        T += pairs
        at += pairs
    return torch.cat(outs, 1)


def _inside_the_bound(got, fmt, raw, N, navg):
    """got [sources, rows, N] (device) against the float64 model of every source's stream raw[s] -> worst |P^ - P| / bound"""
    from radiodsp_sdr_rx_amd import survey
    got = got.cpu().numpy().astype(np.float64)
    w = survey.window(N)
    worst = 0.0
    assert np.isfinite(got).all() and (got >= 0).all()
    for s in range(len(raw)):
        P, B = M.survey_rows(fmt, raw[s], N, navg, w)
        assert got[s].shape == P.shape, (s, got[s].shape, P.shape)
        if not P.size:
            continue
        frac = np.abs(got[s] - P) / B
        assert frac.max() <= 1.0, (s, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
        worst = max(worst, float(frac.max()))
    return worst


# ---- A. the floor ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _floor_case(N):
    """the three sources of the floor test (weak tone at -100 dB, at -120 dB, the -100 dB pair run backwards), the float64
    model's rows of them with their bound and the float32 reference's rows, computed once"""
    from radiodsp_sdr_rx_amd import survey
    a, b = M.two_tone(N, -100, 2), M.two_tone(N, -120, 2)
    raw = np.stack([a, b, a[::-1].copy()])
    w = survey.window(N)
    model = [M.survey_rows(FL, x, N, 2, w) for x in raw]
    P, B = np.stack([m[0][0] for m in model]), np.stack([m[1][0] for m in model])
    R = np.stack([M.survey_rows_f32(FL, x, N, 2, w)[0] for x in raw])
    for v in (raw, P, B, R):
        v.setflags(write=False)
    return raw, P, B, R


@pytest.mark.parametrize("N", [1024, 4096])
def test_gpu_floor_against_the_float32_reference(rdsp, N):
    """F32, navg = 2, one call of N + N / 2 pairs through an odd-offset view, survey_model.two_tone: source 0 with the weak tone at
    -100 dB, source 1 at -120 dB, source 2 the -100 dB pair run backwards (its tones on the mirrored bins).  Floor: each row's
    largest bin more than 8 bins from both tones, relative to its peak, is at most the float32 reference's for the same
    input plus 12 dB (survey_model.floor_within_margin; the reference is computed here).  Weak tone: at -100 dB its bin is
    within 3 % in power of the float64 model's (a floor 38 dB below it moves its amplitude by at most 1.26 %), on the mirrored
    bin too; at -120 dB its bin is a local maximum at least 15 dB over the far-bin maximum.  The peaks sit on their bins, and
    every bin lies inside the bound of the model as well."""
    raw, P, B, R = _floor_case(N)
    sv = _survey(NSRC, N, 2, FL, N + N // 2)
    got = sv.update(_odd_view(raw.copy())).cpu().numpy().astype(np.float64)
    sv.close()
    assert got.shape == (NSRC, 1, N) and np.isfinite(got).all()
    got = got[:, 0]
    assert (np.abs(got - P) <= B).all()
    floors = []
    for s, mirror in ((0, False), (1, False), (2, True)):
        strong, weak = M.tone_indices(N, mirror)
        ok, gpu_db, ref_db = M.floor_within_margin(got[s], R[s], N, mirror)
        ratio = got[s, weak] / P[s, weak]
        print(f"N = {N}, source {s}: GPU floor {gpu_db:.1f} dB, float32 reference {ref_db:.1f} dB, limit {ref_db + M.FLOOR_MARGIN_DB:.1f} dB; "
              f"weak bin GPU / model = {ratio:.5f}, reference / model = {R[s, weak] / P[s, weak]:.5f}")
        floors.append((ok, gpu_db, ref_db))
        assert got[s].argmax() == strong and P[s].argmax() == strong
        far_max = got[s][M.far(N, mirror)].max()
        assert got[s, weak] > got[s, weak - 1] and got[s, weak] > got[s, weak + 1]
        if s == 1:
            assert 10.0 * np.log10(got[s, weak] / far_max) >= 15.0
        else:
            assert abs(ratio - 1.0) <= 0.03, (s, ratio)
    assert all(ok for ok, _, _ in floors), floors


# ---- B. schedule and shape edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,fmt", [(1024, U8), (1024, FL), (4096, S8), (4096, S16)])
def test_gpu_navg_1(rdsp, N, fmt):
    """navg = 1: every unit one frame, no partial sums, no trailing row, the prefetch branch never taken.  One call of 9 H + 5
    pairs (8 rows), and the same stream cut at 1, H - 1, H + 1, N, rest: inside the bound of the model, the same bits"""
    import torch
    H = N // 2
    total = 9 * H + 5
    raw = _rows_of(fmt, NSRC, total, 500 + fmt)
    d = _odd_view(raw)
    one, cut = _survey(NSRC, N, 1, fmt, total), _survey(NSRC, N, 1, fmt, total)
    whole = _walk(one, d, [total])
    assert whole.shape[1] == 8
    cuts = [1, H - 1, H + 1, N]
    parts = _walk(cut, d, cuts + [total - sum(cuts)], spare=1)
    print(f"N = {N}, format {fmt}: worst |P^ - P| / bound = {_inside_the_bound(whole, fmt, raw, N, 1):.4f}")
    assert torch.equal(parts, whole)
    one.close()
    cut.close()


@pytest.mark.parametrize("fmt", [S8, FL])
def test_gpu_a_row_across_many_calls(rdsp, fmt):
    """navg = 8, N = 1024, the two formats test_gpu_call_split_bit_for_bit leaves out: 13 N pairs (25 frames: three rows and a
    frame) in one call against calls of H + 3 pairs -- each completes at most two frames, row 0 spans more than 8 calls and the
    part buffers flip with every call that completes a frame and no row.  Then 7 H pairs more on both, which complete the fourth row
    from what each object kept.  All four rows inside the bound of the model, the same bits"""
    import torch
    N, H, navg = 1024, 512, 8
    total = 13 * N
    raw = _rows_of(fmt, NSRC, total + 7 * H, 510 + fmt)
    d = _odd_view(raw)
    one, cut = _survey(NSRC, N, navg, fmt, total), _survey(NSRC, N, navg, fmt, total)
    whole = _walk(one, d, [total])
    cuts = [H + 3] * (total // (H + 3))
    cuts.append(total - sum(cuts))
    at = np.cumsum([0] + cuts)
    per_call = [M.frames(N, int(b)) - M.frames(N, int(a)) for a, b in zip(at[:-1], at[1:])]
    assert max(per_call) <= 2 and int(np.argmax(np.cumsum(per_call) >= navg)) + 1 > 8 and sum(f > 0 for f in per_call) >= 20
    assert whole.shape[1] == 3 and M.frames(N, total) == 25
    parts = _walk(cut, d, cuts, spare=1)
    assert torch.equal(parts, whole)
    a, b = _walk(one, d, [7 * H], T=total, at=total), _walk(cut, d, [7 * H], T=total, at=total)
    assert a.shape[1] == 1 and torch.equal(a, b)
    print(f"format {fmt}: worst |P^ - P| / bound = {_inside_the_bound(torch.cat([whole, a], 1), fmt, raw, N, navg):.4f}")
    one.close()
    cut.close()


def test_gpu_navg_256(rdsp):
    """navg = 256, the limit, N = 1024, S16: one row of 257 H pairs as one call and cut in three uneven calls (the last of 3
    pairs) -- inside the bound of the model, whose navg 2^-24 sum P term is a share of it worth printing here, and the
    same bits"""
    import torch
    from radiodsp_sdr_rx_amd import survey
    N, H, navg = 1024, 512, 256
    total = 257 * H
    raw = _rows_of(S16, NSRC, total, 520)
    d = _odd_view(raw)
    one, cut = _survey(NSRC, N, navg, S16, total), _survey(NSRC, N, navg, S16, total)
    whole = _walk(one, d, [total])
    parts = _walk(cut, d, [100 * H + 7, total - (100 * H + 7) - 3, 3], spare=1)
    assert whole.shape[1] == 1 and M.frames(N, total - 3) == 255
    P, B = M.survey_rows(S16, raw[0], N, navg, survey.window(N))
    print(f"worst |P^ - P| / bound = {_inside_the_bound(whole, S16, raw, N, navg):.4f}; the sum's share of the bound at most "
          f"{(navg * 2.0 ** -24 * P / B).max():.3f}")
    assert torch.equal(parts, whole)
    one.close()
    cut.close()


@pytest.mark.parametrize("N", [1024, 4096])
def test_gpu_lead_and_trailing_in_one_launch(rdsp, N):
    """navg = 4, U8, three calls held against the model: the first ends inside a row (3 frames, the partial sums in one copy);
    the second brings 7 frames -- a unit that finishes row 0 from part_in (lead 3), a whole row, and a trailing unit of two
    frames that writes part_out in the same launch; the third completes the trailing row.  The shape of the second call is
    asserted from survey_model.frames; a twin that took the stream in one call gives the same bits"""
    import torch
    H, navg = N // 2, 4
    cuts = [2 * N + 5, 7 * H + 95, 2 * H - 97]
    T1, T2, T3 = np.cumsum(cuts).tolist()
    f1, f2, f3 = (M.frames(N, T) for T in (T1, T2, T3))
    assert (f1, f2, f3) == (3, 10, 12) and f1 % navg == 3 and f2 % navg == 2
    assert M.rows_between(N, navg, T1, cuts[1]) == 2 and M.rows_between(N, navg, 0, T1) == 0 and M.rows_between(N, navg, T2, cuts[2]) == 1
    raw = _rows_of(U8, NSRC, T3, 530 + N)
    d = _odd_view(raw)
    cut, one = _survey(NSRC, N, navg, U8, T3), _survey(NSRC, N, navg, U8, T3)
    got = _walk(cut, d, cuts, spare=1)
    print(f"N = {N}: worst |P^ - P| / bound = {_inside_the_bound(got, U8, raw, N, navg):.4f}")
    assert torch.equal(got, _walk(one, d, [T3]))
    cut.close()
    one.close()


def test_gpu_many_units_in_one_launch(rdsp):
    """navg = 1, N = 1024, S16: one call that completes 300 rows a source (grid.x = 300), every one inside the bound of the
    model"""
    N, H = 1024, 512
    total = N + 299 * H + 17
    raw = _rows_of(S16, NSRC, total, 540)
    sv = _survey(NSRC, N, 1, S16, total)
    got = _walk(sv, _odd_view(raw), [total], spare=1)
    assert got.shape[1] == 300
    print(f"worst |P^ - P| / bound = {_inside_the_bound(got, S16, raw, N, 1):.4f}")
    sv.close()


@pytest.mark.parametrize("n_sources", [67, 4096])
def test_gpu_many_sources(rdsp, n_sources):
    """67 sources, and 4096, the most rdsp_survey_create accepts (blockIdx.y carries the source): N = 1024, navg = 1, U8, N + H
    pairs, two rows a source.  Every source has its own drawn row and every source's rows are held against the model; `out`
    has a third row per source, whose sentinel survives"""
    N, H = 1024, 512
    raw = _rows_of(U8, n_sources, N + H, 550 + n_sources)
    assert len({x.tobytes() for x in raw}) == n_sources
    sv = _survey(n_sources, N, 1, U8, N + H)
    got = _walk(sv, _odd_view(raw), [N + H], spare=1)
    assert got.shape == (n_sources, 2, N)
    print(f"{n_sources} sources: worst |P^ - P| / bound = {_inside_the_bound(got, U8, raw, N, 1):.4f}")
    sv.close()


def _draw_session(seed):
    """-> (N, navg, fmt, the pairs of 12 calls, the index of the call a reset() comes before).  Six sizes from {0, 1, H - 1, H,
    H + 1, N - 1, N, N + 1} and six uniform up to 3 N navg, shuffled; the reset before a drawn call that begins in mid-row
    (frames completed so far no multiple of navg; at navg = 1, a frame begun)"""
    r = np.random.default_rng(seed)
    N = int(r.choice([1024, 4096]))
    navg = int(r.choice([1, 2, 8]))
    fmt = int(r.choice([S16, U8, S8, FL]))
    H = N // 2
    cuts = [int(v) for v in r.choice([0, 1, H - 1, H, H + 1, N - 1, N, N + 1], 6)] + [int(v) for v in r.integers(0, 3 * N * navg + 1, 6)]
    cuts = [cuts[i] for i in r.permutation(12)]
    T = np.cumsum([0] + cuts).tolist()
    mid = [i for i in range(2, 11) if T[i] > H and (M.frames(N, T[i]) % navg != 0 or navg == 1)]
    assert mid, seed
    return N, navg, fmt, cuts, int(r.choice(mid))


def _call_shapes(N, navg, cuts):
    """per call of a segment from a reset on: (it completes no frame although at least H pairs are kept, its units)"""
    H, T, out = N // 2, 0, []
    for pairs in cuts:
        f0, f1 = M.frames(N, T), M.frames(N, T + pairs)
        units = (f1 // navg - f0 // navg) + (1 if f1 > f0 and f1 % navg else 0)
        out.append((pairs > 0 and f1 == f0 and T - f0 * H >= H, units))
        T += pairs
    return out


SESSION_SEEDS = (1, 17, 65)     # (1024, 2, F32), (4096, 8, S16), (1024, 1, S8)


@pytest.mark.parametrize("seed", SESSION_SEEDS)
def test_gpu_drawn_sessions(rdsp, seed):
    """N, navg in {1, 2, 8} and the format drawn; 12 calls of drawn sizes (_draw_session) with one reset() before a drawn call
    in mid-row, `out` with a spare row whose sentinel survives, rows_for before every call the model's schedule.  The rows of
    each segment (before and behind the reset) lie inside the bound of the model of that segment's stream and are, bit for
    bit, those of a twin that took the segment in one call.  Every seed's draw has a call that completes no frame while at
    least H pairs are kept (keep_from < 0 in the finish kernel) and a call of three or more units"""
    import torch
    N, navg, fmt, cuts, at_reset = _draw_session(seed)
    segments = [cuts[:at_reset], cuts[at_reset:]]
    shapes = [s for seg in segments for s in _call_shapes(N, navg, seg)]
    print(f"seed {seed}: N = {N}, navg = {navg}, format {fmt}, calls {cuts}, reset before call {at_reset}, units {[u for _, u in shapes]}")
    assert any(quiet for quiet, _ in shapes) and max(u for _, u in shapes) >= 3
    total = sum(cuts)
    raw = _rows_of(fmt, NSRC, total, 600 + seed)
    d = _odd_view(raw)
    sv, twin = _survey(NSRC, N, navg, fmt, total), _survey(NSRC, N, navg, fmt, total)
    at = 0
    for seg in segments:
        n = sum(seg)
        got = _walk(sv, d, seg, at=at, spare=1)
        worst = _inside_the_bound(got, fmt, raw[:, at:at + n], N, navg)
        print(f"  {len(seg)} calls, {n} pairs, {got.shape[1]} rows: worst |P^ - P| / bound = {worst:.4f}")
        assert got.shape[1] > 0 and torch.equal(got, _walk(twin, d, [n], at=at))
        sv.reset()
        twin.reset()
        at += n
    assert at == total and sv.rows_for(N) == 1 // navg
    sv.close()
    twin.close()
