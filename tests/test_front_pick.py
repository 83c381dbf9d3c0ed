"""Which front-kernel instance a call runs (rdsp_front_pick, csrc/rdsp_kernels.h): the one place that decides it, pinned.

No parity test can see a wrong pick: LEAN against the full-register kernel differs by 3e-7, PRE against non-PRE is bit-identical
by design, the families agree to 1e-5.  So tests/host/front_pick_check.cpp calls the function over the whole grid -- host code
only, no device -- and the table below is written out from the rules, not computed by the library:

  radix    256 -> 4, 512 -> 8, 1024 -> 16, 2048 -> 8, 4096 -> 16; any other FFT_L, or a decimation other than 1 or 4: invalid value
  PRE      nb_on, swap_iq, swap_hist != swap_iq, scale_i_hist != scale_i, scale_q_hist != scale_q, scale_i != scale_q
  decim 4 and fir_fd != 0
    fir_fd >= 3, blanker off: rows -- no rd_mask: invalid value; fir_fd 4 (RV 192, measured and not adopted): not supported;
             else RV 128; LEAN = radix >= 8 whatever `lean` says; Q4 = FFT_L 256 and not to_mid
    otherwise wave-wide frames -- VC 4 for fir_fd 2 and 3, else 7; LEAN = radix 16 or `lean`; Q4 = FFT_L 256 and not to_mid
             (RDSP_NO_QUAD unset)
  else the direct form -- LEAN = radix 16 or `lean`; fir_matrix (the matrix-core FIR, measured and not adopted): not
             supported at either decimation
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_VALUE, NOT_SUPPORTED = 1, 801      # hipErrorInvalidValue, hipErrorNotSupported
DIRECT, FD, RD = 0, 1, 2
RADIX = {256: 4, 512: 8, 1024: 16, 2048: 8, 4096: 16}


def expected(fft_l, decim, lean, fir_fd, fir_matrix, nb_on, to_mid, have_rd_mask, trigger):
    """(error, family, radix, lean, pre, q4, frame); zeros behind an error"""
    refuse = lambda e: (e, 0, 0, 0, 0, 0, 0)
    if decim not in (1, 4) or fft_l not in RADIX:
        return refuse(INVALID_VALUE)
    radix = RADIX[fft_l]
    pre = int(bool(nb_on) or trigger != 0)
    if decim == 4 and fir_fd != 0:
        if fir_fd >= 3 and not nb_on:
            if not have_rd_mask:
                return refuse(INVALID_VALUE)
            if fir_fd == 4:
                return refuse(NOT_SUPPORTED)
            return (0, RD, radix, int(radix >= 8), pre, int(fft_l == 256 and not to_mid), 128)
        return (0, FD, radix, int(radix == 16 or lean), pre, int(fft_l == 256 and not to_mid), 4 if fir_fd in (2, 3) else 7)
    if fir_matrix:
        return refuse(NOT_SUPPORTED)
    return (0, DIRECT, radix, int(radix == 16 or lean), pre, 0, 0)


def grid():
    """the loops of front_pick_check.cpp, in its order; trigger: 0 none, 1 swap_iq, 2 swap_hist != swap_iq,
    3 scale_i_hist != scale_i, 4 scale_q_hist != scale_q, 5 scale_i != scale_q (nb_on, the sixth, is an axis of its own)"""
    for fft_l in (256, 512, 1024, 2048, 4096, 300):
        for decim in (1, 4, 2):
            for lean in (0, 1):
                for fir_fd in range(5):
                    for fir_matrix in (0, 1):
                        for nb_on in (0, 1):
                            for to_mid in (0, 1):
                                for have_rd_mask in (0, 1):
                                    for trigger in range(6):
                                        yield fft_l, decim, lean, fir_fd, fir_matrix, nb_on, to_mid, have_rd_mask, trigger


def test_the_front_kernel_instance_of_every_setting(rdsp, tmp_path):
    exe = str(tmp_path / "front_pick_check")
    pkg = os.path.join(ROOT, "radiodsp_sdr_rx_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "csrc"), "-I", "/opt/rocm/include",
                           os.path.join(HERE, "host", "front_pick_check.cpp"), "-o", exe,
                           "-L", pkg, "-lrdsp_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    env = {k: v for k, v in os.environ.items() if k != "RDSP_NO_QUAD"}     # the measurement switch would clear Q4 behind wave-wide frames
    out = subprocess.run([exe], capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    assert out[0].split() == ["experimental", "0"] and rdsp.load().rdsp_experimental_build() == 0
    points = list(grid())
    assert len(out) - 1 == len(points) == 6 * 3 * 2 * 5 * 2 * 2 * 2 * 2 * 6
    seen = set()
    for line, pt in zip(out[1:], points):
        got = tuple(int(t) for t in line.split())
        assert got == expected(*pt), (pt, got)
        seen.add(got)
    # the grid reaches every family with every frame length it has, Q4 on and off, LEAN forced both ways, every refusal
    assert {(g[1], g[6]) for g in seen if g[0] == 0} == {(DIRECT, 0), (FD, 4), (FD, 7), (RD, 128)}
    assert {g[0] for g in seen} == {0, INVALID_VALUE, NOT_SUPPORTED}
    assert {(g[1], g[2], g[3]) for g in seen if g[0] == 0 and g[2] == 4} == {(DIRECT, 4, 0), (DIRECT, 4, 1), (FD, 4, 0), (FD, 4, 1), (RD, 4, 0)}
    assert not any(g[0] == 0 and g[2] == 16 and g[3] == 0 for g in seen)      # no full-register instance at radix 16
