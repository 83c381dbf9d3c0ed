/*
 * rdsp_engine.hip -- `AudioSDR SDR;` (RadioDSP_SDR_RX.ino:54; wired :81-86, configured :117-139, driven from
 * RDSP_controls.h:149-423) for n_channels receivers on one GPU, computing what the reference's engine computes.
 *
 * The engine is Derek Rowell's AudioSDR library, which is not in the reference tree; what the reference holds of it is
 * its compiled code in pre_compiled/RadioDSP_SDR_RX.ino.hex (AudioSDR::update at ITCM 0xe730).  The arithmetic of the
 * kernels follows that code stage by stage -- which products are rounded before they are added, which are fused, where it widens
 * to double, its truncating conversions -- so that, on the same int16 IQ, this object returns the int16 audio the
 * image's update() returns (tests/test_engine_kat.py: the known answers are the image's own, recorded under the
 * interpreter of tests/golden/).  It is a low-IF receiver: IQ / 32767 x gains -> [impulse blanker] -> IF band-pass
 * (4 biquad sections per rail) -> table oscillator shifts the carrier to 0 Hz -> I delayed 128 samples, Q through a
 * 257-tap Hilbert transformer, sum or difference picks the side band  (AM: second IF pass, shift by the IF, low-pass,
 * envelope; SAM: a PLL on the IF signal with the envelope detector as its out-of-lock fallback) -> audio band-pass
 * -> hang AGC (peak envelope, gain by a curve) -> ALS line enhancer (delayed-input LMS) -> x output gain x 32767.
 *
 * Mapping to the machine.  Every stage but the Hilbert transformer is a recursion in time that has to be evaluated in the
 * image's order, so the parallel axes are channels, rails and -- for the transformer -- samples; and a lone wave issues an
 * instruction every five cycles or so whatever it depends on, so a launch lasts as long as ONE workgroup's chain of
 * instructions per block, times the blocks.  Hence: few channels per workgroup (8), the sections of a cascade on the four
 * lanes of a quad (sample n enters section s at step n + s), everything that is a pure function of a recursion's state
 * (table look-ups, gain curve, conversions, pack) spread over all lanes behind a recursion reduced to its few dependent
 * operations, and the passes of a block on different waves, each a block behind the previous one's:
 *   rdsp_engine_front_pipe_kernel  SSB / CW, no blanker: waves 2 + 3 convert block s and rotate / store block s - 2, wave 0
 *                              runs the IF cascades of block s - 1 (16 rows x 4 sections), wave 1 the oscillator's phase
 *   rdsp_engine_front_kernel   blanker, AM, SAM: the same passes one after the other (the PLL and the blanker's running
 *                              average are long recursions of their own)
 *   rdsp_engine_hilbert_kernel eight outputs of one parity per lane, sliding windows in registers, LDS split by parity
 *   rdsp_engine_tail_pipe_kernel   waves 2 + 3 load block s and finish block s - 3 (gain by the curve, clamp, pack), wave 0
 *                              the audio cascade of block s - 1, wave 1 the AGC envelope of block s - 2
 *   rdsp_engine_tail_kernel    with the ALS filter: its 55-tap chain on the lanes of a quad (the four samples between two
 *                              tap moves), taps in registers
 * int16 rows enter and leave in coalesced 256-byte segments through LDS tiles at a 129-word pitch.  The three launches of a
 * call are stream-ordered; a call takes any number of 128-sample blocks up to the engine's max_blocks_per_call.  HBM
 * traffic is 8 B per sample of algorithm (int16 IQ in, int16 L = R out) plus 28 B of float intermediates (the ring and the
 * audio row): the path is bound by the latency of its recursions, not by bandwidth.
 *
 * The image's addresses, their stages and where they are:
 *   0xe7b4  conversion: / 32767 and the rail's gain          convert_block                 rdsp_engine_front.hip
 *   0xe14c  impulse blanker                                   Blanker                       rdsp_engine_front.hip
 *   0xe94e  IF band-pass, shift by the tuning offset          cascade_row, phase_row, rotate_sample  (rdsp_engine_dev.h),
 *                                                             both front kernels            rdsp_engine_front.hip
 *   0xec1c  AM / SAM: the IF filter a second time             rdsp_engine_front_kernel      rdsp_engine_front.hip
 *   0xe390  SAM: the PLL                                      SamPll                        rdsp_engine_front.hip
 *   0xed02  AM, SAM out of lock: shift, low-pass, envelope    am_detector                   rdsp_engine_front.hip
 *   0xea7e  delay and Hilbert transformer, side band          rdsp_engine_hilbert_kernel    rdsp_engine_hilbert.hip
 *   0xd944  audio band-pass                                   both tail kernels             rdsp_engine_tail.hip
 *   0xdb58, 0xdc10  hang AGC: envelope; gain, clamp           agc_envelope, agc_gain_clamp  rdsp_engine_laws.h
 *   0xda24  ALS line enhancer                                 als_block                     rdsp_engine_laws.h
 *   0xebfa  output word                                       engine_out_word               rdsp_engine_laws.h
 * What more than one stage uses (the table oscillator, the cascade on a quad, the walk over a tile, a lane's roles) is
 * rdsp_engine_dev.h.
 *
 * Three of the engine's tables have no closed form (fifteen sets of four biquad sections, 64 Hilbert taps): the host
 * loads them (rdsp_engine_load_tables; tests take them from tests/golden/firmware_tables.npz); update() refuses to run
 * without them.  The sine table and the AGC's gain curve are generated by the host the way the library generates them.
 *
 * The hang AGC, the ALS filter and the output word are the pieces of rdsp_engine_laws.h, which the chain's engine-law
 * tail stage (rdsp_tail_engine.hip) calls too; the two tail kernels keep their lanes, tiles and HBM layouts.
 *
 * The host object (settings, receiver groups, shared sources, state blobs, the C-ABI) is rdsp_engine_host.hip; it hands
 * rdsp_engine_launch, below, one group's arguments (rdsp_engine_int.h).  The stage files are compiled with
 * -ffp-contract=off: every fused operation in them is written as one (fmaf / fma).
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_int.h"

using namespace rdsp_eng;

hipError_t rdsp_engine_launch(const EngParams &p, bool blanker, bool als, hipStream_t s) {
  engine_launch_front(p, blanker, s);
  engine_launch_hilbert(p, s);
  engine_launch_tail(p, als, s);
  return hipGetLastError();
}
