/*
 * rdsp.h -- C-ABI of the MI355X-native many-channel SDR receive chain.
 *
 * Drop-in boundary for the per-block IQ receive path of gcallipo/RadioDSP_SDR_RX.
 * Every entry point cites the reference interface it replaces (paths relative
 * to /root/reference/src):
 *   CONV = RadioDSP_SDR_RX/RDSP_convolutional.h   NR  = RadioDSP_SDR_RX/RDSP_noise_reduction.h
 *   SPEC = backup/RDSP_convolutional_spec.h       INO = RadioDSP_SDR_RX/RadioDSP_SDR_RX.ino
 *   CTL  = RadioDSP_SDR_RX/RDSP_controls.h        FFTIQ = RadioDSP_SDR_RX/analyze_fft256iq.{h,cpp}
 *
 * The reference keeps all DSP state in single-instance globals (CONV:34-80,
 * NR:18-32); here the same functions take a context pointer, and one context
 * (`rdsp_chain_t`) holds n_channels independent receivers on one GPU.  Plain C:
 * pointers and sizes only.  `d_` pointers are device (HBM) addresses, `stream`
 * is a hipStream_t passed as void*.  All functions returning int return
 * RDSP_OK (0) or a negative RDSP_ERR_*; rdsp_last_error() gives the text.
 * There is no CPU fallback: without a GPU every compute call fails loudly.
 */
#ifndef RDSP_H
#define RDSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDSP_BLOCK_SAMPLES 128 /* AUDIO_BLOCK_SAMPLES / BUFFER_SIZE, CONV:34, FFTIQ.cpp:44 */

enum {
  RDSP_OK = 0,
  RDSP_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
  RDSP_ERR_NO_DEVICE = -2,   /* no HIP device: the product has no CPU path */
  RDSP_ERR_HIP = -3,         /* a HIP runtime call failed */
  RDSP_ERR_NOT_READY = -4,   /* not enough queued input (CONV:231) */
  RDSP_ERR_UNSUPPORTED = -5, /* declared engine feature not built yet */
  RDSP_ERR_NOMEM = -6
};

/* demodulator modes: engine enum of CTL:330-410 (+ IQ = literal CONV:314-318) */
typedef enum {
  RDSP_DEMOD_IQ = 0,
  RDSP_DEMOD_USB = 1,    /* USBmode    */
  RDSP_DEMOD_LSB = 2,    /* LSBmode    */
  RDSP_DEMOD_CW_USB = 3, /* CW_USBmode */
  RDSP_DEMOD_CW_LSB = 4, /* CW_LSBmode */
  RDSP_DEMOD_AM = 5,     /* AMmode     */
  RDSP_DEMOD_SAM = 6     /* SAMmode (CTL:387): PLL synchronous detector, build-defined */
} rdsp_demod_t;
typedef enum { RDSP_AGC_OFF = 0, RDSP_AGC_FAST = 1, RDSP_AGC_MEDIUM = 2, RDSP_AGC_SLOW = 3 } rdsp_agc_t; /* CTL:200-218 */
typedef enum { RDSP_ALS_OFF = 0, RDSP_ALS_NOTCH = 1, RDSP_ALS_PEAK = 2 } rdsp_als_t;                    /* CTL:250-261 */
/* SDR.setAudioFilter enum, CTL:153-177,396 */
typedef enum { RDSP_AUDIO_CW = 0, RDSP_AUDIO_2100 = 1, RDSP_AUDIO_2700 = 2, RDSP_AUDIO_3100 = 3,
               RDSP_AUDIO_AM = 4, RDSP_AUDIO_WSPR = 5 } rdsp_audio_filter_t;

/* One configuration shared by all channels of a chain (the reference's
 * compile-time constants CONV:34-38,66-72 and run-time globals GEN:76-111). */
typedef struct {
  double fs_in;         /* input IQ rate, Hz (AUDIO_SAMPLE_RATE_EXACT role, CONV:35) */
  int32_t decim;        /* 1 = no decimator (reference-native), 4 = polyphase /4   */
  int32_t fir_taps;     /* decimator taps, 256                                       */
  double fir_cut_hz;    /* decimator low-pass half-width, Hz                         */
  double nco_hz;        /* tuning offset removed by the mixer (TuningOffset, INO:139) */
  int32_t fft_l;        /* FFT_L, CONV:36: 256 512 1024 2048 4096                    */
  int32_t window;       /* FIR_filter_window, CONV:66 (1 = Blackman-Harris)          */
  double flo_hz;        /* FLoCut, CONV:67                                           */
  double fhi_hz;        /* FHiCut, CONV:68                                           */
  int32_t filter_on;    /* bFilterEnabled, CONV:228,300                              */
  int32_t demod;        /* rdsp_demod_t                                              */
  int32_t spectral_nr;  /* spectral-subtraction NR: 0 off, 1 SPEC:112-269, 2 the older
                           variant of backup/RadioDSP_SDR_RX_Conv.ino:1520-1669 (bins
                           60..120, /60, x3, no smoothing; the sketch runs it at nrndx == 3) */
  float spectral_level; /* iNRLevel of SPEC:112,202                                  */
  int32_t lms_nr;       /* nr_level: 0 off, else DSP-NR strength, CONV:326, NR:35    */
  int32_t als_mode;     /* rdsp_als_t                                                */
  int32_t als_strength; /* mu law input for the ALS instance                         */
  int32_t agc_mode;     /* rdsp_agc_t                                                */
  float input_gain;     /* SDR.setInputGain, INO:133                                 */
  float output_gain;    /* SDR.setOutputGain, INO:134                                */
  float iq_balance;     /* SDR.setIQgainBalance, INO:135                             */
  int32_t mute;         /* SDR.setMute, INO:177                                      */
} rdsp_chain_config_t;

typedef struct rdsp_chain rdsp_chain_t;

const char *rdsp_last_error(void);
const char *rdsp_version(void);
/* Always 0: there is one build of the library.  The kernel variants that were measured and not adopted (matrix-core
 * FIR and tail reductions, half-row / DPP-shift tail layouts: docs/history.md) are not in it -- a build that carried
 * them answered 1 -- and the variant setters below return RDSP_ERR_UNSUPPORTED for them. */
int rdsp_experimental_build(void);
int rdsp_device_count(void);

/* ---- host-side design helpers ---------------------------------------------*/
/* calc_cplx_FIR_coeffs, CONV:127 (window id added as a parameter: the
 * reference reads the global FIR_filter_window, CONV:66) */
void rdsp_calc_cplx_FIR_coeffs(double *coeffs_I, double *coeffs_Q, int numCoeffs, double FLoCut,
                               double FHiCut, double SampleRate, int window);
/* init_filter_mask, CONV:87: natural-order mask, 2*fft_l floats */
int rdsp_init_filter_mask(float *mask, const double *coef_I, const double *coef_Q, int fft_l);

/* ---- chain: n_channels receivers on one GPU ---------------------------------*/
/* max_blocks_per_call sizes the intermediate audio buffer (no allocation ever
 * happens inside rdsp_chain_process). */
int rdsp_chain_create(const rdsp_chain_config_t *cfg, int n_channels, int device,
                      int max_blocks_per_call, rdsp_chain_t **out);
void rdsp_chain_destroy(rdsp_chain_t *c);
int rdsp_chain_channels(const rdsp_chain_t *c);
/* number of 128-sample input blocks per call must be a multiple of this
 * (N_BLOCKS of CONV:38-39 seen from the input rate: 8 for FFT_L <= 512 at decim 4) */
int rdsp_chain_call_unit_blocks(const rdsp_chain_t *c);
/* The unit a stream is cut in for output bits that do not depend on the cut.  The call unit for the default
 * decimator, the direct form and decim-1 chains (any call split gives the same bits).  With the 448-sample decimator
 * frames of rdsp_chain_set_fir_variant(c, 2) -- 14 input blocks a frame -- lcm(14, call unit): 56 blocks for
 * FFT_L <= 512.  Calls of whole granules are whole frames, the frame grid then sits at absolute stream positions,
 * and the stream gives the same bits however it is cut into such calls: restricting the call boundaries is how the
 * reference has the property too (`available() > N_BLOCKS`, CONV:231).  Other multiples of the call unit are
 * accepted in that form; such a call ends in a partial frame and re-anchors the grid at the next call's first
 * sample (valid output, rounds differently: <= 3e-7 of the peak). */
int rdsp_chain_granule_blocks(const rdsp_chain_t *c);
/* zero all per-channel state (overlap block, FIR history, NLMS, NFloor, AGC); settings kept.  An engine-literal chain
 * (rdsp_sdr_set_engine_literal) also resets its pre-processor (rdsp_preproc_reset: detection off until
 * rdsp_pre_startAutoI2SerrorDetection is called again, a one-shot command) and its engine (rdsp_engine_reset). */
int rdsp_chain_reset(rdsp_chain_t *c, void *stream);

/* doConvolutionalInitialize(), CONV:187 */
int rdsp_doConvolutionalInitialize(rdsp_chain_t *c, void *stream);
/* reInitializeFilter(lo, hi), CONV:209 (PBT retune path CTL:569-612) */
int rdsp_reInitializeFilter(rdsp_chain_t *c, double dFLoCut, double dFHiCut, void *stream);
/* Init_LMS_NR(strength), NR:35 */
int rdsp_Init_LMS_NR(rdsp_chain_t *c, int LMS_nr_strength, void *stream);

/* LMS_NoiseReduction(blockSize, nrbuffer), NR:66: the DSP-NR NLMS instance
 * alone, in place on float audio d_nrbuffer[n_channels][stride]; n_samples per
 * channel, a multiple of 128 (the reference calls it with 128, CONV:332) */
int rdsp_LMS_NoiseReduction(rdsp_chain_t *c, int n_samples, float *d_nrbuffer, size_t stride,
                            void *stream);

/* ---- the law of the chain's tail: A8 ALS notch / peak and A9 AGC ---------------------------------------------
 * RDSP_TAIL_BUILD (the default): this build's stand-ins -- A8 a 96-tap NLMS instance on the DSP-NR core, A9 a per-block
 * RMS gain -- in the order ALS, AGC.  RDSP_TAIL_ENGINE: the reference engine's own laws (AudioSDR, restated from the
 * firmware image; rdsp_engine_t runs them too), bit for bit with the image's stage taps:
 *   Order.  [A7 DSP-NR NLMS if lms_nr > 0, unchanged, x 1.1 as CONV:334] -> engine AGC -> engine ALS -> output gain ->
 *     the chain's pack (arm_float_to_q15 rounding, L = R; not the engine's truncating wrap).  d_out_f32 is the parity
 *     surface.  Spectral stage, IIR bank and SAM in front are unchanged.
 *   AGC (0xdb58).  Peak envelope with attack, hang counter and decay; the gain is looked up from the generated 130-entry
 *     curve (0xdd40: trunc((double)env x 32767), fmaf interpolation), then (g x 10) x, clamped to +-1.  The chain's
 *     agc_mode 1 .. 3 at creation, and rdsp_sdr_setAGCmode(c, k), select the image's set k (0xdfe0: fast / medium / slow);
 *     mode 0 switches the AGC off and keeps the set; enableAGC / disableAGC switch it on / off as the engine's do.
 *     Before any set is selected the constructor's applies (0xdf14: medium attack, slow decay, hang 4410).
 *   ALS (0xda24).  55 taps, delay 3, mu 0.5, always adaptive (the image has no setter for it): the taps move on the
 *     first and every fourth sample of each block, in the image's serial fmaf order.  als_mode RDSP_ALS_NOTCH outputs
 *     the error, RDSP_ALS_PEAK the prediction; als_strength is ignored.  rdsp_sdr_enableALSfilter clears the line and
 *     the taps at the next launch (0xdb2c).
 *   Rate.  Both laws are defined per sample, as the image stores them, and are not rescaled: at the chain's 24 kHz
 *     audio (96 kHz / 4) the hang times of the fast / medium / slow sets are 0.18 / 0.92 / 3.7 s, not the 0.1 / 0.5 /
 *     2.0 s they are at the engine's 44.1 kHz, and the attack / decay time constants stretch by the same 1.84.
 *   Where it runs.  With the engine law and the AGC or the ALS filter on, a tail stage follows the front kernel (the
 *     front kernel's own AGC stays off); the default decimator picks its tail-side form accordingly.
 *   State.  Per channel: envelope, gain, hang counter, active flag, the ALS line's newest 64 samples and the 55 taps;
 *     allocated by the first switch to RDSP_TAIL_ENGINE, at the engine constructor's values (gain 0, active 1, the rest
 *     0).  Switching law resets the tail state of the law switched to (RDSP_TAIL_BUILD: ALS instance cleared, AGC gain
 *     1); setting the current law again changes nothing.  rdsp_chain_reset returns it to those values;
 *     rdsp_chain_get_scalars slot 1 reports the engine AGC's gain; rdsp_chain_get_status reports no ALS bits under this
 *     law; rdsp_chain_save_state / load_state carry it as an optional part once it is allocated (a blob that carries it
 *     loads only into a chain switched to RDSP_TAIL_ENGINE first).  Chains that never switch keep their blobs.
 *   Channel groups share the chain-wide AGC / ALS settings.  A set-up call: not while calls are in flight. */
typedef enum { RDSP_TAIL_BUILD = 0, RDSP_TAIL_ENGINE = 1 } rdsp_tail_law_t;
/* RDSP_ERR_INVALID for a law outside {0, 1}; RDSP_ERR_UNSUPPORTED for RDSP_TAIL_ENGINE on an engine-literal chain
 * (rdsp_sdr_set_engine_literal: there the setters reach the engine object itself) */
int rdsp_chain_set_tail_law(rdsp_chain_t *c, int law);
int rdsp_chain_get_tail_law(const rdsp_chain_t *c);
/* the engine-law AGC then ALS filter (as the chain's settings select them), in place on float audio
 * d_audio[n_channels][stride], n_samples a positive multiple of 128; carries the chain's own tail state.  No NR, no
 * output gain, no pack.  RDSP_ERR_UNSUPPORTED under RDSP_TAIL_BUILD. */
int rdsp_chain_run_tail_f32(rdsp_chain_t *c, float *d_audio, size_t stride, int n_samples, void *stream);

/* The hot path.  doConvolutionalProcessing (CONV:228 / SPEC:112) with the
 * engine stages in front and behind it, for every channel, over n_blocks
 * input blocks of 128 IQ samples per channel.
 *   d_iq   : int16 [n_channels][in_stride][2]   (I, Q interleaved)
 *   d_out  : int16 [n_channels][out_stride][2]  (L, R interleaved), receives
 *            n_blocks*128/decim sample pairs per channel
 *   d_out_f32 : optional float [n_channels][out_stride][2], the same audio
 *            before arm_float_to_q15 (parity tests)
 * strides are in samples (pairs); in_stride must be a multiple of 4. */
int rdsp_chain_process(rdsp_chain_t *c, const int16_t *d_iq, size_t in_stride, int n_blocks,
                       int16_t *d_out, size_t out_stride, float *d_out_f32, void *stream);
/* reference-shaped call: nr level and filter enable per call (CONV:228);
 * the cut-off arguments are ignored exactly as in the reference (CONV:300). */
int rdsp_doConvolutionalProcessing(rdsp_chain_t *c, float iNRLevel, int bFilterEnabled,
                                   double dFLoCut, double dFHiCut, const int16_t *d_iq,
                                   size_t in_stride, int n_blocks, int16_t *d_out,
                                   size_t out_stride, void *stream);

/* arm_q15_to_float / arm_float_to_q15 call sites CONV:241-242,346-347.  q / 32768.0f; and, in the variant the reference's
 * firmware image holds (CMSIS under ARM_MATH_ROUNDING): in = x * 32768, in += in > 0 ? 0.5f : -0.5f, (q15_t)__SSAT((q31_t)in,
 * 16) -- round to nearest, halves away from zero, saturating; finite input.  Every int16 output of the library is packed
 * this way. */
int rdsp_q15_to_float(const int16_t *d_src, float *d_dst, size_t n, void *stream);
int rdsp_float_to_q15(const float *d_src, int16_t *d_dst, size_t n, void *stream);

/* ---- engine setters: AudioSDR API visible at INO:117-139, CTL:149-423 ------*/
int rdsp_sdr_enableAGC(rdsp_chain_t *c);                          /* INO:120 */
int rdsp_sdr_disableAGC(rdsp_chain_t *c);                         /* CTL:268 */
int rdsp_sdr_setAGCmode(rdsp_chain_t *c, int mode);               /* INO:121, CTL:200-218 */
int rdsp_sdr_enableALSfilter(rdsp_chain_t *c);                    /* CTL:259 */
int rdsp_sdr_disableALSfilter(rdsp_chain_t *c);                   /* INO:125 */
int rdsp_sdr_setALSfilterNotch(rdsp_chain_t *c);                  /* CTL:260 */
int rdsp_sdr_setALSfilterPeak(rdsp_chain_t *c);                   /* BK_INO:665 */
int rdsp_sdr_setALSfilterAdaptive(rdsp_chain_t *c);               /* CTL:261 */
/* noise blanker: engine feature, arithmetic build-defined: on the
 * wide-band IQ stream before the mixer, a sample whose power exceeds the reference
 * level by threshold dB (default 10, range 0..60) is zeroed; the reference level is
 * the smoothed mean power of the previous windows of 256*decim input samples */
int rdsp_sdr_enableNoiseBlanker(rdsp_chain_t *c);                 /* BK_INO:1259 */
int rdsp_sdr_disableNoiseBlanker(rdsp_chain_t *c);                /* INO:131 */
int rdsp_sdr_setNoiseBlankerThresholdDb(rdsp_chain_t *c, float db); /* BK_INO:1260 */
/* AudioSDRpreProcessor */
/* swapIQ and the input-side gains take effect with the first sample of the next call (samples
 * already inside the decimator's delay line keep what they came in with) */
int rdsp_pre_swapIQ(rdsp_chain_t *c, int swap);                   /* INO:118 */
int rdsp_pre_startAutoI2SerrorDetection(rdsp_chain_t *c);         /* INO:117: accepted; there is no I2S bus to watch at run time */
/* What INO:117 guards against is an I2S fault that leaves one rail of the codec stream a sample behind
 * the other; a RECORDING made through such a front end carries it (the image rejection of the
 * quadrature pair is gone).  rdsp_estimate_iq_slip finds it in a recording (host, no GPU),
 * rdsp_pre_setIQslip corrects it: slip +1 pairs I[n-1] with Q[n] (delays the I rail by one sample),
 * -1 pairs I[n] with Q[n-1], 0 switches the correction off.  It acts on the raw words in a pass of
 * its own in front of the front kernel (8 bytes of HBM traffic per input sample while it is on), before
 * swapIQ and the input gains, on samples as they arrive from the next call on.  The first non-zero
 * value allocates the corrected-input buffer (n_channels x max_blocks_per_call x 128 words): a set-up
 * call.  Build-defined (the AudioSDR pre-processor is not in the reference tree).  A non-zero slip on an
 * engine-literal chain is refused (RDSP_ERR_UNSUPPORTED): its pre-processor repairs the slip itself. */
int rdsp_pre_setIQslip(rdsp_chain_t *c, int slip);
/* iq: n_samples interleaved int16 I,Q pairs of ONE channel (host memory).  *slip: the value to pass to
 * rdsp_pre_setIQslip; rejection_db (optional, 3 values): image rejection of the strongest line with the
 * slip undone as 0, +1, -1.  Needs a dominant one-sided line in the first 2^k samples (k <= 14); without
 * one (noise, a real-valued or double-side-band signal: all three rejections near 0 dB) *slip is 0 -- a
 * correction is only recommended when it rejects the image by 15 dB at least and beats "no slip" by 10 dB. */
int rdsp_estimate_iq_slip(const int16_t *iq, size_t n_samples, int *slip, double *rejection_db);
int rdsp_sdr_setInputGain(rdsp_chain_t *c, float g);              /* INO:133 */
int rdsp_sdr_setOutputGain(rdsp_chain_t *c, float g);             /* INO:134 */
int rdsp_sdr_setIQgainBalance(rdsp_chain_t *c, float g);          /* INO:135 */
int rdsp_sdr_enableAudioFilter(rdsp_chain_t *c);                  /* INO:137 */
int rdsp_sdr_setAudioFilter(rdsp_chain_t *c, int filter, void *stream); /* INO:138, CTL:153-177 */
/* returns the tuning offset in Hz like the reference (INO:139, CTL:337-407) -- the AudioSDR engine's own answers, read
 * by running its constructor and setDemodMode out of the reference's firmware image (tests/test_firmware_kat.py): a low
 * IF centred on 6890 Hz, the carrier half a band (SSB 3000 Hz, CW 1000 Hz) above it for the lower and below it for the
 * upper side band: LSBmode 8390, USBmode 5390, CW_LSBmode 7390, CW_USBmode 6390, AMmode / SAMmode 6890 (RDSP_DEMOD_IQ,
 * the literal CONV stage: 0).  The sketch puts its LO at vfoFreq - TuningOffset (CTL:447) and the engine moves the
 * carrier from there to 0 Hz itself; in this library the mixer is a setting of its own, so a host that mirrors the
 * sketch hands the returned value to rdsp_sdr_setTuningOffsetHz (tests/host/rdsp_binding.h does), and a host with many
 * carriers in one recorded stream sets each group's mixer to where its carrier is.  The engine's modes pick
 * the side band the selected audio filter sits on, so the pass band is re-applied for the new mode
 * (USB/CW_USB: +a..+b, LSB/CW_LSB: -b..-a, AM/SAM: -b..+b of setAudioFilter's a..b); a later
 * rdsp_reInitializeFilter / PBT step overrides it, as RDSP_controls.h:569-612 does in the sketch. */
uint32_t rdsp_sdr_setDemodMode(rdsp_chain_t *c, int mode, void *stream);
int rdsp_sdr_setMute(rdsp_chain_t *c, int mute);                  /* INO:177 */
int rdsp_sdr_setTuningOffsetHz(rdsp_chain_t *c, double hz);       /* NCO side of CTL:447 */
int rdsp_set_nr_level(rdsp_chain_t *c, int nr_level);             /* nr_level, GEN:111, CTL:237-297 */
/* The window energy of arm_lms_norm_f32 (NR:73) in both NLMS instances.  running = 0 (default): the reference's running
 * difference, re-started from the exact 96-sample window sum at every 128-sample block -- a deviation from NR:73, made
 * because the reference's own float32 recursion leaves `energy + 1.19e-7 <= 0` after loud-to-quiet transitions (164 of
 * 320 in tests/test_gpu_parity.py) and can lose a channel for good; on ordinary signals the two agree to the reference's
 * accumulated rounding (~1e-6).  running = 1: no anchor -- one running sum for the whole stream like NR:73's, but in the
 * kernel's own form: the increments are fused x^2 - q^2 terms added by a 16-lane prefix scan, where arm_lms_norm_f32
 * subtracts and adds sample by sample.  Neither bit-equal to the reference's recursion nor statistically the same (the
 * scan form draws bad residues more often: 90 channels flagged / 8 lost on the loud-to-quiet test against 1 in the CPU
 * restatement); tested <= 1e-5 against the oracle, which always runs the reference's form, and 4.0e-4 (against 1.3e-4 in
 * the default mode) from the firmware image's own output on the `conv_fade` fixture. */
int rdsp_set_nlms_energy_mode(rdsp_chain_t *c, int running);
int rdsp_set_spectral_nr(rdsp_chain_t *c, int on, float level);   /* on: 0, 1 (SPEC:112 iNRLevel), 2 (older variant, level unused) */
/* How the spectral stage rebuilds a bin from its new magnitude (SPEC:221-235).  literal = 1: as the file writes it,
 * `mag' * arm_cos_f32(phi)`, `mag' * arm_sin_f32(phi)` with `phi = atan2(im, re)` -- CMSIS-DSP's table sine (513
 * entries, linear interpolation) restated from the published routine.  literal = 0 (default): the exact-arithmetic
 * equivalent X mag'/mag.  The two sit 1.7e-5 ... 1.9e-5 of the output's peak apart (the table's interpolation error,
 * (2 pi / 512)^2 / 8), so "within 1e-5 of the reference's CPU path" can only hold for one of them at a time: each form
 * is tested <= 1e-5 against the oracle evaluating the SAME form (tests/test_gpu_parity.py).  literal = 1 evaluates
 * the table's interpolation in closed form (csrc/rdsp_front_frame.h spec_table_factor: the as-written bin is the exact one
 * times 1 - (h^2 / 2) f (1 - f), f the fraction between table nodes; within 5e-8 of the table's own arithmetic, +5 % on a
 * K3 step); literal = 2 calls atan2f and looks the table up (round 5's code, +35 %); both are held to the oracle's
 * literal form. */
int rdsp_set_spectral_resynthesis(rdsp_chain_t *c, int literal);

/* ---- receiver groups: per-group retune / PBT / mode tables -------
 * The sketch has one receiver, so one filter mask, one tuning offset and one
 * demodulator (globals of CONV:66-80, CTL:330-423).  A chain of many channels is
 * partitioned into groups that each carry their own; channels of a group share
 * the group's mask (a gather by group index in the kernel).  Every group call is
 * the per-group form of a reference call and is non-blocking for the processing
 * stream: the new mask is designed on the host, uploaded on an internal copy
 * stream into the group's idle mask buffer (masks are double-buffered on the
 * device) and switched in, in stream order, by the next rdsp_chain_process; calls
 * already queued keep the old mask.  The chain-wide calls above
 * (rdsp_reInitializeFilter, rdsp_sdr_setDemodMode, ...) apply to every group. */
int rdsp_chain_set_groups(rdsp_chain_t *c, int n_groups, const uint16_t *group_of_channel);
int rdsp_chain_groups(const rdsp_chain_t *c);
int rdsp_group_reInitializeFilter(rdsp_chain_t *c, int group, double dFLoCut, double dFHiCut,
                                  void *stream);                                  /* CONV:209 */
int rdsp_group_setAudioFilter(rdsp_chain_t *c, int group, int filter, void *stream); /* CTL:153-177 */
uint32_t rdsp_group_setDemodMode(rdsp_chain_t *c, int group, int mode, void *stream); /* CTL:337-407 */
int rdsp_group_setTuningOffsetHz(rdsp_chain_t *c, int group, double hz);          /* CTL:447 */
int rdsp_group_get_mask(rdsp_chain_t *c, int group, float *host_out);
/* checkPBT_Increase / checkPBT_Decrease (CTL:569-612): one 50 Hz step of the low
 * (edge 0, button D3) or high (edge 1, button D6) cut-off, dir = +1 / -1, with the
 * limits MIN_LOW 0, MAX_LOW 700, MIN_HI 800, MAX_HI 4000 (GEN:79-82) and the
 * reference's comparisons.  rdsp_pbt_step is the pure host function; rdsp_group_pbt
 * steps a group's cut-offs and calls reInitializeFilter like CTL:575,582,597,605. */
int rdsp_pbt_step(double *dFLoCut, double *dFHiCut, int edge, int dir);
int rdsp_group_pbt(rdsp_chain_t *c, int group, int edge, int dir, void *stream);
/* tuningMode() (CTL:330-423): mndx 0 "CW N", 1 "CW", 2 "USB", 3 "LSB", 4 "AM",
 * 5 "SAM", 6 "RTTY"; the CW side follows vfoFreq > 10 MHz (CTL:337).  Sets the group's audio filter and
 * demodulator, returns TuningOffset in Hz. */
uint32_t rdsp_group_tuningMode(rdsp_chain_t *c, int group, int mndx, double vfo_hz, void *stream);

/* ---- pipelined mode (streaming throughput) -------------------------------------
 * The NLMS/AGC tail stage is serial in time, so its duration is set by the batch
 * length, not by the channel count.  With pipelining on, the tail stage of call k
 * runs on an internal stream concurrently with the front stage of call k+1 (the
 * intermediate audio lives in three buffers).  rdsp_chain_process then returns with
 * the tail possibly still queued: d_out of a call is complete after the next
 * rdsp_chain_flush(c, stream) on the consuming stream. */
int rdsp_chain_set_pipelined(rdsp_chain_t *c, int on);
int rdsp_chain_flush(rdsp_chain_t *c, void *stream);
/* front-kernel variant: -1 auto (full-register), 0 full-register, 1 lean (FFT twiddles
 * rebuilt per pass from one base each: 24 fewer VGPRs, ~3 % slower) */
int rdsp_chain_set_front_variant(rdsp_chain_t *c, int lean);
/* pipelined mode launches a call in channel sub-batches of this many channels (multiple of 64,
 * default 4096, 0 = off) once the chain has at least 1.5 of them: every launch then has the shape
 * the two kernels share a SIMD at, and the sub-batches of one call overlap each other (8192
 * channels: -8 % per step).  Outputs do not depend on it, bit for bit. */
int rdsp_chain_set_sub_batch(rdsp_chain_t *c, int channels);

/* wave priorities in pipelined mode (front kernel during its FIR, tail kernel), 0..3 */
int rdsp_chain_set_priorities(rdsp_chain_t *c, int front_fir_prio, int tail_prio);
/* stage A3 (the decimating FIR, y[m] = sum_k h[k] x[4m - k]; decim 4).  4: in the frequency
 * domain -- polyphase overlap-save: four low-rate transforms, branch spectra, one inverse -- with
 * frames of ONE GRANULE (256 outputs, the rest of the 512-point window zeros): every call boundary is a frame
 * boundary and every frame's input is a function of the absolute sample position, so a stream gives the same
 * bits however it is cut into calls -- the property the reference has by construction (fixed 128-sample
 * blocks, CONV:231-245).  -1 (default): that form, or the row form 5 (below; split-invariant in the same way) for a
 * call that no later stage follows -- no NLMS / ALS / SAM / IIR stage, whose kernel would share the SIMDs -- and
 * that runs without the noise blanker: a function of the chain's settings at the call, never of the call split.
 * 0: the direct form (packed FMAs): split-invariant too, about 1.3x slower.  2: the
 * frequency domain with 448-sample frames: 5 transforms per 448 outputs instead of per 256 (the front kernel
 * ~1.4x faster).  The frames start at the call's first sample, so this form has the property for a restricted
 * set of call boundaries: calls that are multiples of rdsp_chain_granule_blocks() (56 input blocks for FFT_L <=
 * 512) are whole frames and give the same bits for any split into such calls
 * (test_throughput_decimator_is_split_invariant_on_whole_frames); any other multiple of the call unit is accepted
 * and ends in a partial frame -- another split then frames and rounds differently (2.6e-7 of the output's peak
 * over random splits, 2.8e-6 through K3's recursive stages: tests/test_gpu_parity.py pins both).  bench.py selects 2
 * with BASELINE.md's 512-block steps (9 frames and a partial one) and says so in its `config`.  5: the
 * frequency domain on 16-lane rows (rdsp_front_rd_kernel: 256-point windows, four per wave, 128 outputs each, two
 * frames per granule): split-invariant like the default and ~10 % faster than it for chains without a tail stage
 * (K2 0.727 against 0.808 ms per step), no gain beside a tail kernel; with the noise blanker on it runs the default
 * form.  All of them are the same exact linear convolution with the same taps (RDSP_ERR_UNSUPPORTED for 2 / 4 / 5
 * on decim-1 chains, which have no decimator).  RDSP_ERR_UNSUPPORTED, measured and not adopted (docs/history.md):
 * 1 matrix-core GEMM slices, 3 the same unless the tail stage shares the SIMDs, 6 the row form with 192 outputs
 * per window.
 * One more thing decides how the wave-wide frequency-domain forms (2, 4 and the default beside a tail stage) round: the
 * number of receiver groups.  A chain of at most 64 groups keeps, per group, the decimator's branch spectra multiplied by
 * the mixer's rotations of the branches (rebuilt on the host at every retune) and mixes every branch with one phasor per
 * quad column; above 64 groups each branch's phasors are rotated per frame on the device.  Where the filter's transform
 * is at most 1024 points long, a chain of at most 64 groups goes one step further: it keeps the branch spectra of the
 * decimator's taps shifted by the group's tuning offset, transforms the unmixed samples and mixes behind the decimator, on
 * a quarter of the samples (FFT_L 2048 and 4096 keep the rotated spectra).  The same arithmetic to 1e-6
 * of the output's peak, not to the bit: rdsp_chain_set_groups across that threshold changes the last bits of what
 * follows, like a change of variant.  Within either range calls, splits, pipelining and sub-batches give the bits they
 * gave before. */
int rdsp_chain_set_fir_variant(rdsp_chain_t *c, int variant);
/* tail-kernel variant: (16, 2) is the kernel there is -- a channel per 16-lane DPP row, two steps per
 * DPP reduction, delay line fed from LDS.  RDSP_ERR_UNSUPPORTED, measured and not adopted (docs/history.md): (16, 4)
 * weights one block stale with a hand-interleaved issue order, (16, 3) one reduction per step, (8, 2) half a row per
 * channel, (16 | 8, 1) cross-lane sums on the matrix pipe, (16, 0) delay line shifted by DPP */
int rdsp_chain_set_tail_variant(rdsp_chain_t *c, int lanes_per_channel, int matrix_reduce);

/* ---- per-kernel timing (HIP events on the launch stream; measurement only) ---*/
int rdsp_chain_set_timing(rdsp_chain_t *c, int on);
/* name of the front kernel the most recent call launched, as a profiler shows it without template
 * arguments: "rdsp_front_fd_kernel" (stage A3 in the frequency domain) or "rdsp_front_kernel" */
const char *rdsp_chain_front_kernel_name(const rdsp_chain_t *c);
/* total milliseconds spent in the front and tail kernels over `calls` calls */
int rdsp_chain_get_timing(rdsp_chain_t *c, double *front_ms, double *tail_ms, int *calls);
/* milliseconds between the end of the first and of the last recorded call (calls - 1 steady-state periods
 * of a pipelined sequence: what a long stream pays per call, without the pipeline's fill) */
int rdsp_chain_get_timing_span(rdsp_chain_t *c, double *span_ms, int *calls);

/* ---- state read-back (tests, checkpoint/resume) ------------------------------*/
/* scal: float[n_channels][4] = NFloor (SPEC:109), AGC gain, AM DC, noise-blanker level */
int rdsp_chain_get_scalars(rdsp_chain_t *c, float *host_out, void *stream);
/* which: 0 = DSP-NR instance (NR:31), 1 = ALS instance; float[n_channels][96] in
 * CMSIS coefficient order */
int rdsp_chain_get_lms_coeffs(rdsp_chain_t *c, int which, float *host_out, void *stream);
/* Per-channel health word, host_out[n_channels].  The reference's NLMS keeps its window energy as a
 * running difference (RDSP_noise_reduction.h:73 -> arm_lms_norm_f32): after a loud-to-quiet transition
 * the residue can leave energy + 1.19e-7 at or below zero, the step size turns negative or infinite
 * and the channel's weights run away to +-inf -- the reference's own behaviour, reproduced here.  The
 * tail kernel records it per channel: bits are sticky until rdsp_Init_LMS_NR (DSP-NR instance) or
 * rdsp_chain_reset (both), the arithmetic is untouched.  Synchronises `stream` and the tail stream. */
#define RDSP_STATUS_NR_ENERGY 0x01u     /* DSP-NR: divided by energy + eps <= 0 */
#define RDSP_STATUS_NR_NONFINITE 0x02u  /* DSP-NR: a weight or the energy is inf / NaN */
#define RDSP_STATUS_ALS_ENERGY 0x10u    /* ALS notch / peak instance, likewise */
#define RDSP_STATUS_ALS_NONFINITE 0x20u
int rdsp_chain_get_status(rdsp_chain_t *c, uint32_t *host_out, void *stream);
/* Recovery for the channels the health words name: arm_lms_norm_init_f32 leaves the coefficients
 * (RDSP_noise_reduction.h:62), so Init_LMS_NR does not clear weights that have run away, and the sketch's
 * only cure is a power cycle.  which 0: the DSP-NR instance, 1: the ALS instance; weights, delay block,
 * energy and health word of channels [first_channel, first_channel + n_channels) go back to their boot
 * values, in stream order behind what is queued; every other channel continues bit for bit. */
int rdsp_chain_reset_nlms_channels(rdsp_chain_t *c, int which, int first_channel, int n_channels, void *stream);
/* natural-order filter mask currently in use, float[2*fft_l] (CONV:77) */
int rdsp_chain_get_mask(rdsp_chain_t *c, float *host_out);
int rdsp_chain_get_fir_taps(rdsp_chain_t *c, float *host_out);

/* ---- per-channel state as data (the reference's DSP state is a set of globals,
 * CONV:50-57,77-80, NR:26-32, SPEC:109; here an explicit per-channel record) ------------------------
 * Checkpoint / resume and moving channels between chains or GPUs: the state of channels
 * first_channel .. first_channel + n_channels - 1 (FIR history, overlap block, NFloor / AGC gain / AM DC /
 * blanker level, both NLMS instances, SAM PLL, IIR cascade) as one host blob.  Settings (modes, filters,
 * gains, groups) are configuration and are re-applied by the caller; FFT_L and decimation must match.
 * Loading into a chain that has not processed anything also restores the stream position and call
 * history (resume: the next call continues the stream bit for bit); a chain that has must be at the
 * same stream position.  Control-path calls: both wait for everything queued so far.
 * rdsp_chain_state_bytes is an upper bound for every later rdsp_chain_save_state of that many channels; it
 * grows only with set-up calls that allocate optional state (a SAM group, RDSP_AUDIO_KIND_IIR, the first
 * non-zero rdsp_pre_setIQslip, rdsp_chain_set_groups): size the buffer after set-up.  Blobs carry a
 * version (4 in this library); a blob of another version is refused (RDSP_ERR_INVALID), nothing is restored.
 * An engine-literal chain refuses both (RDSP_ERR_UNSUPPORTED): the blob does not carry the pre-processor's and the
 * engine's state; use rdsp_engine_save_state / load_state on rdsp_chain_engine(chain) for the engine. */
size_t rdsp_chain_state_bytes(const rdsp_chain_t *c, int n_channels);
int rdsp_chain_save_state(rdsp_chain_t *c, int first_channel, int n_channels, void *host_buf, size_t bytes, void *stream);
int rdsp_chain_load_state(rdsp_chain_t *c, int first_channel, const void *host_buf, size_t bytes, void *stream);

/* ---- recorded IQ in, audio out ----------------------------------
 * The ends of the sketch's graph are an I2S bus and a codec (AudioInputI2S IQinput,
 * AudioOutputI2S audio_out, AudioControlSGTL5000 codec: INO:52,55,159-169).  A
 * host has recordings: little-endian int16 I,Q pairs, RAW (no header) or RIFF/WAVE
 * PCM 16-bit stereo with I on the left channel and Q on the right (the codec wiring
 * INO:71-72); audio goes out as int16 L,R pairs (Q_out_L / Q_out_R, CONV:344-349). */
enum { RDSP_IO_AUTO = 0, RDSP_IO_RAW = 1, RDSP_IO_WAV = 2 };
typedef struct rdsp_iq_reader rdsp_iq_reader_t;
typedef struct rdsp_audio_writer rdsp_audio_writer_t;
int rdsp_iq_reader_open(const char *path, int format, rdsp_iq_reader_t **out);
double rdsp_iq_reader_sample_rate(const rdsp_iq_reader_t *r); /* 0: the container does not say */
int64_t rdsp_iq_reader_frames(const rdsp_iq_reader_t *r);     /* IQ pairs, -1 unknown */
int rdsp_iq_reader_format(const rdsp_iq_reader_t *r);
size_t rdsp_iq_reader_read(rdsp_iq_reader_t *r, int16_t *dst, size_t n_pairs);
/* Recordings in the engine's other source formats (RDSP_SRC_* below): RAW takes the format it is told (.cu8, .cs8, .cf32);
 * WAV accepts PCM 8-bit stereo as U8, PCM 16-bit as S16 and IEEE float (tag 3, also through the extensible header) 32-bit as
 * F32, sample_format -1 for "what the header says" (any other value must match the header or the open is refused).  frames
 * counts pairs in every format; read_samples delivers elements in the file's own format.  rdsp_iq_reader_open / _read keep
 * their behaviour (int16); _read on a reader that is not S16 returns 0 and sets the error text. */
int rdsp_iq_reader_open_samples(const char *path, int container, int sample_format, rdsp_iq_reader_t **out);
int rdsp_iq_reader_sample_format(const rdsp_iq_reader_t *r);
size_t rdsp_iq_reader_read_samples(rdsp_iq_reader_t *r, void *dst, size_t n_pairs);
void rdsp_iq_reader_close(rdsp_iq_reader_t *r);
int rdsp_audio_writer_open(const char *path, int format, double sample_rate, rdsp_audio_writer_t **out);
size_t rdsp_audio_writer_write(rdsp_audio_writer_t *w, const int16_t *lr, size_t n_pairs);
int64_t rdsp_audio_writer_frames(const rdsp_audio_writer_t *w);
int rdsp_audio_writer_close(rdsp_audio_writer_t *w); /* patches the WAV sizes */

/* Streaming runner: what loop() does with the record/play queues (INO:195-198,
 * CONV:231-244,344-349), for host data.  source fills int16 IQ rows
 * dst[ch * stride_pairs * 2 ...] with n_blocks * 128 pairs per channel and returns
 * the blocks delivered (fewer = end of stream; a trailing partial granule is not
 * processed, as the sketch never processes one); sink receives the int16 L,R rows.
 * Uploads, kernels and downloads of consecutive batches overlap (three streams,
 * two pinned slots).  blocks_per_call must be a multiple of the chain's call unit (of
 * rdsp_chain_granule_blocks() for audio that does not depend on the batch size in every decimator form);
 * max_blocks <= 0 means "until the source ends". */
typedef int (*rdsp_source_fn)(void *user, int16_t *dst, size_t stride_pairs, int n_blocks);
typedef int (*rdsp_sink_fn)(void *user, const int16_t *src, size_t stride_pairs, int n_pairs);
typedef struct {
  int64_t blocks;      /* 128-sample input blocks processed per channel */
  int64_t samples_in;  /* per channel */
  int64_t samples_out; /* per channel */
  double seconds;      /* wall time of the run, set-up included */
  double read_seconds; /* host time inside source() */
  double write_seconds;/* host time inside sink()   */
} rdsp_stream_stats_t;
int rdsp_stream_run(rdsp_chain_t *c, rdsp_source_fn source, void *source_user, rdsp_sink_fn sink,
                    void *sink_user, int blocks_per_call, int64_t max_blocks, rdsp_stream_stats_t *stats);
/* one reader and one writer per channel; the shortest recording ends the run */
int rdsp_stream_run_files(rdsp_chain_t *c, rdsp_iq_reader_t *const *readers,
                          rdsp_audio_writer_t *const *writers, int blocks_per_call, int64_t max_blocks,
                          rdsp_stream_stats_t *stats);
/* host arrays int16 [n_channels][stride_pairs][2] at both ends */
int rdsp_stream_run_memory(rdsp_chain_t *c, const int16_t *host_iq, size_t in_stride_pairs, int64_t n_blocks,
                           int16_t *host_out, size_t out_stride_pairs, int blocks_per_call,
                           rdsp_stream_stats_t *stats);

/* ---- block graph: the AudioStream node/connection API --------------
 * A block is a tile int16 [n_channels][128]; n_channels = 1 is the reference's
 * audio_block_t (FFTIQ.cpp:44,67).  Host-side plumbing in plain C. */
typedef struct rdsp_graph rdsp_graph_t;
typedef struct rdsp_node rdsp_node_t;   /* AudioStream, FFTIQ.h:52-57 */
typedef struct rdsp_block rdsp_block_t; /* audio_block_t */
typedef void (*rdsp_update_fn)(rdsp_node_t *self, void *user); /* virtual void update(void), FFTIQ.h:98 */

rdsp_graph_t *rdsp_graph_create(int n_channels);
void rdsp_graph_destroy(rdsp_graph_t *g);
int rdsp_graph_channels(const rdsp_graph_t *g);
int rdsp_memory(rdsp_graph_t *g, int n_blocks);          /* AudioMemory(40), INO:151 */
int rdsp_memory_usage(const rdsp_graph_t *g);            /* AudioMemoryUsage() */
int rdsp_memory_usage_max(const rdsp_graph_t *g);
/* AudioStream(ninputs, inputQueueArray), FFTIQ.h:55: nodes update in creation order */
rdsp_node_t *rdsp_node_create(rdsp_graph_t *g, int ninputs, rdsp_update_fn update, void *user);
void rdsp_node_set_destructor(rdsp_node_t *n, void (*fn)(void *));
void *rdsp_node_user(rdsp_node_t *n);
rdsp_graph_t *rdsp_node_graph(rdsp_node_t *n);
/* AudioConnection c(src, srcPort, dst, dstPort), INO:71-89 (fan-out allowed) */
int rdsp_connect(rdsp_node_t *src, int src_port, rdsp_node_t *dst, int dst_port);
int rdsp_update_all(rdsp_graph_t *g);                    /* one audio-ISR tick */
void rdsp_no_interrupts(rdsp_graph_t *g);                /* AudioNoInterrupts(), INO:152, CONV:211 */
void rdsp_interrupts(rdsp_graph_t *g);                   /* AudioInterrupts(), INO:175, CONV:222 */
/* inside update() */
rdsp_block_t *rdsp_allocate(rdsp_node_t *n);
rdsp_block_t *rdsp_receive_readonly(rdsp_node_t *n, int port); /* FFTIQ.cpp:70-71 */
rdsp_block_t *rdsp_receive_writable(rdsp_node_t *n, int port);
void rdsp_transmit(rdsp_node_t *n, rdsp_block_t *b, int port);
void rdsp_release(rdsp_block_t *b);                            /* FFTIQ.cpp:114-115 */
int16_t *rdsp_block_data(rdsp_block_t *b);
int rdsp_block_refcount(const rdsp_block_t *b);
/* AudioRecordQueue, CONV:205-206,231-244 */
rdsp_node_t *rdsp_record_queue_create(rdsp_graph_t *g);
void rdsp_record_queue_begin(rdsp_node_t *q);
void rdsp_record_queue_end(rdsp_node_t *q);
int rdsp_record_queue_available(const rdsp_node_t *q);
int16_t *rdsp_record_queue_readBuffer(rdsp_node_t *q);
void rdsp_record_queue_freeBuffer(rdsp_node_t *q);
/* AudioPlayQueue, CONV:344-349 */
rdsp_node_t *rdsp_play_queue_create(rdsp_graph_t *g);
int16_t *rdsp_play_queue_getBuffer(rdsp_node_t *q);
int rdsp_play_queue_playBuffer(rdsp_node_t *q);
/* AudioInputI2S role (INO:52): port 0 = I tile, port 1 = Q tile of this tick */
rdsp_node_t *rdsp_input_node_create(rdsp_graph_t *g);
int rdsp_input_node_push(rdsp_node_t *n, const int16_t *i_tile, const int16_t *q_tile);
/* AudioSDR engine node (INO:53-54,81-86): inputs I,Q; outputs L,R; runs `chain` */
rdsp_node_t *rdsp_sdr_node_create(rdsp_graph_t *g, rdsp_chain_t *chain);
int rdsp_sdr_node_status(rdsp_node_t *n);
int rdsp_chain_decim(const rdsp_chain_t *c);
int rdsp_chain_device(const rdsp_chain_t *c);   /* the device index given to rdsp_chain_create */

/* ---- F1: IQ panadapter spectrum analyser (AudioAnalyzeFFT256IQ, FFTIQ.h:52-110) ----
 * Integer q15 path batched over channels; bit-exact against the oracle.
 *
 * Tables.  Teensy Audio's windows.c / sqrt_integer.c and CMSIS-DSP are not in the reference tree, but
 * the tables the sketch links are in its shipped firmware image (pre_compiled/RadioDSP_SDR_RX.ino.hex)
 * and the generators below reproduce them entry for entry: AudioWindowHanning256 (INO:144),
 * AudioWindowHanning1024 (INO:147), AudioWindowBlackmanNuttall256 (the constructor's default,
 * FFTIQ.h:56) = min(32767, round(32768 w(i / (N - 1)))); twiddleCoef_4096_q15; the 33-entry guess
 * table of sqrt_uint32_approx (tests/test_firmware_tables.py, tests/golden/firmware_tables.npz).
 * The other window ids follow the same rule from the textbook definitions of the names in
 * FFTIQ.h:30-50; the image does not hold them (not pinned).  A caller with its own table uses the
 * reference's signature, rdsp_spectrum_windowFunction_table. */
enum {
  RDSP_WINDOW_NONE = 0,             /* windowFunction(NULL): FFTIQ.cpp:81 skips the multiply */
  RDSP_WINDOW_HANNING = 1,          /* AudioWindowHanning256 / 1024 */
  RDSP_WINDOW_BLACKMAN_HARRIS = 2,
  RDSP_WINDOW_BLACKMAN_NUTTALL = 3, /* AudioWindowBlackmanNuttall256 */
  RDSP_WINDOW_BARTLETT = 4,
  RDSP_WINDOW_BLACKMAN = 5,
  RDSP_WINDOW_FLATTOP = 6,
  RDSP_WINDOW_NUTTALL = 7,
  RDSP_WINDOW_WELCH = 8,
  RDSP_WINDOW_HAMMING = 9,
  RDSP_WINDOW_COSINE = 10,
  RDSP_WINDOW_TUKEY = 11
};
typedef struct rdsp_spectrum rdsp_spectrum_t;
void rdsp_window_q15(int window_id, int16_t *w256);
void rdsp_window_q15_n(int window_id, int n, int16_t *w);
uint32_t rdsp_sqrt_uint32_approx(uint32_t in); /* FFTIQ.cpp:105 (Teensy utility/sqrt_integer.h), host twin of the device routine */
int rdsp_spectrum_create(int n_channels, int device, int naverage, int window_id, rdsp_spectrum_t **out);
int rdsp_spectrum_create_default(int n_channels, int device, rdsp_spectrum_t **out); /* FFTIQ.h:55-58: BlackmanNuttall256, naverage 8 */
void rdsp_spectrum_destroy(rdsp_spectrum_t *s);
int rdsp_spectrum_device(const rdsp_spectrum_t *s);
int rdsp_spectrum_averageTogether(rdsp_spectrum_t *s, int n);      /* FFTIQ.h:88 */
int rdsp_spectrum_windowFunction(rdsp_spectrum_t *s, int window_id); /* FFTIQ.h:93 by table name */
/* void windowFunction(const int16_t *w), FFTIQ.h:93-95, as the reference declares it: a host pointer
 * to 256 q15 taps (copied), NULL = no window */
int rdsp_spectrum_windowFunction_table(rdsp_spectrum_t *s, const int16_t *w256);
int rdsp_spectrum_outputs_for(const rdsp_spectrum_t *s, int n_blocks);
/* float read(unsigned int binNumber), FFTIQ.h:70-73, on one output row (uint16 [256]) */
float rdsp_spectrum_read(const uint16_t *output256, unsigned int binNumber);
/* float read(unsigned int binFirst, unsigned int binLast), FFTIQ.h:75-86, loop as written (`do ... while
 * (binFirst < binLast)`: bins binFirst .. binLast - 1; the single bin when the two are equal) */
float rdsp_spectrum_read_range(const uint16_t *output256, unsigned int binFirst, unsigned int binLast);
/* n_blocks update() ticks (FFTIQ.cpp:65); d_out uint16 [n_channels][out_stride][256] */
int rdsp_spectrum_update(rdsp_spectrum_t *s, const int16_t *d_iq, size_t in_stride, int n_blocks,
                         uint16_t *d_out, size_t out_stride, int *n_outputs, void *stream);

/* the analyser as a node of the block graph (`AudioAnalyzeFFT256IQ FFT;` wired to the
 * pre-processor's I and Q outputs, INO:57,73-74): 2 inputs, no outputs */
rdsp_node_t *rdsp_spectrum_node_create(rdsp_graph_t *g, rdsp_spectrum_t *spec);
int rdsp_spectrum_node_available(rdsp_node_t *n);            /* FFTIQ.h:62-68 */
const uint16_t *rdsp_spectrum_node_output(rdsp_node_t *n);   /* FFTIQ.h:99, [n_channels][256] */
float rdsp_spectrum_node_read(rdsp_node_t *n, int ch, unsigned int binNumber);                          /* FFTIQ.h:70 */
float rdsp_spectrum_node_read_range(rdsp_node_t *n, int ch, unsigned int binFirst, unsigned int binLast); /* FFTIQ.h:75 */
int rdsp_spectrum_node_status(rdsp_node_t *n);

/* ---- band survey: averaged power spectra of shared IQ sources, station finder ---------------------------------------------
 * rdsp_engine_tune wants every receiver's station in Hz from its source's centre; rdsp_survey_t finds them.  An object of its
 * own (several engines, or a chain, may share one band and one survey) that takes the rows of
 * rdsp_engine_update_source_samples -- the four formats RDSP_SRC_* (declared with the engine below), the same value per
 * element, the same stride in pairs -- and returns Welch-averaged power spectra per source as float rows on the device.
 *
 * Definition.  N = fft_n (1024 or 4096), H = N / 2, navg a power of two 1 ... 256, fs = 44100 P / Q.  v[n] = (value of I_n,
 * value of Q_n) for pair n of a source, counted from the last reset (the table of values of the engine's source formats).
 * - Window: w[n] = 0.35875 - 0.48829 cos(2 pi n / N) + 0.14128 cos(4 pi n / N) - 0.01168 cos(6 pi n / N) (the periodic 4-term
 *   Blackman-Harris window), evaluated in double, divided by its double sum and rounded to float: a complex exponential of A
 *   counts on a bin centre reads A^2.  rdsp_survey_window returns these floats; the kernel uses exactly them.
 * - Frame f covers pairs [f H, f H + N): x_f[n] = (w[n] v_I, w[n] v_Q), one rounded float product each; X_f the forward
 *   N-point DFT in float; p_f[k] = |X_f[k]|^2.  No leading zeros: frame 0 is the first N pairs.  A frame's arithmetic is a
 *   function of its N values only.
 * - Row r covers frames r navg ... r navg + navg - 1: acc = 0, acc += p_f[k] in ascending f (float adds), out = acc / navg
 *   (exact).  Output index j = (k + N / 2) mod N lies (j - N / 2) fs / N Hz from the band centre (rdsp_survey_bin_hz);
 *   positive frequency is I + jQ, the sign of rdsp_engine_tune.
 * - Delivery: row r is delivered by the call in which pair (r navg + navg - 1) H + N - 1 arrives.  With T pairs before a
 *   call it completes rows(T + pairs) - rows(T) rows per source, rows(T) = T < N ? 0 : ((T - N) / H + 1) / navg
 *   (rdsp_survey_rows_between; rdsp_survey_rows_for for the object's T).  A stream gives the SAME BITS however it is cut into
 *   calls, calls of 0 pairs and calls that complete no frame included.
 *
 * Rules: source rows aligned to one pair (2 / 2 / 4 / 8 bytes for U8 / S8 / S16 / F32), src_stride >= pairs (a host may walk
 * a pointer through a recording); d_rows 16-byte aligned, rows_stride a multiple of 4 and at least rows_for(pairs) fft_n;
 * pairs <= max_pairs_per_call; 1 ... 4096 sources.  A bad fft_n, navg, format, stride, alignment or size is refused
 * (RDSP_ERR_INVALID, rdsp_last_error) with nothing changed in the object.  Everything is launched on the caller's stream;
 * update does not synchronise.
 *
 * rdsp_survey_find_stations (host, double): db[j] = 10 log10(max(row[j], 1e-30)); the floor is the median of db (the mean of
 * the two middle values); candidates are 1 <= j <= N - 2 with db[j] >= floor + min_db_over_floor, row[j] >= row[j - 1] and
 * row[j] > row[j + 1]; a candidate's frequency is its bin's plus the vertex of the parabola through db[j - 1 ... j + 1];
 * candidates are taken in descending power (equal powers: ascending j), one closer than min_spacing_hz to one already taken
 * is dropped, at most max_out are written (power may be NULL).  Returns the number written, or RDSP_ERR_INVALID. */
typedef struct rdsp_survey rdsp_survey_t;
int rdsp_survey_create(int n_sources, int device, int fft_n, int navg, int format /* RDSP_SRC_* */, size_t max_pairs_per_call,
                       rdsp_survey_t **out);
void rdsp_survey_destroy(rdsp_survey_t *s);
int rdsp_survey_reset(rdsp_survey_t *s, void *stream);          /* T = 0, histories and partial rows zero */
int rdsp_survey_rows_for(const rdsp_survey_t *s, size_t pairs); /* rows per source the NEXT update(pairs) completes */
/* d_src [source][src_stride] pairs; d_rows float [source][row][fft_n], rows_stride floats between sources */
int rdsp_survey_update(rdsp_survey_t *s, const void *d_src, size_t src_stride /* pairs */, size_t pairs, float *d_rows,
                       size_t rows_stride, int *rows_out, void *stream);
int rdsp_survey_sources(const rdsp_survey_t *s);
int rdsp_survey_fft_n(const rdsp_survey_t *s);
int rdsp_survey_navg(const rdsp_survey_t *s);
int rdsp_survey_format(const rdsp_survey_t *s);
int rdsp_survey_device(const rdsp_survey_t *s);
/* host only, no device */
int rdsp_survey_window(int fft_n, float *out /* [fft_n] */);
int rdsp_survey_rows_between(int fft_n, int navg, uint64_t pairs_before, size_t pairs);
double rdsp_survey_bin_hz(int fft_n, int P, int Q, int j);
int rdsp_survey_find_stations(const float *row, int fft_n, int P, int Q, double min_db_over_floor, double min_spacing_hz,
                              int max_out, double *station_hz, float *power);

/* ---- F3: biquad cascades ----------------------------------------------------------------------------------------
 * Two different routines of two different libraries, neither in the reference tree, both restated from their published
 * sources and both confirmed in structure by the code of the reference's firmware image (tests/test_firmware_tables.py):
 *
 * (1) the engine's IIR audio filter bank (CTL:153-177 / SURVEY Appendix C): CMSIS-DSP's arm_biquad_cascade_df1_f32 --
 *     direct form 1 in float, acc = (b0 Xn) + (b1 Xn1) + (b2 Xn2) + (a1 Yn1) + (a2 Yn2), every product rounded
 *     before it is added, feedback coefficients stored negated.  In the chain: rdsp_sdr_setAudioFilterKind below.
 *     Design helpers (host): */
void rdsp_biquad_design(int kind, double freq, double q, double fs, float *coef5); /* 0 LP, 1 HP, 2 BP, 3 notch */
void rdsp_design_audio_iir(double f1, double f2, double fs, float *coef20);        /* 8th-order Butterworth band-pass */
/* (2) `AudioFilterBiquad biquad1, biquad2;` (INO:58-59,75-78; `setHighpass(0, 500, 0.5)` INO:155-156): the Teensy Audio
 *     library's FIXED-POINT cascade -- coefficients int32 x 2^30 (a1, a2 stored negated), five 32 x 16 products per
 *     sample that keep the top 32 of 48 bits (SMLAWB / SMLAWT), accumulated on the 14 fractional bits the previous
 *     sample left (`sum &= 0x3FFF`), output `signed_saturate_rshift(sum, 16, 14)`; a fresh object passes nothing
 *     (all-zero coefficients); update() runs stage 0 and goes on to stage s + 1 only if setCoefficients(s + 1) was
 *     ever called; a setter clears its stage's residue and keeps its sample history.  int16 in, int16 out, bit-exact
 *     against the test restatement.  fs: AUDIO_SAMPLE_RATE_EXACT (44100.0 in the reference's image). */
typedef struct rdsp_biquad rdsp_biquad_t; /* AudioFilterBiquad for n_channels streams */
int rdsp_biquad_create(int n_channels, int device, double fs, rdsp_biquad_t **out);
void rdsp_biquad_destroy(rdsp_biquad_t *b);
/* setCoefficients(stage, const double *{b0, b1, b2, a1, a2}) with H = (b0 + b1/z + b2/z^2) / (1 + a1/z + a2/z^2): each
 * coefficient x 1073741824.0 converted to int; setCoefficients(stage, const int *) takes them already scaled */
int rdsp_biquad_setCoefficients(rdsp_biquad_t *b, int stage, const double *coefficients);
int rdsp_biquad_setCoefficients_int(rdsp_biquad_t *b, int stage, const int32_t *coefficients);
int rdsp_biquad_setLowpass(rdsp_biquad_t *b, int stage, float frequency, float q);
int rdsp_biquad_setHighpass(rdsp_biquad_t *b, int stage, float frequency, float q);  /* INO:155-156 */
int rdsp_biquad_setBandpass(rdsp_biquad_t *b, int stage, float frequency, float q);
int rdsp_biquad_setNotch(rdsp_biquad_t *b, int stage, float frequency, float q);
/* what the four setters compute (host, no device): RBJ cookbook in double with w0 = frequency * (2 * 3.141592654 / fs),
 * each coefficient x 2^30 / (1 + alpha) converted to int; a1, a2 as the transfer function writes
 * them (setCoefficients negates).  kind 0 LP, 1 HP, 2 BP, 3 notch */
void rdsp_teensy_biquad_design(int kind, float frequency, float q, float fs, int32_t *coef5);
int rdsp_biquad_get_definition(const rdsp_biquad_t *b, int32_t *out20, int *n_stages); /* b0, b1, b2, -a1, -a2 x 2^30 per stage */
int rdsp_biquad_get_coeffs(const rdsp_biquad_t *b, float *out20);                    /* the same / 2^30 */
/* n_blocks update() ticks: int16 [n_channels][stride] samples read / written every `step` int16
 * (1: planar mono blocks; 2: one side of interleaved pairs, e.g. the I or the Q of an IQ stream) */
int rdsp_biquad_update(rdsp_biquad_t *b, const int16_t *d_in, size_t in_stride, int in_step, int n_blocks,
                       int16_t *d_out, size_t out_stride, int out_step, void *stream);
rdsp_node_t *rdsp_biquad_node_create(rdsp_graph_t *g, rdsp_biquad_t *b); /* 1 input, 1 output */
int rdsp_biquad_node_status(rdsp_node_t *n);
/* Implementation of the engine's audio filter (SDR.enableAudioFilter / setAudioFilter):
 * RDSP_AUDIO_KIND_MASK (default): the pass band is the overlap-save mask (CONV:209-224).
 * RDSP_AUDIO_KIND_IIR: the mask keeps only the side-band selection (50 Hz ... 4 kHz on the
 * demodulator's side) and the selected audio filter is an 8th-order band-pass of four biquads on
 * the demodulated audio, between the overlap-save filter and the NR / notch / AGC stages. */
enum { RDSP_AUDIO_KIND_MASK = 0, RDSP_AUDIO_KIND_IIR = 1 };
int rdsp_sdr_setAudioFilterKind(rdsp_chain_t *c, int kind, void *stream);
int rdsp_chain_get_iir_coeffs(rdsp_chain_t *c, int group, float *out20);
/* An explicit cascade instead of the designed one: coef20 = four sections {b0, b1, b2, a1, a2} in
 * arm_biquad_cascade_df1_f32 order (feedback terms added), e.g. one of the fifteen sets of the engine's own audio
 * filters that the reference's firmware image holds (tests/golden/firmware_tables.npz `biquad_sets`; the first eight
 * are 150 Hz ... 2.1 / 2.3 / 2.5 / 2.7 / 2.9 / 3.1 / 3.3 / 3.9 kHz band-passes for fs = 44 117.647 Hz, each a 4th-order
 * elliptic-type high-pass and low-pass pair: zeros on the unit circle at 21 / 50 Hz and at 2.8 fu / 5.4 fu).  Needs
 * RDSP_AUDIO_KIND_IIR; in force until the next setAudioFilter / setDemodMode of the group -- or until
 * rdsp_chain_set_groups, which re-designs every group's filter from its settings: load explicit sets after regrouping. */
int rdsp_group_setAudioIIRCoefficients(rdsp_chain_t *c, int group, const float *coef20);
int rdsp_sdr_setAudioIIRCoefficients(rdsp_chain_t *c, const float *coef20);

/* ---- AudioAnalyzeFFT1024 (Teensy Audio library; `AudioAnalyzeFFT1024 AudioFFT` on Q_out_L,
 * INO:57,87): 1024-point frames of the audio stream with hop 512 (blocks collected eight at a time,
 * four kept), q15 window, arm_cfft_radix4_q15 of the real samples, output[i] = sqrt_uint32_approx(|X_i|^2)
 * for the 512 bins from DC up (integer, bit-exact against the test restatement; FFT, window, twiddles
 * and square root as for F1).  window_id: RDSP_WINDOW_*. */
typedef struct rdsp_fft1024 rdsp_fft1024_t;
int rdsp_fft1024_create(int n_channels, int device, int window_id, rdsp_fft1024_t **out);
void rdsp_fft1024_destroy(rdsp_fft1024_t *s);
int rdsp_fft1024_windowFunction(rdsp_fft1024_t *s, int window_id); /* INO:147 by table name */
int rdsp_fft1024_windowFunction_table(rdsp_fft1024_t *s, const int16_t *w1024); /* windowFunction(const int16_t *), NULL = none */
float rdsp_fft1024_read(const uint16_t *output512, unsigned int binNumber);   /* AudioAnalyzeFFT1024::read(bin) */
float rdsp_fft1024_read_range(const uint16_t *output512, unsigned int binFirst, unsigned int binLast); /* ::read(first, last), inclusive */
int rdsp_fft1024_averageTogether(rdsp_fft1024_t *s, int n);       /* INO:148: a no-op in the library too */
int rdsp_fft1024_outputs_for(const rdsp_fft1024_t *s, int n_blocks);
/* n_blocks update() ticks; d_audio int16 [n_channels][in_stride] samples taken every in_step int16
 * (2 with an offset pointer picks L or R of the chain's interleaved output); d_out uint16
 * [n_channels][out_stride][512] receives the spectra completed in this call */
int rdsp_fft1024_update(rdsp_fft1024_t *s, const int16_t *d_audio, size_t in_stride, int in_step, int n_blocks,
                        uint16_t *d_out, size_t out_stride, int *n_outputs, void *stream);
rdsp_node_t *rdsp_fft1024_node_create(rdsp_graph_t *g, rdsp_fft1024_t *s); /* 1 input, no outputs */
int rdsp_fft1024_node_available(rdsp_node_t *n);
const uint16_t *rdsp_fft1024_node_output(rdsp_node_t *n); /* [n_channels][512] */
float rdsp_fft1024_node_read(rdsp_node_t *n, int ch, unsigned int binNumber);
float rdsp_fft1024_node_read_range(rdsp_node_t *n, int ch, unsigned int binFirst, unsigned int binLast);
int rdsp_fft1024_node_status(rdsp_node_t *n);

/* ---- deterministic synthetic IQ generator (host) -------------------*/
typedef struct {
  double fs;        /* 96000 */
  double f_off;     /* IF offset, 12000 */
  int32_t cw;       /* 0: two USB tones + interferer; 1: keyed CW tone (K4) */
  double amp_tone;  /* 0.20 */
  double amp_carrier; /* 0.30 */
  double sigma;     /* 0.05 per rail */
} rdsp_synth_config_t;
/* dst: int16 [n_ch][n_samples][2]; channels ch0..ch0+n_ch-1, samples t0..t0+n_samples-1 */
void rdsp_synth_iq(int16_t *dst, int ch0, int n_ch, uint64_t t0, int n_samples,
                   const rdsp_synth_config_t *cfg, int n_threads);

/* ---- `AudioSDR SDR;` as the reference's engine computes it (INO:54; wired INO:81-86) ------------------------------
 * The engine (Derek Rowell's AudioSDR library) is not in the reference tree; its compiled code is, in
 * pre_compiled/RadioDSP_SDR_RX.ino.hex.  rdsp_engine_t follows that code (AudioSDR::update, ITCM 0xe730, and the setters
 * the sketch calls) for n_channels receivers: on the same int16 IQ blocks it returns the int16 audio the image's update()
 * returns (tests/test_engine_kat.py; csrc/rdsp_engine.hip describes the signal path and names the three stage files of the kernels; the host object is csrc/rdsp_engine_host.h and the five host files it names).  Native rate only:
 * 44.1 kHz, one 128-sample block in, one out, no decimation.  The rdsp_sdr_* setters above belong to rdsp_chain_t, this
 * build's own many-channel receiver with a decimator in front; these are the reference's.  Numbers are the engine's
 * (`mode`: 0 LSBmode, 1 USBmode, 2 CW_LSBmode, 3 CW_USBmode, 4 AMmode, 5 SAMmode, as the compiled tuningMode() passes
 * them, CTL:337-407; audio filter ids as the compiled filterMode() passes them: 0 audioAM, 1 audioCW, 3 audio2100,
 * 6 audio2700, 8 audio3100, 10 = none, CTL:153-177; AGC modes 0 off ... 3 slow, CTL:200-218). */
typedef struct rdsp_engine rdsp_engine_t;
int rdsp_engine_create(int n_channels, int device, int max_blocks_per_call, rdsp_engine_t **out); /* AudioSDR::AudioSDR */
void rdsp_engine_destroy(rdsp_engine_t *e);
int rdsp_engine_reset(rdsp_engine_t *e, void *stream); /* signal state as the constructor leaves it; settings kept */
/* The engine's tables without a closed form, in the image's order: fifteen sets of four {b0, b1, b2, a1, a2} sections
 * (arm_biquad_cascade_df1_f32 layout) and the 64 taps of one side of its Hilbert transformer, outermost first.
 * rdsp_engine_update fails with RDSP_ERR_NOT_READY until they are loaded. */
int rdsp_engine_load_tables(rdsp_engine_t *e, const float *biquad_sets15x20, const float *hilbert64);
int rdsp_engine_enableAGC(rdsp_engine_t *e);                       /* INO:120 */
int rdsp_engine_setAGCmode(rdsp_engine_t *e, int mode);            /* INO:121, CTL:200-218 */
int rdsp_engine_enableALSfilter(rdsp_engine_t *e);                 /* CTL:259 (clears the filter) */
int rdsp_engine_disableALSfilter(rdsp_engine_t *e);                /* INO:125 */
int rdsp_engine_setALSfilterNotch(rdsp_engine_t *e);               /* CTL:260 */
int rdsp_engine_setALSfilterPeak(rdsp_engine_t *e);                /* backup/RadioDSP_SDR_RX_Conv.ino:665 */
int rdsp_engine_setALSfilterAdaptive(rdsp_engine_t *e);            /* CTL:261 */
int rdsp_engine_enableNoiseBlanker(rdsp_engine_t *e);              /* backup/RadioDSP_SDR_RX_Conv.ino:1259; the constructor's default */
int rdsp_engine_disableNoiseBlanker(rdsp_engine_t *e);             /* INO:131 */
int rdsp_engine_setInputGain(rdsp_engine_t *e, float g);           /* INO:133 */
int rdsp_engine_setOutputGain(rdsp_engine_t *e, float g);          /* INO:134 */
int rdsp_engine_setIQgainBalance(rdsp_engine_t *e, float b);       /* INO:135 */
int rdsp_engine_enableAudioFilter(rdsp_engine_t *e);               /* INO:137 */
int rdsp_engine_setAudioFilter(rdsp_engine_t *e, int id);          /* INO:138, CTL:153-177 */
float rdsp_engine_setDemodMode(rdsp_engine_t *e, int mode);        /* INO:139: returns TuningOffset, Hz */
int rdsp_engine_setMute(rdsp_engine_t *e, int on);                 /* INO:177 */
/* AudioSDR::update() for n_blocks consecutive blocks of every channel, stream-ordered.  d_iq: [ch][t] int16 pairs (I, Q),
 * in_stride pairs between channel rows; d_lr: [ch][t] int16 pairs = the engine's two outputs (the same block on both).
 * Each row must already hold its station at the engine's IF; this call does not advance the tuning phases below. */
int rdsp_engine_update(rdsp_engine_t *e, const int16_t *d_iq, size_t in_stride, int n_blocks, int16_t *d_lr,
                       size_t out_stride, void *stream);
/* Shared IQ streams: many receivers tuned to stations inside a few source rows -- the sketch's VFO, which puts its LO at
 * vfoFreq - TuningOffset (RDSP_controls.h:447), done per receiver on the GPU.
 * - Sources: d_src is int16 pairs [n_sources][src_stride] at 44 100 Hz; receiver ch listens to row source_of_channel[ch]
 *   (several receivers may share a row).  rdsp_engine_set_sources sets the map; the first call allocates the engine's
 *   tuned rows ([ch][max_blocks_per_call * 128] pairs) and per-channel phases (an engine that never calls it uses no more
 *   memory than before).  It takes no stream: it waits for everything queued on the engine's device before it changes a map.
 * - Station: station_hz[k] is where receiver first_channel + k's station sits in its source, from the stream's centre,
 *   |f| < 22 050 (0 until tuned).  Positive frequency is I + jQ, the engine's own convention.  Stations are settings: kept
 *   by rdsp_engine_reset, not part of a state blob.
 * - Tuned row: x_ch[n] = sat16(rne(x_src[n] e^{+j phi_ch[n]})), phi_ch a uint32 phase accumulator (turns x 2^32) that is 0
 *   at create and after rdsp_engine_reset, stays continuous across calls, retunes, mode changes and regroupings, and
 *   advances per sample by dphi = round((TuningOffset of ch's group's mode - station_hz) 2^32 / 44100), computed from the
 *   group's mode at every call (a receiver stays on its station when its mode changes, as the sketch re-tunes its LO;
 *   round is half away from zero, taken mod 2^32).  The phasor comes from a 1024-entry table of cos / sin with linear
 *   interpolation (error below 2^-17; phase 0 is exactly (1, 0), so a shift of 0 is the identity); the rotation is the
 *   engine shifter's, I' = fmaf(I, c, -(Q s)), Q' = fmaf(Q, c, I s); rounding half to even, saturation to int16.
 *   rdsp_engine_tune_table gives the table: [1024][4] = cos, sin of 2 pi k / 1024, and the steps to entry k + 1.
 * - rdsp_engine_update_sources = the tuning pass, then rdsp_engine_update on the tuned rows, every group: the audio is
 *   bit for bit what rdsp_engine_update returns on those rows.  Source rows must be 16-byte aligned, a multiple of 4 pairs
 *   apart (src_stride) and at least n_blocks * 128 pairs long.
 * - Refused with nothing changed (RDSP_ERR_INVALID): a source index outside [0, n_sources), n_sources < 1, |station| >=
 *   22 050 (or NaN), a channel range outside the object, a short or misaligned src_stride or d_src, n_blocks > max_blocks;
 *   rdsp_engine_update_sources before rdsp_engine_set_sources is RDSP_ERR_NOT_READY.
 * - State as data: once an engine has sources, its blobs carry each channel's phase (a flag in the header word that was 0,
 *   one word per channel appended; rdsp_engine_state_bytes says so), and a moved receiver continues bit for bit.  The blob
 *   of an engine without sources is unchanged.  Loading a blob with phases needs sources (RDSP_ERR_NOT_READY); loading one
 *   without phases into an engine with sources sets those channels' phases to 0. */
int rdsp_engine_set_sources(rdsp_engine_t *e, int n_sources, const int *source_of_channel);
int rdsp_engine_tune(rdsp_engine_t *e, int first_channel, int n_channels, const double *station_hz);
int rdsp_engine_update_sources(rdsp_engine_t *e, const int16_t *d_src, size_t src_stride, int n_blocks, int16_t *d_lr,
                               size_t out_stride, void *stream);
const float *rdsp_engine_tune_table(void);
/* Wide-band sources: rows at D x 44 100 Hz, D an integer 1 ... 64 (up to 2.8224 MHz), one D per engine.  The pass becomes a
 * digital down-converter: shift the station to the engine's IF, low-pass, decimate by D to 44 100 Hz.
 * - rdsp_engine_set_source_decimation(e, D, gain), after rdsp_engine_set_sources (RDSP_ERR_NOT_READY before).  It takes no
 *   stream and waits for everything queued on the engine's device.  D = 1 (the state at create) is the tuning pass above,
 *   no filter, gain unused.  For D > 1 output sample m of receiver ch, x its source row with the pairs of earlier calls
 *   before it:
 *     y[m] = sat16(rne(e^{+j phi_m} sum_{k < T} g_k x[(m + 1) D - 1 - k])),  g_k = h_k e^{-j 2 pi k dphi / 2^32},  T = 16 D,
 *     phi_{m + 1} = phi_m + D dphi,  dphi = round((TuningOffset - station_hz) 2^32 / (D 44100)), half away from zero:
 *   the prototype low-pass h translated onto the station, then the rotation to the IF; the window of output m ends at the
 *   newest of its D source samples, so the filter delays by (T - 1) / 2 source samples.  The phasors are the table's, the
 *   rotation, rounding and saturation the tuning pass's; the sum is one chain of fmaf over k ascending (csrc/rdsp_tune.h).
 * - h (a design of this build, not the reference's): a sinc with its cutoff at 22 050 Hz under a Kaiser window, beta = 9,
 *   16 D taps, normalised to sum 1, times gain (> 0, finite), rounded to float.  For every D in 2 ... 64: ripple <= 0.00041 dB
 *   for |f| <= 12 000 Hz, >= 90.2 dB down from 32 100 Hz on (all that folds onto |f| <= 12 000 Hz), sum |h| <= 1.65.  The
 *   gain is folded into h because a station in a wide band sits far below full scale: requantising to int16 at unit gain
 *   would throw away the decimation's processing gain.  rdsp_engine_ddc_taps writes the 16 D taps; it needs no GPU.
 * - Per channel the state stays the one phase, with the rules above (a retune re-centres the filter at once, phase
 *   continuous).  Per SOURCE the engine keeps the last 15 D pairs of each row after every call: zero at create, after
 *   rdsp_engine_reset, and when D or n_sources changes.  It is not part of a channel's blob: a moved receiver continues bit
 *   for bit when both objects heard the same source stream.
 * - With D set: |station_hz| < D x 22 050 in rdsp_engine_tune; source rows of rdsp_engine_update_sources are n_blocks x
 *   128 x D pairs (src_stride at least that); d_lr, out_stride and max_blocks count 44 100 Hz samples as before.
 * - Refused with nothing changed (RDSP_ERR_INVALID): D outside 1 ... 64, gain not above 0 or not finite, a channel already
 *   tuned to |f| >= D x 22 050.
 * - Decimation in several stages is not this pass's business: rdsp_channelizer_t (below) is a first stage shared by all
 *   receivers of a source, and its sub-band rows are sources of this pass at a small D. */
int rdsp_engine_set_source_decimation(rdsp_engine_t *e, int D, float gain);
int rdsp_engine_source_decimation(const rdsp_engine_t *e);
int rdsp_engine_ddc_taps(int D, float gain, float *out /* [16 D] */);
/* Sources at any rational multiple of 44 100 Hz: rows at 44 100 P / Q Hz (48 k = 160 / 147, 96 k = 320 / 147, 192 k = 640 / 147,
 * 2.4 M = 8000 / 147, 250 k = 2500 / 441, 1.024 M = 10240 / 441, 2.048 M = 20480 / 441; Q is 147 or 441 for every integer-Hz rate
 * on the 1 kHz or 2 kHz grid).  The pass becomes a polyphase rational resampler: it tunes, low-passes and changes the rate by
 * Q / P in one pass per receiver (csrc/rdsp_engine_rate.hip, arithmetic in csrc/rdsp_tune.h).
 * - rdsp_engine_set_source_rate(e, P, Q, gain), after rdsp_engine_set_sources (RDSP_ERR_NOT_READY before).  P, Q are divided
 *   by their gcd first; after that 1 <= Q <= 441, Q <= P <= 64 Q, gain finite and above 0.  Q = 1 after reduction IS
 *   rdsp_engine_set_source_decimation(e, P, gain): the same code path, the same bits.  rdsp_engine_set_source_decimation
 *   called later replaces a rational rate.  Dc = ceil(P / Q); a branch of the filter has Tb = 16 Dc taps.
 * - The prototype (rdsp_engine_rate_taps, host only, Tp = Tb Q floats): the low-pass of rdsp_engine_ddc_taps at the rate
 *   44 100 P -- a sinc with its cutoff at 22 050 Hz under a Kaiser window, beta = 9, by the same libm-free series, with
 *   q = |2 i - (Tp - 1)|, u = pi q / (2 P), rho = q / (Tp - 1), summed in tap order, out[i] = (float)((h[i] / sum) (Q gain)).
 *   For Q = 1 it is rdsp_engine_ddc_taps(P, gain) bit for bit.  Branch r is hb[r][j] = out[j Q + r], j = 0 ... Tb - 1: the tap
 *   for a delay of j + r / Q source samples.  Over the rates of tests/test_engine_rate.py: ripple <= 0.001 dB on |f| <=
 *   12 000 Hz, >= 89 dB down from 32 100 Hz to the prototype's Nyquist frequency (the images of the source spectrum
 *   included), sum_j |hb[r][j]| <= 2.5 (a branch of a ratio near 1 spans up to 32 output periods).
 * - Schedule: one integer for all sources, frac = (M P) mod Q, M the outputs since the last reset: zero at create, after
 *   rdsp_engine_reset and when the rate or n_sources changes (the source histories are zeroed on the same occasions).  A call
 *   of n_out = n_blocks x 128 outputs consumes pairs = (frac + n_out P) div Q pairs of every source row, then frac <- (frac +
 *   n_out P) mod Q.  rdsp_engine_source_pairs(e, n_blocks) returns pairs for the NEXT call (it varies by one between calls;
 *   for an integer rate it is n_blocks x 128 x D).  Output i of a call has its newest source pair at local index n(i) =
 *   (frac + (i + 1) P) div Q - 1 and uses branch r(i) = (frac + (i + 1) P) mod Q (64-bit products).
 * - Arithmetic, x the source row with the pairs of earlier calls before it:
 *     dphi = llround((TuningOffset - station) 2^32 / ((P 44100.0) / Q))  (uint32)
 *     e_j  = table phasor at 0 - j dphi;  u_j = (hb[r(i)][j] xI[n(i) - j], hb[r(i)][j] xQ[n(i) - j]), two rounded products;
 *     one chain over j ascending from re = im = 0, four fmaf a tap: re += e.x u.x; re += -e.y u.y; im += e.x u.y; im += e.y u.x;
 *     y[i] = the tuning pass's rotation, rounding and saturation at the phase ph0 + (n(i) + 1 - Dc) dphi;
 *     the phase after the call is ph0 + pairs dphi.
 *   The order has no tile, register block or call size in it, so neither has the result; tests/test_engine_rate.py restates
 *   it in numpy bit for bit, and the audio is bit for bit rdsp_engine_update on the tuned rows.
 * - State: per channel the one phase, with all its rules (continuous through calls, retunes, mode changes and regroupings,
 *   zeroed by reset, in the blob behind the header flag).  Per SOURCE the last Tb pairs; they are in no blob and blob sizes
 *   are unchanged: a moved receiver continues bit for bit when both engines heard the same source stream since the same
 *   reset.
 * - With a rational rate set: |station_hz| < 22 050 P / Q in rdsp_engine_tune; rdsp_engine_update_sources reads
 *   rdsp_engine_source_pairs(e, n_blocks) pairs per row, src_stride at least that, rows and stride int16-PAIR (4-byte)
 *   aligned only, so a host can walk a pointer through a long recording (the 16-byte rule stays for Q = 1);
 *   rdsp_engine_source_decimation returns 0; rdsp_engine_source_rate gives P, Q (D, 1 for an integer rate).
 * - rdsp_engine_rate_of_hz(fs_hz, &P, &Q): for an integer-Hz rate fs / g, 44100 / g, g their gcd; refused when fs is not an
 *   integer or the ratio is outside the limits above (44 101 Hz: Q = 44 100; 32 000 Hz: P < Q; 3.2 MHz: above 64).
 * - Refused with nothing changed (RDSP_ERR_INVALID): P or Q below 1, Q above 441 or P outside Q ... 64 Q after reduction, gain
 *   not above 0 or not finite, a channel already tuned to |f| >= 22 050 P / Q, a src_stride below rdsp_engine_source_pairs. */
int rdsp_engine_set_source_rate(rdsp_engine_t *e, int P, int Q, float gain);
int rdsp_engine_source_rate(const rdsp_engine_t *e, int *P, int *Q);
size_t rdsp_engine_source_pairs(const rdsp_engine_t *e, int n_blocks);
int rdsp_engine_rate_of_hz(double fs_hz, int *P, int *Q);
int rdsp_engine_rate_taps(int P, int Q, float gain, float *out /* [16 ceil(P / Q) Q], P / Q in lowest terms */);
/* Source sample formats: what the source rows of every rate above hold.  One format per engine.
 *   RDSP_SRC_S16 (default)  int16                          value (float)x
 *   RDSP_SRC_U8             uint8, offset binary (.cu8)    value (float)(2 u - 255) x 128: exact, +-32 640, symmetric about 127.5
 *   RDSP_SRC_S8             int8 (.cs8)                    value (float)s x 256: exact
 *   RDSP_SRC_F32            float, full scale +-1.0 (cf32) NaN -> 0; otherwise clamp(x, -256, 256) x 32768: +-inf and wild values
 *                                                          stay finite at +-2^23 counts; the output saturates as always
 *   Pairs are I then Q, interleaved.  The value, in counts on the int16 scale, enters the arithmetic of the three passes where
 *   the int16 sample does (csrc/rdsp_tune.h, src_value); everything after it is the same, operation for operation.  So an 8-bit
 *   row gives the bits of the int16 pass on the row widened by the table, and a float row of values k / 32768 the bits of the
 *   int16 row k.  The passes read the rows in place in their own format: no widened copy, no conversion pass.
 * - rdsp_engine_set_source_format(e, format), after rdsp_engine_set_sources (RDSP_ERR_NOT_READY before); an unknown format is
 *   RDSP_ERR_INVALID.  A setting: kept by rdsp_engine_reset, rdsp_engine_set_sources and the rate setters, in no state blob (blob
 *   sizes are unchanged).  Setting the format the engine has changes nothing; another one begins another stream: the source
 *   histories and frac go to zero as with a change of rate, the phases stay with their channels.  It takes no stream and
 *   waits for everything queued on the engine's device.  The histories of the three new formats are kept as float2 VALUES
 *   (a fresh history is exactly 0 in every format; no uint8 byte has the value 0), those of S16 as the packed words.
 * - rdsp_engine_update_source_samples is rdsp_engine_update_sources for any format (with S16 the same code path, the same
 *   bits).  src_stride and rdsp_engine_source_pairs count PAIRS whatever the format.  Alignment in bytes: the integer rates
 *   need rows 16-byte aligned and src_stride x bytes-per-pair (4 / 2 / 2 / 8) a multiple of 16; a rational rate needs rows
 *   and stride aligned to one pair.  rdsp_engine_update_sources stays for S16 and is RDSP_ERR_INVALID under another format.
 *   Every refusal changes nothing in the object. */
enum { RDSP_SRC_S16 = 0, RDSP_SRC_U8 = 1, RDSP_SRC_S8 = 2, RDSP_SRC_F32 = 3 };
int rdsp_engine_set_source_format(rdsp_engine_t *e, int format);
int rdsp_engine_source_format(const rdsp_engine_t *e);
int rdsp_engine_update_source_samples(rdsp_engine_t *e, const void *d_src, size_t src_stride /* pairs */, int n_blocks,
                                      int16_t *d_lr, size_t out_stride, void *stream);
/* ---- channelizer: a wide source split once into sub-bands that all its receivers share --------------------------------------
 * The passes above do all of a receiver's down-conversion per receiver: 64 Dc FMAs per output sample, Dc = ceil(P / Q), and
 * the same coarse filtering again for every receiver of a source.  rdsp_channelizer_t does the coarse part once per SOURCE: a
 * polyphase channelizer splits the band into M overlapping sub-bands at D2 x 44 100 Hz, float rows on the device, and every
 * receiver listens to the sub-band nearest its station through the engine's decimating pass at D = D2.  An object of its
 * own, as rdsp_survey_t is (several engines may share one band); the engine does not know it.  A receiver is set up with the
 * calls above: rdsp_channelizer_place(P, Q, M, station) -> subband, residual; rdsp_engine_set_sources(n_sources M, src M +
 * subband); rdsp_engine_set_source_decimation(D2, gain); rdsp_engine_set_source_format(RDSP_SRC_F32);
 * rdsp_engine_tune(residual); rdsp_engine_update_source_samples(d_sub, sub_stride, n_blocks, ...).
 *
 * Rates.  fs = 44100 P / Q; sub-band spacing fs / M, M one of 8, 16, 32, 64; sub-band rate fo = 44100 D2, D2 an integer 2 ... 64;
 * P1 / Q1 = P / (Q D2) in lowest terms (rdsp_channelizer_rate).  Accepted when P / Q passes the rule of
 * rdsp_engine_set_source_rate, P1 >= Q1, Q1 <= 441 and
 *     fs / (2 M) + 12000 <= 12000 D2.
 * The last condition is no tuning knob: a station anywhere in the band lies within half a spacing of a sub-band centre, so the
 * +-12 kHz around it lie within fs / (2 M) + 12000 of that centre -- inside the prototype's flat band |f| <= 12000 D2 -- and all
 * that aliases onto them at the rate fo lies at 44100 D2 - 12000 D2 = 32100 D2 or above, in its stop band.  Everything else is
 * refused (RDSP_ERR_INVALID, nothing changed): 8000 / 147 with M = 32, D2 = 4; 2500 / 441 with M = 8, D2 = 2; 10240 / 441 with D2 =
 * 3 (Q1 = 1323).
 *
 * Prototype (rdsp_channelizer_taps, host only): the taps of rdsp_engine_rate_taps(P1, Q1, 1.0) times 2^-15 (exact), so that
 * sub-band rows are full scale +-1.0, what RDSP_SRC_F32 expects: the same Kaiser-windowed sinc as both passes above, its
 * cutoff at the sub-band rate's Nyquist frequency.  Dc1 = ceil(P1 / Q1), Tb = 16 Dc1, branch r is hb[r][j] = out[j Q1 + r].  Over
 * the configurations of tests/test_channelizer.py (and times 2^15): ripple <= 0.001 dB on |f| <= 12000 D2, >= 89 dB down from
 * 32100 D2 to the prototype's Nyquist frequency, sum_j |hb[r][j]| <= 2.5.
 *
 * Schedule: the polyphase pass's with P1, Q1.  frac starts at 0; a call of n_out = n_blocks x 128 x D2 outputs per sub-band
 * consumes (frac + n_out P1) div Q1 pairs of every source row (rdsp_channelizer_source_pairs for the NEXT call), then frac <-
 * (frac + n_out P1) mod Q1.  Output i has its newest pair at local index n(i) = (frac + (i + 1) P1) div Q1 - 1 and uses branch
 * r(i) = (frac + (i + 1) P1) mod Q1 (64-bit products).  The object also keeps T mod M, T the pairs consumed since the reset.
 *
 * Arithmetic of output i, sub-band k; x the source VALUES (the table of the engine's source formats, counts) with the pairs
 * of earlier calls in front and zeros before the stream; N = T + n(i) the absolute index of the newest pair:
 *     fold:  v[q] = 0 for q = 0 ... M - 1;  for j = 0 ... Tb - 1 ascending, q = (N - j) mod M:
 *                vI[q] = fmaf(hb[r][j], xI[n - j], vI[q]);  vQ[q] = fmaf(hb[r][j], xQ[n - j], vQ[q])
 *     DFT:   re = im = 0;  for q = 0 ... M - 1 ascending, (c, s) = twiddles[(k q) mod M]:
 *                re = fmaf(c, vI[q], re);  re = fmaf(s, vQ[q], re);  im = fmaf(c, vQ[q], im);  im = fmaf(-s, vI[q], im)
 * twiddles[m] = (cos, sin)(2 pi m / M), evaluated in double and rounded to float, exactly 0 and +-1 at quarter turns and
 * symmetric between octants (rdsp_channelizer_twiddles; the kernel uses exactly these values).  This is mixing by
 * e^{-j 2 pi k m / M} at the source's sample times, then low-passing and resampling; positive frequency is I + jQ.  Row
 * src M + k of d_sub is sub-band k of source src; its centre lies ((k + M / 2) mod M - M / 2) fs / M Hz from the band centre.
 * The order has no tile, lane or call size in it: a stream gives the SAME BITS however it is cut into calls, and
 * tests/channelizer_model.py restates it in numpy bit for bit.  (A direct DFT, M^2 complex MACs an instant, for that reason.)
 *
 * State: per source the last Tb pairs as float2 values in every format, frac and T mod M; zero at create and after
 * rdsp_channelizer_reset.  Nothing of it is in any engine blob.
 *
 * Rules: source rows aligned to one pair of their format, src_stride >= source_pairs(n_blocks); d_sub 16-byte aligned, float2
 * [n_sources M][sub_stride], sub_stride (pairs) even and at least n_blocks x 128 x D2 -- the rows then satisfy the engine's
 * rule for RDSP_SRC_F32 rows at an integer rate; n_blocks <= max_blocks_per_call (at most 4096); 1 ... 4096 sources.  Everything
 * is launched on the caller's stream; update does not synchronise.  Every refusal leaves the object unchanged and sets
 * rdsp_last_error.
 *
 * rdsp_channelizer_place (host, double): spacing = fs / M; kk = station / spacing rounded half away from zero; subband =
 * kk mod M, non-negative; residual = station - kk spacing, so |residual| <= spacing / 2.  Refused for |station| >= fs / 2 or NaN. */
typedef struct rdsp_channelizer rdsp_channelizer_t;
int rdsp_channelizer_create(int n_sources, int device, int P, int Q, int M, int D2, int format /* RDSP_SRC_* */,
                            int max_blocks_per_call, rdsp_channelizer_t **out);
void rdsp_channelizer_destroy(rdsp_channelizer_t *c);
int rdsp_channelizer_reset(rdsp_channelizer_t *c, void *stream);   /* histories, frac and T mod M zero */
size_t rdsp_channelizer_source_pairs(const rdsp_channelizer_t *c, int n_blocks); /* pairs the NEXT update consumes */
int rdsp_channelizer_update(rdsp_channelizer_t *c, const void *d_src, size_t src_stride /* pairs */, int n_blocks,
                            float *d_sub /* float2 [n_sources * M][sub_stride] */, size_t sub_stride /* pairs */, void *stream);
int rdsp_channelizer_sources(const rdsp_channelizer_t *c);
int rdsp_channelizer_subbands(const rdsp_channelizer_t *c);        /* M */
int rdsp_channelizer_decimation(const rdsp_channelizer_t *c);      /* D2 */
int rdsp_channelizer_source_rate(const rdsp_channelizer_t *c, int *P, int *Q); /* in lowest terms */
int rdsp_channelizer_format(const rdsp_channelizer_t *c);
int rdsp_channelizer_device(const rdsp_channelizer_t *c);
/* host only, no device */
int rdsp_channelizer_rate(int P, int Q, int D2, int *P1, int *Q1);   /* P / (Q D2) in lowest terms, or refused */
int rdsp_channelizer_taps(int P, int Q, int D2, float *out /* [16 ceil(P1 / Q1) Q1] */);
int rdsp_channelizer_twiddles(int M, float *out /* [M][2] */);
int rdsp_channelizer_place(int P, int Q, int M, double station_hz, int *subband, double *residual_hz);
/* Signal meter, squelch and active-receiver list.  The engine writes audio for every receiver on every call; the meter says
 * which receivers hear something.  Off until rdsp_engine_enable_meter: an engine that never calls it allocates, launches,
 * returns and saves exactly what it did before the meter existed.  Everything runs on the device inside rdsp_engine_update,
 * rdsp_engine_update_sources and rdsp_engine_update_source_samples, stream-ordered behind the call's audio.
 * What is measured: the float row of demodulated audio per channel -- behind the IF band-pass and the detector (so in-band),
 *   in front of the audio filter, the AGC and the ALS filter (so it still carries the level); full scale is +-1.0.
 * Per channel and per block of 128 samples a[0..127] of that row, in block order (arithmetic: csrc/rdsp_meter.h, float32, no
 *   contraction):
 *   - mean square: q[t] = a[t] a[t], one rounded product each; the q are summed by the balanced binary tree over adjacent
 *     pairs in index order (q[0] + q[1], q[2] + q[3], ...; seven levels); ms = sum x 0.0078125f (exact).  The tree is the
 *     definition: it is what a wave computes by an exchange reduction, and float addition being commutative an xor butterfly
 *     with strides 1, 2, 4, ... gives the same bits.
 *   - peak: pk = max over t of fabsf(a[t]) by fmaxf (a NaN sample is passed over; the order does not matter).
 *   - level: d = ms - L; L <- fmaf(d > 0 ? attack : decay, d, L).  L is 0 at create and after rdsp_engine_reset.  attack and
 *     decay lie in (0, 1]; the defaults 0.5f and 0.0625f rise within two blocks and fall over about 16 (46 ms).
 *   - gate, evaluated after the level, with integer state open and hang (both 0 at create and after reset):
 *       squelch off (the default): open = 1, hang = hang_blocks;
 *       squelch on: if L >= open_ms: open = 1, hang = hang_blocks; else if open and L >= close_ms: hang = hang_blocks;
 *       else if open and hang > 0: hang--; otherwise open = 0.
 *     0 <= close_ms <= open_ms, both finite; 0 <= hang_blocks <= 65535.  Thresholds are mean squares: a sine at x dB re full
 *     scale has ms = 0.5 x 10^(x / 10).
 *   - audio: a block whose gate is closed leaves as 128 zero words (what rdsp_engine_setMute writes); an open block leaves
 *     exactly as without the meter.  The engine's own signal state (filters, AGC, ALS) runs on regardless: opening restarts
 *     nothing.
 *   - active list: after a call, the channels whose gate was open in at least one block of that call, ascending, and their
 *     count (an ordered scan on the device; no atomics).
 *   Everything is a function of whole blocks and calls are whole blocks: levels, gates, audio and the union of the lists do
 *   not depend on how the stream is cut into calls.
 * - rdsp_engine_enable_meter allocates (per channel 32 bytes, 9 bytes per block of max_blocks_per_call, one list entry); it
 *   takes no stream and waits for everything queued on the engine's device, as rdsp_engine_set_sources does.  Again: a no-op.
 * - rdsp_engine_set_meter, rdsp_engine_set_squelch, rdsp_engine_disable_squelch are settings of the selected group
 *   (rdsp_engine_select_group): a new group copies them, rdsp_engine_reset keeps them, no blob carries them.  They may
 *   precede rdsp_engine_enable_meter and are in force once it is on.
 * - rdsp_engine_read_meter copies the last call's per-block L, pk and open, [ch][n_blocks] with the given strides (elements),
 *   into the caller's DEVICE buffers, stream-ordered; any pointer may be NULL; n_blocks may not exceed the last call's.
 *   rdsp_engine_active copies the list (room for n_channels entries; the entries behind the count are unspecified) and the
 *   count likewise.  rdsp_engine_get_meter reads through the host: host_out[ch][4] = level, the last call's last block's ms,
 *   its pk, open (0.0 / 1.0).
 * - rdsp_engine_read_demod copies the last call's rows of demodulated float audio -- what the meter measured -- into d_out
 *   [ch][out_stride], n_blocks x 128 floats a row; it works without the meter (float audio in front of the AGC).
 * - L, open and hang are signal state: they stay with the channel through regroupings, are zeroed by rdsp_engine_reset, and
 *   travel in rdsp_engine_save_state / load_state as the tuning phases do: an engine with the meter sets header flag 2 and
 *   appends three words per channel (level, open, hang), behind the phase words if there are any; rdsp_engine_state_bytes
 *   says so.  The blob of an engine without the meter is unchanged.  Loading a blob with meter words needs the meter
 *   (RDSP_ERR_NOT_READY); loading one without them into an engine with the meter zeroes those channels' meter state.
 * - Refused with nothing changed: RDSP_ERR_INVALID for a NaN or out-of-range parameter, close_ms > open_ms, a stride below
 *   n_blocks (n_blocks x 128 for read_demod), n_blocks above the last call's; RDSP_ERR_NOT_READY for rdsp_engine_read_meter,
 *   rdsp_engine_active and rdsp_engine_get_meter before rdsp_engine_enable_meter. */
int rdsp_engine_enable_meter(rdsp_engine_t *e);
int rdsp_engine_meter_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_meter(rdsp_engine_t *e, float attack, float decay);
int rdsp_engine_set_squelch(rdsp_engine_t *e, float open_ms, float close_ms, int hang_blocks);
int rdsp_engine_disable_squelch(rdsp_engine_t *e);
int rdsp_engine_read_meter(rdsp_engine_t *e, int n_blocks, float *d_level, size_t level_stride, float *d_peak, size_t peak_stride,
                           uint8_t *d_open, size_t open_stride, void *stream);
int rdsp_engine_active(rdsp_engine_t *e, int32_t *d_list, int32_t *d_count, void *stream);
int rdsp_engine_get_meter(rdsp_engine_t *e, float *host_out /* [n_channels][4] */, void *stream);
int rdsp_engine_read_demod(rdsp_engine_t *e, int n_blocks, float *d_out, size_t out_stride, void *stream);
/* Packed audio of the open receivers.  The engine hands back every receiver's stereo row on every call; with a squelch in
 * force most of it is zero words, and the right word always repeats the left.  rdsp_engine_pack_active gathers, after a call,
 * the blocks whose gate was open into dense mono blocks with a record each.  Opt-in, and needs rdsp_engine_enable_meter: an
 * engine that never calls it launches and allocates what it did before.  On the device, no atomics, the same bytes every time.
 *   - open[ch][b] are the last call's gate records (what rdsp_engine_read_meter returns).  The packed sequence is every
 *     (ch, b) with b < n_blocks and open[ch][b] != 0, by channel ascending, then block ascending.  needed = its length,
 *     written = min(needed, capacity_blocks); d_counts[0] = needed, d_counts[1] = written.
 *   - for k < written: d_records[k] = {ch, b} of the k-th element (b: the block's index inside the call), and
 *     d_audio[k * 128 + t] = the LEFT word d_lr[(ch * out_stride + b * 128 + t) * 2], t = 0 ... 127.  Nothing at or behind
 *     index `written` is written in either buffer.  Closed blocks of d_lr are never read.
 *   - d_lr, out_stride are the rows the last update wrote, as passed to it (any of rdsp_engine_update, _update_sources,
 *     _update_source_samples); n_blocks may be less than the call's.  The call is stream-ordered on `stream` behind whatever
 *     that update left; it modifies neither d_lr nor the meter's state or records, and may be repeated, also with another
 *     capacity.  d_audio must be 16-byte aligned; d_lr rows that are not take 4-byte loads.
 *   - sizing call: capacity_blocks == 0 with d_audio == d_records == NULL writes the counts only.
 *   - squelch off: every block is open, and the call is the stereo-to-mono transpose of the whole output.
 *   - n_blocks == 0, or no update made yet: counts {0, 0}.
 *   - the first call allocates the scratch (4 bytes per channel), not rdsp_engine_enable_meter; if that fails the call
 *     returns RDSP_ERR_NOMEM and the engine is as it was.
 *   - Refused with nothing written: RDSP_ERR_NOT_READY before rdsp_engine_enable_meter; RDSP_ERR_INVALID for d_lr or d_counts
 *     NULL, n_blocks < 0 or above the last call's, out_stride < n_blocks x 128, capacity_blocks > 0 with a NULL d_audio or
 *     d_records, d_audio not 16-byte aligned, capacity_blocks above INT32_MAX (and n_channels x n_blocks above INT32_MAX,
 *     which the counts could not hold).
 * rdsp_pack_runs (host only) merges records of one channel with consecutive blocks into runs: block = first_block + the
 *   first record's block (the run's absolute first block, first_block being the call's), record = the index of its first
 *   packed block, n_blocks its length: "receiver c, blocks B ... B + n - 1, audio at offset r".  It returns the number of runs,
 *   also when max_runs is too small (then the first max_runs are written), or RDSP_ERR_INVALID -- nothing written -- for
 *   records that are negative or not strictly ascending in (channel, block), negative counts or a NULL array with a count above
 *   0.  Runs that touch a call boundary are joined by the caller, with first_block. */
typedef struct { int32_t channel, block; } rdsp_pack_record_t;
typedef struct { int32_t channel, n_blocks, record; int64_t block; } rdsp_pack_run_t;
int rdsp_engine_pack_active(rdsp_engine_t *e, const int16_t *d_lr, size_t out_stride, int n_blocks,
                            int16_t *d_audio /* [capacity_blocks][128] */, rdsp_pack_record_t *d_records /* [capacity_blocks] */,
                            size_t capacity_blocks, int32_t *d_counts /* [2]: needed, written */, void *stream);
int rdsp_pack_runs(const rdsp_pack_record_t *records, int n_records, int64_t first_block, rdsp_pack_run_t *runs, int max_runs);
/* Voice-rate audio.  The engine writes int16 audio at 44 100 Hz; what its audio filters pass is voice, about 3 kHz wide.  With
 * rdsp_engine_enable_voice(e, R), R = 2 or 4 (one per engine), every call also low-passes and decimates the LEFT words of every
 * receiver's output row by R on the device, behind the meter's gate, into rows the engine owns: 22 050 or 11 025 Hz, a half or
 * a quarter of the bytes.  Opt-in: an engine that never calls it allocates, launches, returns and saves what it did before.
 *   Taps: T = 16 R, q_k = (int32) rint((double) h_k x 2^18), h = rdsp_engine_ddc_taps(R, 1.0f): the Kaiser-windowed sinc (beta 9)
 *     of the source passes, here at the input rate 44 100 Hz with its cutoff at the output's Nyquist frequency 44100 / (2 R).
 *     rdsp_engine_voice_taps writes them; host only, no GPU.  sum q = 2^18 (R = 2), 2^18 + 2 (R = 4); sum |q| / 2^18 = 1.649,
 *     1.603; ripple <= 0.0005 dB on |f| <= 0.544 fs / (2 R) (6 000 / 3 000 Hz); at least 91.0 dB down from 1.456 fs / (2 R)
 *     (16 050 / 8 025 Hz) to 22 050 Hz.  Between those two edges lies the transition band: at R = 4 whatever the audio filter
 *     leaves between 5.5 and 8 kHz folds onto 3 ... 5.5 kHz; R = 2 is the setting for AM.
 *   Stream: x[n] is the stream of left words of a channel's output row exactly as the call leaves it -- behind the gate, so a
 *     closed block is 128 zeros; n counts from the last reset and x[n] = 0 for n < 0.
 *   Output:  acc[m] = sum_{k < T} q_k x[R m + R - 1 - k]                 exact integer, |acc| < 2^34
 *            y[m]   = clamp((acc[m] + 2^17) >> 18, -32768, 32767)         arithmetic shift: floor, ties upwards
 *     The window of output m ends at the newest of its R samples (the decimating pass's convention); a block of 128 samples
 *     gives 128 / R outputs, so blocks stay aligned and there is no phase state.  The sum is exact, so the order of the adds
 *     is free: no tile, lane or call size is in the bits, and the rows do not depend on how the stream is cut into calls.
 *   State: per channel the last 60 left words of x, oldest first, as int32 (60 = 15 R at R = 4; R = 2 uses the newest 30):
 *     the same words whatever R, so a receiver moves between engines with different R.  Signal state: it stays with the channel
 *     through rdsp_engine_set_groups, is zeroed by rdsp_engine_reset, and travels in rdsp_engine_save_state / load_state as a
 *     third optional part: header flag 4, 60 words per channel, behind the meter's words; rdsp_engine_state_bytes says so.  The
 *     blob of an engine without the stage is unchanged; a blob with the part is refused by an engine without the stage
 *     (RDSP_ERR_NOT_READY, nothing changed); a blob without it zeroes the history of the channels it lands on.
 * - rdsp_engine_enable_voice works as rdsp_engine_enable_meter does: it takes no stream, waits for everything queued on the
 *   engine's device, then allocates the history (240 bytes a channel) and the rows, int16 [ch][max_blocks x 128 / R]; if that
 *   fails the object is as it was (RDSP_ERR_NOMEM).  The same R again: RDSP_OK, nothing changed.  Another R once the stage is on,
 *   or an R other than 2 or 4: RDSP_ERR_INVALID, nothing changed.  It does not need the meter.  rdsp_engine_voice_rate: 0 while
 *   the stage is off, otherwise R.
 * - From then on every rdsp_engine_update runs the stage once, behind the last group's meter kernel, on the caller's stream
 *   -- so also inside rdsp_engine_update_sources and _update_source_samples.  It reads d_lr and writes the engine's rows and
 *   the history; n_blocks == 0 launches nothing.
 * - rdsp_engine_read_voice copies the last call's rows, n_blocks x 128 / R words a row, into d_out [ch][out_stride] (a DEVICE
 *   buffer), stream-ordered, as rdsp_engine_read_demod does.  RDSP_ERR_NOT_READY before rdsp_engine_enable_voice;
 *   RDSP_ERR_INVALID for a NULL d_out, n_blocks negative or above the last call's, out_stride below the row.
 * - rdsp_engine_pack_voice is rdsp_engine_pack_active for these rows: the packed sequence, the records, needed / written, the
 *   sizing call, "nothing at or behind written is written", the counts {0, 0} of n_blocks == 0, repeatability and the refusals
 *   are the same; the blocks are 128 / R words (d_audio[k x 128 / R + t]), there is no d_lr, and d_audio must be 16-byte
 *   aligned.  It needs the meter and the stage, otherwise RDSP_ERR_NOT_READY.  rdsp_pack_runs serves unchanged. */
int rdsp_engine_voice_taps(int R, int32_t *out /* [16 R] */);
int rdsp_engine_enable_voice(rdsp_engine_t *e, int R);
int rdsp_engine_voice_rate(const rdsp_engine_t *e);
int rdsp_engine_read_voice(rdsp_engine_t *e, int n_blocks, int16_t *d_out, size_t out_stride, void *stream);
int rdsp_engine_pack_voice(rdsp_engine_t *e, int n_blocks, int16_t *d_audio /* [capacity_blocks][128 / R] */,
                           rdsp_pack_record_t *d_records /* [capacity_blocks] */, size_t capacity_blocks,
                           int32_t *d_counts /* [2]: needed, written */, void *stream);
/* Narrow-band FM.  Between 30 MHz and 1 GHz nearly every voice channel is narrow-band FM; the sketch's engine has no FM mode,
 * this is a design of this build.  After rdsp_engine_enable_fm(e), rdsp_engine_setDemodMode(e, RDSP_ENGINE_MODE_NFM) puts the
 * selected group(s) into NFM: one kernel stands where the IF filter, the mixer and the detector stood, the audio filter, AGC,
 * ALS, output gain and mute run unchanged on what it writes, and the group's meter measures the POWER IN THE CHANNEL, not the
 * audio -- a carrier squelch: a discriminator with no signal delivers full-scale noise, which would hold an audio squelch open.
 * Opt-in: an engine that never calls rdsp_engine_enable_fm allocates, launches, returns and saves what it did before.
 *   Input: the receiver's int16 IQ row at 44 100 Hz exactly as rdsp_engine_update receives it (with sources: the tuned row).
 *     x[n] = ((float) I, (float) Q) in counts; n counts from the last FM reset and x[n] = 0 for n < 0.  NFM ignores
 *     rdsp_engine_setInputGain, rdsp_engine_setIQgainBalance and the blanker: a discriminator does not care about amplitude.
 *   1. Channel filter.  h = rdsp_engine_ddc_taps(W, 1.0f), T = 16 W taps: the Kaiser-windowed sinc of the source passes at the
 *      input rate.  zI[n] is ONE chain over k ascending from 0, zI = fmaf(h[k], xI[n - k], zI); zQ likewise.  On the float taps:
 *        W = 2 (wide):   within 0.001 dB to 7 kHz, -0.07 dB at 8 kHz, -6 dB at 11.0 kHz, -17 dB at 12.5 kHz, >= 90 dB from 16.05 kHz
 *        W = 3 (narrow): within 0.001 dB to 4 kHz, -0.13 dB at 5.5 kHz, -6 dB at 7.35 kHz, >= 82 dB from 10 kHz
 *      for 5 kHz deviation on 25 kHz channels (Carson +-8 kHz) and 2.5 kHz on 12.5 kHz channels (+-5.5 kHz).  sum |h| <= 1.65.
 *   2. Level row.  lvl[n] = sqrtf(fmaf(zI, zI, zQ zQ)) 2^-15, the square root correctly rounded.  A full-scale complex carrier
 *      reads 1.0; its mean square, 1.0, is +3 dB on the scale of the meter's thresholds, which is referred to a real sine.
 *   3. Discriminator.  (pI, pQ) = z[n - 1]; re = fmaf(zI, pI, zQ pQ); im = fmaf(zQ, pI, -(zI pQ)); d[n] = fm_atan2(im, re).
 *      fm_atan2(y, x) is this build's own function (csrc/rdsp_fm.h has every operation): +0 when both arguments are 0; t =
 *      min(|x|, |y|) / max(|x|, |y|), one correctly rounded quotient; a seven-term odd polynomial in t by Horner with fmaf;
 *      pi/2 - p when |y| > |x|, pi - p when x < 0, the sign bit of y.  Its worst error against the double atan2, measured over
 *      every t = j / 2^20 and a million drawn pairs, is 5.2e-7 rad (the bound: 2^-19).  rdsp_engine_fm_atan2 exports it.
 *   4. Scale and clip.  k = (float)(44100.0 / (6.283185307179586 (double) deviation_hz)); u[n] = fminf(fmaxf(d[n] k, -1), 1).
 *      The peak deviation reads +-1.0; the noise of an empty channel is clipped to the rails.
 *   5. De-emphasis.  a = (float)(1.0 / (1.0 + 44100.0 (double) tau_us 1e-6)); y[n] = fmaf(a, u[n] - y[n - 1], y[n - 1]).
 *      tau_us == 0 bypasses the stage (y = u).  rdsp_engine_fm_constants writes {k, a}; host only, no GPU.
 *   6. Output.  y[n] is the "demod" tap (rdsp_engine_read_demod); the tail runs on it with the group's settings.  The useful
 *      combination is one of the audio band-passes (they remove sub-audible tones from the audio; the tone squelch below
 *      listens for them on this tap, in front of those filters) with the AGC off.
 *   7. Meter.  For a group in NFM the meter is handed the level rows in place of the demodulated ones: level, peak, gate, hang,
 *      the zeroing of closed blocks, the active list, rdsp_engine_pack_active, the voice stage and rdsp_engine_pack_voice work
 *      unchanged.  Thresholds stay mean squares.
 *   Everything is a function of the sample index: a stream gives the same bits however it is cut into calls.
 *   State: per channel 50 words -- the newest 47 input pair words (I | Q << 16), oldest first (W = 2 uses the newest 31); z[n - 1],
 *     two floats; y[n - 1].  Signal state: it stays with the channel through rdsp_engine_set_groups, is zeroed by
 *     rdsp_engine_reset and by a pending FM reset at the next update, is maintained only while the group is in NFM, and travels
 *     in rdsp_engine_save_state / load_state as a fourth optional part: header flag 8, 50 words per channel, behind the voice
 *     history; rdsp_engine_state_bytes says so.  The blob of an engine without FM is unchanged; a blob with the part is refused
 *     by an engine without FM (RDSP_ERR_NOT_READY, nothing changed); a blob without it zeroes the detector words of the channels
 *     it lands on.  NFM groups do not move the side-band lines (as AM).
 * - rdsp_engine_enable_fm works as rdsp_engine_enable_meter does: it takes no stream, waits for everything queued on the
 *   engine's device, then allocates the state (200 bytes a channel) and the level rows, float [ch][max_blocks x 128]; if that
 *   fails the object is as it was (RDSP_ERR_NOMEM).  Again: RDSP_OK, nothing changed.
 * - rdsp_engine_setDemodMode(e, RDSP_ENGINE_MODE_NFM) after it: returns TuningOffset 0.0 (the station sits at DC, so
 *   rdsp_engine_tune, the source passes and rdsp_channelizer_place work unchanged) and leaves a reset of the group's detector
 *   words pending, with the rules of the other pending resets (rdsp_engine_set_groups below).  Before rdsp_engine_enable_fm
 *   the value is one the engine does not know, as ever: the group's mode word becomes 7 and nothing else changes.  A later
 *   rdsp_engine_enable_fm leaves such a group alone -- it runs no detector until rdsp_engine_setDemodMode(e, 7) is called again,
 *   after rdsp_engine_enable_fm.  Leaving the mode and coming back resets the detector.
 * - rdsp_engine_set_fm(e, W, deviation_hz, tau_us): settings of the selected group(s), copied by a new group, kept by reset,
 *   in no blob; they may precede rdsp_engine_enable_fm.  W is 2 or 3, deviation_hz in [1000, 7500], tau_us 0 or in [25, 1000];
 *   the defaults are 2, 5000, 750.  Anything else: RDSP_ERR_INVALID, nothing changed.
 * - rdsp_engine_read_fm_level copies the last call's level rows, n_blocks x 128 floats a row, into d_out [ch][stride] (a DEVICE
 *   buffer), stream-ordered, as rdsp_engine_read_demod does; rows of receivers not in NFM read as zeros.  RDSP_ERR_NOT_READY
 *   before rdsp_engine_enable_fm; RDSP_ERR_INVALID for a NULL d_out, n_blocks negative or above the last call's, a short stride. */
#define RDSP_ENGINE_MODE_NFM 7
int rdsp_engine_enable_fm(rdsp_engine_t *e);
int rdsp_engine_fm_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_fm(rdsp_engine_t *e, int W, float deviation_hz, float tau_us);
int rdsp_engine_read_fm_level(rdsp_engine_t *e, int n_blocks, float *d_out, size_t stride, void *stream);
float rdsp_engine_fm_atan2(float y, float x);
int rdsp_engine_fm_constants(float deviation_hz, float tau_us, float *out /* [2]: k, a */);
/* Tone squelch (CTCSS).  Repeater outputs and shared simplex channels carry several user groups on one frequency, separated by
 * a sub-audible tone (67.0 ... 254.1 Hz at 10 ... 15 % of the peak deviation); a receiver set to one group stays shut for the
 * others, and for interference that opens a carrier gate.  After rdsp_engine_enable_tone(e) every NFM group runs one more kernel
 * behind its meter kernel (behind its tail kernel without a meter): a correlator per receiver at the receiver's own tone, on the
 * "demod" tap, where +-1.0 is the peak deviation -- so a tone's amplitude there is a physical quantity and needs no AGC or
 * reference level.  The tone is per CHANNEL (rdsp_engine_set_tones, as rdsp_engine_tune gives one station per channel), the
 * window and the thresholds per GROUP (rdsp_engine_set_tone_squelch).  Opt-in: an engine that never calls
 * rdsp_engine_enable_tone allocates, launches, returns and saves what it did before.  The arithmetic is csrc/rdsp_tone.h's.
 *   a[n] is the receiver's "demod" tap, y[n] of step 6 above: what rdsp_engine_read_demod returns.  Per channel:
 *   1. Step.  dphi = (uint32) llround((double) tone_hz 2^32 / 44100.0); tone_hz is 0 (no tone, the default) or in [60, 300].
 *   2. Block correlation.  The phase ph is a uint32.  For t = 0 ... 127 of a block: (c, s) = the tuning pass's phasor at
 *      ph + t dphi (the 1024-entry table of rdsp_engine_tune_table and its interpolation, unchanged; the detector keeps a copy of
 *      its own); pr[t] = a[t] c, pi[t] = a[t] s, one rounded product each; Sr, Si = their sums by the meter's balanced binary
 *      tree over adjacent pairs.  Then re = re + Sr, im = im + Si (one add each), ph += 128 dphi, cnt += 1.
 *   3. Window.  K blocks, non-overlapping, counted from the detector's last reset.  When cnt == K:
 *      a2 = fmaf(re, re, im im) scale, scale = (float)(4.0 / ((128.0 K) (128.0 K))): the squared amplitude of a sinusoid at the
 *      tone's frequency; tone = a2 >= (tone ? off2 : on2), on2 = on_amp on_amp and off2 = off_amp off_amp as float products;
 *      then re = im = 0 and cnt = 0.
 *   4. Records.  After block b of a call: a2_rec[ch][b] = a2, the last completed window's value (0 before the first), and
 *      tone_rec[ch][b] = tone.
 *   5. Gate.  Only with the meter on, and only for a channel with dphi != 0: open[ch][b] <- open[ch][b] & tone_rec[ch][b] in the
 *      meter's per-call record; a block closed this way is written as 128 zero words, exactly what the meter writes for its own
 *      closed blocks; the channel's entry in the active list follows the combined records.  The meter's signal state (level,
 *      open, hang) is NOT touched: the carrier gate evolves as it does without the detector.  So rdsp_engine_read_meter's
 *      d_open, rdsp_engine_active, rdsp_engine_pack_active, the voice stage and rdsp_engine_pack_voice see the COMBINED gate,
 *      while rdsp_engine_get_meter's fourth value stays the CARRIER gate.  With the meter's squelch off (always open) the tone
 *      gate works alone.  Without the meter nothing is gated: the records are all there is.
 *   6. Everything is a function of whole blocks counted from a reset: a stream gives the same bits however it is cut into calls.
 *   Latency: the gate opens at the end of the first full window that carries the tone, so up to two windows of a transmission's
 *     start are lost (K = 128 blocks: 0.37 s a window), and it closes a window after the tone stops.  This is the nature of tone
 *     squelch.
 *   State: per channel 8 words -- dphi, K, ph, re, im, cnt, tone, a2.  At the start of a call the stored dphi and K are compared
 *     with the channel's current tone and its group's K; if either differs the detector starts from zeros (tone = 0, a2 = 0).
 *     That one rule covers a changed tone, a changed K, a regrouping into a group with another K and a loaded blob that does not
 *     match.  A channel with dphi == 0 has its words and its records written as zeros and is not gated.  Signal state: it stays
 *     with the channel through rdsp_engine_set_groups, is zeroed by rdsp_engine_reset and by the group's pending FM reset at the
 *     next update, is maintained only while the group is in NFM, and travels in rdsp_engine_save_state / load_state as a fifth
 *     optional part: header flag 16, 8 words per channel, behind the FM words; rdsp_engine_state_bytes says so.  The blob of an
 *     engine without the detector is unchanged; a blob with the part is refused by an engine without it (RDSP_ERR_NOT_READY,
 *     nothing changed); a blob without it zeroes the words of the channels it lands on.
 * - rdsp_engine_enable_tone works as rdsp_engine_enable_fm does: it takes no stream, waits for everything queued on the engine's
 *   device, then allocates 32 bytes of state and 4 bytes of step per channel, 5 bytes per channel and block of max_blocks and the
 *   16 KiB table; if that fails the object is as it was (RDSP_ERR_NOMEM).  Again: RDSP_OK, nothing changed.  It needs
 *   rdsp_engine_enable_fm first (RDSP_ERR_NOT_READY) and does not need the meter.
 * - rdsp_engine_set_tones(e, first_channel, n_channels, tone_hz): the tones of a channel range from a HOST array, kept in a host
 *   mirror and uploaded stream-ordered at the next update, as rdsp_engine_tune's steps are.  Settings: kept by reset, in no
 *   blob, and they may precede rdsp_engine_enable_tone.  A NaN or a value outside {0} and [60, 300] anywhere in the array, a NULL
 *   array or a range outside the object: RDSP_ERR_INVALID, nothing changed.
 * - rdsp_engine_set_tone_squelch(e, K, on_amp, off_amp): settings of the selected group(s), copied by a new group, kept by
 *   reset, in no blob.  K in 4 ... 512; 0 < off_amp <= on_amp <= 1; the defaults are 128, 0.04, 0.025.  Anything else:
 *   RDSP_ERR_INVALID, nothing changed.
 * - rdsp_engine_read_tone copies the last call's records, [ch][n_blocks] with the given strides (elements), into the caller's
 *   DEVICE buffers, stream-ordered; either pointer may be NULL; rows of receivers the detector did not run on read as zeros.
 *   RDSP_ERR_NOT_READY before rdsp_engine_enable_tone; RDSP_ERR_INVALID for n_blocks negative or above the last call's, a stride
 *   below n_blocks.
 * - rdsp_engine_tone_gain(tone_hz, tau_us), host only: the magnitude of the de-emphasis of step 5 above at tone_hz, in double
 *   (1.0 for tau_us == 0), with which a caller turns "tone deviation in Hz" into a threshold on the tap: a tone at d Hz of
 *   deviation reads d / deviation_hz x gain.  0.0 for a tone_hz outside (0, 22050) or a tau_us rdsp_engine_set_fm refuses. */
int rdsp_engine_enable_tone(rdsp_engine_t *e);
int rdsp_engine_tone_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_tones(rdsp_engine_t *e, int first_channel, int n_channels, const float *tone_hz /* host */);
int rdsp_engine_set_tone_squelch(rdsp_engine_t *e, int K, float on_amp, float off_amp);
int rdsp_engine_read_tone(rdsp_engine_t *e, int n_blocks, float *d_a2, size_t a2_stride, uint8_t *d_tone, size_t tone_stride, void *stream);
double rdsp_engine_tone_gain(float tone_hz, float tau_us);
/* Tone search (CTCSS).  The tone squelch above holds a receiver shut until ITS tone is there; the tone search tells a caller WHICH
 * tone a channel carries -- receivers parked on stations a band survey found know their frequencies and not their tones.  After
 * rdsp_engine_enable_tone_search(e) every NFM group whose search window K is above 0 runs one more kernel behind its tone-squelch
 * kernel: a bank of correlators per receiver, one per tone of the engine's bank, on the "demod" tap decimated by 32.  It only
 * measures: it reads the demodulated rows and writes its own records and words; the audio, the meter's records and the active
 * list are untouched, and acting on the result (rdsp_engine_set_tones) is the caller's.  Opt-in: an engine that never calls
 * rdsp_engine_enable_tone_search allocates, launches, returns and saves what it did before.  It is independent of
 * rdsp_engine_enable_tone: each works without the other.  The arithmetic is csrc/rdsp_tone_search.h's.
 *   a[n] is the receiver's "demod" tap, the row the tone squelch reads; blocks of 128 samples are counted from the detector's
 *   last reset.
 *   1. Bank (one per engine, a setting).  n_tones frequencies, 1 <= n_tones <= 64, each in [60, 300] Hz, strictly ascending; the
 *      default is the 50 standard CTCSS tones 67.0 ... 254.1 Hz of the EIA list (rdsp_engine_tone_standard).  Step per DECIMATED
 *      sample: dphi_t = (uint32) llround((double) tone_hz_t 2^32 32 / 44100.0).  bank_key = 32-bit FNV-1a (offset basis
 *      2166136261, prime 16777619) over the little-endian bytes of n_tones (a uint32) and then of every dphi_t; a result of 0 is
 *      replaced by 1.
 *   2. Decimation by 32.  Block b gives four values d[b][q], q = 0 ... 3: the sum of a[128 b + 32 q ... + 31] by the meter's
 *      balanced binary tree over adjacent pairs in index order, cut off after five levels.  No products.  The rate is
 *      1378.125 Hz; every tone lies below 689 Hz.
 *   3. Bank correlation.  m = 4 cnt + q is the index of a decimated sample inside the current window, cnt the blocks completed in
 *      it.  For every tone t: (c, s) = the tuning pass's phasor at the uint32 product m dphi_t (it wraps; the 1024-entry table of
 *      rdsp_engine_tune_table and its interpolation, unchanged); re_t = fmaf(d, c, re_t), im_t = fmaf(d, s, im_t): one chain per
 *      tone over m ascending.  No phase is carried: a window starts at phase 0.
 *   4. Window.  K blocks, non-overlapping.  After a block cnt += 1; when cnt == K:
 *      P_t = fmaf(re_t, re_t, im_t im_t) scale, scale = (float)(4.0 / ((128.0 K) (128.0 K))) as in the tone squelch: the squared
 *      amplitude of a sinusoid at the tone as seen BEHIND the boxcar of step 2 (rdsp_engine_tone_search_gain);
 *      i = the lowest index with the largest P_t; next = the largest P_t over |t - i| > 1, or 0 if there is none (the two
 *      neighbours in the bank are left out: a short window cannot separate tones 2.3 Hz apart);
 *      found = P_i >= min2 && P_i >= ratio next, min2 = min_amp min_amp and ratio next one rounded float product each;
 *      best1 = found ? i + 1 : 0, a2 = P_i, and next is kept.  The P_t stay as the "last spectrum"; re, im and cnt go to 0.
 *   5. Records.  After block b of a call: best_rec[ch][b] = (uint8)(best1 - 1), 255: none; a2_rec[ch][b] = a2; next_rec[ch][b] =
 *      next -- the values of the last completed window, 255 / 0 / 0 before the first.
 *   6. Everything is a function of whole blocks counted from a reset: a stream gives the same bits however it is cut into calls.
 *   A short window declines to decide at the low end of the list (K = 32: 0.09 s a window, tones 2.3 Hz apart three bins away
 *     still leak above 1 / ratio); K = 128 separates every standard tone.
 *   State: per channel 200 words -- K, bank_key, cnt, best1, a2, next, 0, 0, then re[64], im[64], P[64]; lanes at or above n_tones
 *     hold zeros.  At the start of a call the stored K and bank_key are compared with the group's K and the engine's bank; if
 *     either differs, or the group's FM reset is pending, the detector starts from zeros.  That one rule covers a changed K, a
 *     changed bank, a regrouping into a group with another K and a loaded blob that does not match.  The words are zeroed by
 *     rdsp_engine_reset, are maintained only for NFM groups with K > 0 (a channel of a group with K == 0 has zero words from the
 *     next update on and the records 255 / 0 / 0 -- whatever the group's mode: K == 0 is looked at before the mode, so "off"
 *     never leaves words behind, while a group outside NFM with K > 0 leaves them alone), stay with the channel through
 *     rdsp_engine_set_groups, and travel in rdsp_engine_save_state / load_state as a sixth optional part: header flag 32, 200
 *     words per channel, behind the tone words;
 *     rdsp_engine_state_bytes says so.  The blob of an engine without the search is unchanged; a blob with the part is refused by
 *     an engine without it (RDSP_ERR_NOT_READY, nothing changed); a blob without it zeroes the words of the channels it lands on.
 * - rdsp_engine_enable_tone_search works as rdsp_engine_enable_tone does: it takes no stream, waits for everything queued on the
 *   engine's device, then allocates 800 bytes of state per channel, 9 bytes per channel and block of max_blocks, the bank's 256
 *   bytes and the 16 KiB table; if that fails the object is as it was (RDSP_ERR_NOMEM).  Again: RDSP_OK, nothing changed.  It
 *   needs rdsp_engine_enable_fm first (RDSP_ERR_NOT_READY) and neither the meter nor the tone squelch.
 * - rdsp_engine_set_tone_bank(e, tone_hz, n_tones): the bank from a HOST array, kept in a host mirror and uploaded stream-ordered
 *   at the next update when it changed.  A setting: kept by reset, in no blob, and it may precede the enable.
 *   rdsp_engine_tone_bank(e, out64) writes the bank in force (room for 64) and returns n_tones.  A NaN or a value outside
 *   [60, 300] anywhere, a bank that is not strictly ascending, n_tones outside 1 ... 64 or a NULL array: RDSP_ERR_INVALID, nothing
 *   changed.
 * - rdsp_engine_set_tone_search(e, K, min_amp, ratio): settings of the selected group(s), copied by a new group, kept by reset,
 *   in no blob.  K is 0 (off, the default) or 4 ... 512; 0 < min_amp <= 1 (default 0.04); 1 <= ratio <= 1e6 (default 4).  Anything
 *   else: RDSP_ERR_INVALID, nothing changed.
 * - rdsp_engine_read_tone_search copies the last call's records, [ch][n_blocks] with the given strides (elements), into the
 *   caller's DEVICE buffers, stream-ordered; any pointer may be NULL; rows of receivers the kernel did not run on read 255 / 0 /
 *   0.  RDSP_ERR_NOT_READY before rdsp_engine_enable_tone_search; RDSP_ERR_INVALID for n_blocks negative or above the last
 *   call's, a stride below n_blocks.
 * - rdsp_engine_read_tone_spectrum copies the last completed window's P_t of n_channels receivers from first_channel on,
 *   [ch][n_tones] floats with `stride` elements a row (at least n_tones of the bank in force), from the state words into the
 *   caller's DEVICE buffer, stream-ordered.  RDSP_ERR_NOT_READY before the enable; RDSP_ERR_INVALID for a NULL buffer, a range
 *   outside the object or a short stride.
 * - rdsp_engine_tone_standard(out50), host only: the 50 standard tones, ascending; returns 50.
 * - rdsp_engine_tone_search_gain(tone_hz, tau_us), host only, in double:
 *   |sin(32 pi f / 44100) / (32 sin(pi f / 44100))| x rdsp_engine_tone_gain(f, tau_us) -- the boxcar of step 2 and the
 *   de-emphasis: sqrt(a2) of a tone at d Hz of deviation reads d / deviation_hz x this.  The argument limits are
 *   rdsp_engine_tone_gain's (0.0 outside them). */
int rdsp_engine_enable_tone_search(rdsp_engine_t *e);
int rdsp_engine_tone_search_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_tone_bank(rdsp_engine_t *e, const float *tone_hz /* host */, int n_tones);
int rdsp_engine_tone_bank(const rdsp_engine_t *e, float *out64 /* host */);
int rdsp_engine_set_tone_search(rdsp_engine_t *e, int K, float min_amp, float ratio);
int rdsp_engine_read_tone_search(rdsp_engine_t *e, int n_blocks, uint8_t *d_best, size_t best_stride, float *d_a2, size_t a2_stride, float *d_next,
                                 size_t next_stride, void *stream);
int rdsp_engine_read_tone_spectrum(rdsp_engine_t *e, int first_channel, int n_channels, float *d_power, size_t stride, void *stream);
int rdsp_engine_tone_standard(float *out50 /* host */);
double rdsp_engine_tone_search_gain(float tone_hz, float tau_us);
/* Code squelch (DCS).  The other half of VHF / UHF channels separates its user groups not by a tone but by Digital Coded Squelch:
 * a 23-bit Golay word, repeated without a gap at 134.4 bit/s as sub-audible NRZ on the same "demod" tap.  After
 * rdsp_engine_enable_dcs(e) every NFM group runs one more kernel behind its tone-squelch kernel (behind its meter kernel without
 * one, behind its tail kernel without either), in front of the list kernel and the voice stage: per receiver bit timing, slicing
 * and code matching.  The code is per CHANNEL (rdsp_engine_set_dcs_codes), the window and the counts per GROUP
 * (rdsp_engine_set_dcs_squelch).  RDSP_DCS_ANY opens on any valid code and reads it out: that tells a caller WHICH code a channel
 * carries.  Opt-in: an engine that never calls rdsp_engine_enable_dcs allocates, launches, returns and saves what it did before.
 * It is independent of rdsp_engine_enable_tone and rdsp_engine_enable_tone_search.  The arithmetic is csrc/rdsp_dcs.h's.
 *   Code words (host only).  rdsp_dcs_codeword(code), code = 0 ... 511 (the octal digits read as a number: 023 is 19):
 *     data = 0x800 | code; parity = the remainder of data x^11 by g = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1 (0xC75);
 *     word = parity << 12 | data; code 023 gives 0x763813.  The word is sent LSB first, bit 1 is positive deviation (the tap above
 *     its mean); the inverted code is word ^ 0x7FFFFF.  A receiver does not know where a word begins, so a code is its word's
 *     class under the 23 rotations.  The 104 standard codes 023 ... 754 (rdsp_dcs_standard) lie in 104 distinct classes, any two
 *     at least 7 bits apart over all rotations; the 512 codes fall into 177 classes with at most one standard code each; and the
 *     inverted word of every standard code is a rotation of ANOTHER standard code's word (inverted 023 is normal 047).  So a
 *     read-out cannot tell "047" from "023 inverted": rdsp_dcs_code_of_word reports the NORMAL-polarity reading.
 *   a[n] is the receiver's "demod" tap; blocks of 128 samples are counted from the detector's last reset.
 *   1. Decimation by 32.  Exactly the tone search's step 2: d[b][q], q = 0 ... 3.  1378.125 Hz, 10.254 values a bit.
 *   2. Eight timing hypotheses p = 0 ... 7 with the bit phase bp_p = p 2^29 + M step (uint32, wrapping), M the count of decimated
 *      values since the detector's last reset, step = (uint32) llround(134.4 32 2^32 / 44100.0) = 418861572.  For every decimated
 *      value v in order: acc_p = acc_p + v for every p, a plain float add; then, if adding step wraps bp_p, hypothesis p TICKS.
 *      step < 2^29, so at most one hypothesis ticks per value.
 *   3. Tick.  ring_p[pos_p] = acc_p; pos_p = (pos_p + 1) mod 23; acc_p = 0; nb_p = min(nb_p + 1, 23);
 *      thr = (ring_p[0] + ring_p[1] + ... + ring_p[22]) (float)(1.0 / 23.0), the sum left to right, no contraction -- this removes
 *      the discriminator's DC, a tuning error: a whole word has a fixed weight, 11 or 12 ones for every standard code;
 *      w has bit j set iff ring_p[(pos_p + j) mod 23] > thr: j = 0 is the oldest bit.
 *   4. Match, counted only when nb_p == 23.  For a code: min over r of popcount(w ^ rot(want, r)) <= max_err, want the code's
 *      word, inverted if asked; the matched word is canon(want).  For RDSP_DCS_ANY: parity(w & 0xFFF) == w >> 12 and some rotation
 *      of w has bits 9 ... 11 equal to 100 (max_err is ignored); the matched word is canon(w).  canon is the smallest of the 23
 *      rotations, rot(w, r) = (w >> r | w << (23 - r)) & 0x7FFFFF.  On a match hits_p += 1 and last_p = the matched word.
 *   5. Window of K blocks, non-overlapping, counted from the detector's last reset.  After a block cnt += 1; when cnt == K:
 *      best = the lowest p with the largest hits_p; H = hits_best; dcs = H >= (dcs ? off_hits : on_hits);
 *      word = H ? last_best : 0; every hits_p and last_p go to 0 and cnt = 0.  Rings, phases and acc run on.
 *   6. Records.  After block b of a call dcs_rec (uint8), hits_rec (uint8) and word_rec (uint32) hold dcs, H and word of the last
 *      completed window, 0 before the first.
 *   7. Gate.  The tone squelch's rule 5 with dcs_rec in place of tone_rec and "code != 0" in place of "dphi != 0": only with the
 *      meter on, open[ch][b] <- open[ch][b] & dcs_rec[ch][b] in the meter's per-call record; a newly closed block is written as
 *      128 zero words; the channel's entry in the active list (MT_ANY) follows the combined records; the meter's signal state is
 *      NOT touched.  A channel with a tone and a code is gated by both.  Without the meter nothing is gated.
 *   8. Everything is a function of whole blocks counted from a reset: a stream gives the same bits however it is cut into calls.
 *   Latency: 23 bits take 59 blocks before anything can match; at the defaults the gate opens at the end of the second window.
 *   State: per channel 232 words -- a header key, K, cnt, dcs, H, word, M step (uint32), 0, then per hypothesis acc, pos, nb,
 *     hits, last, ring[23] (acc and ring floats).  key = 2^31 | ANY 2^30 | inverted 2^29 | max_err 2^24 | want, want the word
 *     looked for (inverted if asked; 0 for ANY).  At the start of a call the stored key and K are compared with the channel's
 *     and its group's; if either differs, or the group's FM reset is pending, the detector starts from zeros.  That one rule
 *     covers a changed code, polarity, max_err or K, a regrouping into a group with another K and a loaded blob that does not
 *     match.  A channel with code 0 has its words and its records written as zeros and is not gated.  The words are zeroed by
 *     rdsp_engine_reset, maintained only while the group is in NFM, stay with the channel through rdsp_engine_set_groups and
 *     travel in rdsp_engine_save_state / load_state as a seventh optional part: header flag 64, 232 words per channel, behind
 *     the tone-search words; rdsp_engine_state_bytes says so.  The blob of an engine without the detector is unchanged; a blob
 *     with the part is refused by an engine without it (RDSP_ERR_NOT_READY, nothing changed); a blob without it zeroes the
 *     words of the channels it lands on.
 *   Not built: the 134.4 Hz turn-off code a transmitter sends at the end of an over (the gate closes a window after the code
 *     stops instead); acting on a read-out on the device (setting the code found is the caller's); fusing the detectors into
 *     the FM kernel.
 * - rdsp_engine_enable_dcs works as rdsp_engine_enable_tone does: no stream, it waits for the engine's device, then allocates 928
 *   bytes of state and 4 bytes of setting per channel and 6 bytes per channel and block of max_blocks; if that fails the object
 *   is as it was (RDSP_ERR_NOMEM).  Again: RDSP_OK, nothing changed.  It needs rdsp_engine_enable_fm first (RDSP_ERR_NOT_READY).
 * - rdsp_engine_set_dcs_codes(e, first_channel, n_channels, codes): the codes of a channel range from a HOST array, kept in a
 *   host mirror and uploaded stream-ordered at the next update.  0: none (the default); 1 ... 511: a code; + 0x8000: that code
 *   with inverted polarity; RDSP_DCS_ANY.  Settings: kept by reset, in no blob, and they may precede the enable.  Any other value
 *   anywhere in the array, a NULL array or a range outside the object: RDSP_ERR_INVALID, nothing changed.
 * - rdsp_engine_set_dcs_squelch(e, K, max_err, on_hits, off_hits): settings of the selected group(s), copied by a new group, kept
 *   by reset, in no blob.  K in 8 ... 512; max_err in 0 ... 3; 1 <= off_hits <= on_hits <= K 128 134.4 / 44100 rounded down
 *   (= K 1024 / 2625: the bits of a window); the defaults are 64, 1, 16, 12 -- a window the code fills counts 25, and the window behind a code that
 *   stopped still counts up to 9 from the bits left in the rings (at max_err 1), which off_hits has to exceed for the gate to close
 *   one window after the code.  Anything else: RDSP_ERR_INVALID, nothing changed.
 * - rdsp_engine_read_dcs copies the last call's records, [ch][n_blocks] with the given strides (elements), into the caller's
 *   DEVICE buffers, stream-ordered; any pointer may be NULL; rows of receivers the kernel did not run on read as zeros.
 *   RDSP_ERR_NOT_READY before rdsp_engine_enable_dcs; RDSP_ERR_INVALID for n_blocks negative or above the last call's, a stride
 *   below n_blocks.
 * - rdsp_dcs_codeword(code), host only: the word above; 0 (and rdsp_last_error) for a code outside 0 ... 511.
 * - rdsp_dcs_standard(out104), host only: the 104 standard codes, ascending; returns 104.
 * - rdsp_dcs_code_of_word(word, code, inverted), host only: the lowest standard code whose word has `word` among its 23
 *   rotations, *inverted = 0; failing that the lowest standard code whose INVERTED word has, *inverted = 1 (by the class facts
 *   above this never happens for a standard word); failing that RDSP_ERR_INVALID, as for a NULL pointer or a word outside
 *   1 ... 0x7FFFFF. */
#define RDSP_DCS_ANY 0xFFFFu
#define RDSP_DCS_INVERTED 0x8000u
int rdsp_engine_enable_dcs(rdsp_engine_t *e);
int rdsp_engine_dcs_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_dcs_codes(rdsp_engine_t *e, int first_channel, int n_channels, const uint16_t *codes /* host */);
int rdsp_engine_set_dcs_squelch(rdsp_engine_t *e, int K, int max_err, int on_hits, int off_hits);
int rdsp_engine_read_dcs(rdsp_engine_t *e, int n_blocks, uint8_t *d_dcs, size_t dcs_stride, uint8_t *d_hits, size_t hits_stride, uint32_t *d_word,
                         size_t word_stride, void *stream);
uint32_t rdsp_dcs_codeword(int code);
int rdsp_dcs_standard(uint16_t *out104 /* host */);
int rdsp_dcs_code_of_word(uint32_t word, int *code, int *inverted);
/* Noise squelch.  The carrier squelch above compares the mean square of the IQ input with absolute thresholds, which depend on the
 * source's sample format, the gain folded into its filter, the channelizer and the dongle's AGC: receivers on sources of different
 * gains cannot share a pair of thresholds.  An FM receiver reads the discriminator's noise above the voice band instead: an empty
 * channel delivers full-scale noise there and a captured carrier quiets it, whatever the input level -- the "demod" tap reads
 * +-1.0 at the peak deviation at any gain.  After rdsp_engine_enable_noise(e) every NFM group whose mode is above 0 runs one more
 * kernel behind its meter kernel (behind its tail kernel without a meter), in front of its tone-squelch kernel.  Opt-in: an engine
 * that never calls rdsp_engine_enable_noise allocates, launches, returns and saves what it did before.  It is independent of the
 * tone squelch, the tone search and the code squelch.  The arithmetic is csrc/rdsp_noise.h's (compiled with -ffp-contract=off).
 *   a[n] is the receiver's "demod" tap, y[n] of the FM detector; n counts from the detector's last start.  Per channel:
 *   1. Taps.  rdsp_engine_noise_taps(tau_us, out[65]), host only.  The prototype is a band-pass of T = 64 taps, the difference of
 *      two windowed sincs with cutoffs f2 = 8000 Hz and f1 = 4500 Hz: hb[k] = (2 f2 / fs sinc(2 f2 / fs m) - 2 f1 / fs sinc(2 f1 / fs m))
 *      w[k], m = k - 31.5, fs = 44100, w the Kaiser window of beta 6; evaluated in double as ((s2 - s1) / u) (I0(6 sqrt(1 - rho^2)) /
 *      I0(6)) with q = |2 k - 63|, u = pi q / 2, rho = q / 63, s2 = sin(pi 160 q / 882), s1 = sin(pi 90 q / 882), the sine and I0 by
 *      the libm-free series of rdsp_engine_ddc_taps: every host and the numpy restatement give the same bits.  The tap sits behind
 *      the de-emphasis, which takes 29 dB off this band at 750 us; the taps undo it: with a the float of the FM detector's
 *      de-emphasis coefficient and r = 1 - (double) a, g[k] = (float)((hb[k] - r hb[k - 1]) / a), k = 0 ... 64, hb[-1] = hb[64] = 0;
 *      tau_us == 0: g[k] = (float) hb[k], g[64] = 0.  No normalisation: the prototype reads 0.0 dB at 6 kHz, -6 dB at 8 kHz,
 *      at most -63 dB up to 3 kHz and -37.6 dB at 3.4 kHz; the compensated taps at 750 us read -40 dB at 3 kHz.  The taps belong to
 *      the group through the tau_us of its rdsp_engine_set_fm.
 *   2. Block reading.  Only every fourth output of the filter is computed (the mean square of a subsampled stationary signal is
 *      the same mean square).  For j = 0 ... 31 of a block that begins at sample n0: v_j = ONE chain over k = 0 ... 64 ascending
 *      from 0, v = fmaf(g[k], a[n0 + 4 j + 3 - k], v); samples in front of the call come from the detector's history, zeros
 *      after a start.  q_j = v_j v_j; nz = tree(q_0 ... q_31) 0.03125f, adjacent pairs in index order over five levels (the
 *      strides 1, 2, 4, 8, 16 of the meter's exchange over 32 lanes).
 *   3. Level.  N <- the meter's level step, fmaf(nz - N > 0 ? rise : fall, nz - N, N): rise applies while the noise grows (the
 *      channel empties), fall while it drops (a carrier arrives).
 *   4. Gate, the meter's with the sense reversed.  N <= open_n: open = 1, hang = hang_blocks; else open && N <= close_n:
 *      hang = hang_blocks; else open && hang > 0: hang--; else open = 0.
 *   5. Settings, per group: mode 0 (off, the default), 1 (measure only) or 2 (gate); 0 < open_n <= close_n, both finite;
 *      hang_blocks 0 ... 65535; fall and rise in (0, 1].  The defaults are 0.01, 0.025, 8, 0.75, 0.125: rms 0.10 and 0.16 on the
 *      tap against an empty channel's 0.33.  (fall 0.5 was proposed first; from N = 1 it needs seven blocks to reach 0.01, and a
 *      strong station is to be open from its fourth block on: docs/engine.md.)
 *   6. Start.  Zero state must not read as "quiet", so the detector has a key word: 2^31 | mode 2^24 | W 2^16 | (tau_us != 0).  A
 *      stored key that differs from the one the channel is run with, or the group's pending FM reset, starts the detector:
 *      N = 1.0f, open = 0, hang = 0, history zeros.  That one rule covers a changed mode or W, a regrouping, a zeroing blob and
 *      rdsp_engine_reset (which zeroes the words).  A group with mode 0 has its channels' words and records written as zeros
 *      and is not gated.
 *   7. Records.  After block b of a call: noise_rec[ch][b] = N and nopen_rec[ch][b] = open.
 *   8. Gate into the engine, mode 2 only: the tone squelch's rule 5 with nopen_rec in place of tone_rec, for every channel of the
 *      group.  With the meter's squelch off the noise gate works alone -- the intended use.  Without the meter nothing is gated.
 *      The gates are ANDs: their order changes no result.
 *   9. Everything is a function of whole blocks counted from a start: a stream gives the same bits however it is cut into calls.
 *   An all-zero row (a dead source) lets N decay from 1.0: the gate OPENS on silence.  A dead source is not an empty channel.
 *   State: per channel 68 words -- key, N, open, hang, the newest 64 samples of the tap, oldest first.  Signal state: it stays with
 *     the channel through rdsp_engine_set_groups, is zeroed by rdsp_engine_reset, is maintained only while the group is in NFM, and
 *     travels in rdsp_engine_save_state / load_state as an eighth optional part: header flag 128, 68 words per channel, behind the
 *     code-squelch words.  The blob of an engine without the detector is unchanged; a blob with the part is refused by an engine
 *     without it (RDSP_ERR_NOT_READY, nothing changed); a blob without it zeroes the words, which by rule 6 restarts the
 *     detector closed.
 * - rdsp_engine_enable_noise works as rdsp_engine_enable_tone does: no stream, it waits for the engine's device, then allocates 272
 *   bytes of state per channel and 5 bytes per channel and block of max_blocks; if that fails the object is as it was
 *   (RDSP_ERR_NOMEM).  Again: RDSP_OK, nothing changed.  It needs rdsp_engine_enable_fm first (RDSP_ERR_NOT_READY), not the meter.
 * - rdsp_engine_set_noise_squelch: settings of the selected group(s), copied by a new group, kept by reset, in no blob.  Anything
 *   outside rule 5 (a NaN among them): RDSP_ERR_INVALID, nothing changed.
 * - rdsp_engine_read_noise copies the last call's records, [ch][n_blocks] with the given strides (elements), into the caller's
 *   DEVICE buffers, stream-ordered; either pointer may be NULL; rows of receivers the kernel did not run on read as zeros.
 *   RDSP_ERR_NOT_READY before rdsp_engine_enable_noise; RDSP_ERR_INVALID for n_blocks negative or above the last call's, a stride
 *   below n_blocks.
 * - rdsp_engine_noise_taps: RDSP_ERR_INVALID for a NULL out or a tau_us rdsp_engine_set_fm refuses. */
#define RDSP_NOISE_OFF 0
#define RDSP_NOISE_MEASURE 1
#define RDSP_NOISE_GATE 2
int rdsp_engine_enable_noise(rdsp_engine_t *e);
int rdsp_engine_noise_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_noise_squelch(rdsp_engine_t *e, int mode, float open_n, float close_n, int hang_blocks, float fall, float rise);
int rdsp_engine_read_noise(rdsp_engine_t *e, int n_blocks, float *d_noise, size_t noise_stride, uint8_t *d_open, size_t open_stride, void *stream);
int rdsp_engine_noise_taps(float tau_us, float *out /* [65], host */);
/* DTMF decoder.  The detectors above read what lies below and above the voice band; DTMF is the signalling INSIDE it (repeater
 * control, autopatch, selective calling and ANI, node control).  After rdsp_engine_enable_dtmf(e) every NFM group whose DTMF
 * frame length K is above 0 runs one more kernel behind its other detector kernels.  It only measures: it reads the "demod" tap
 * (1.0: the peak deviation, so a tone's amplitude is absolute and needs no AGC) and writes its own records and state words; the
 * audio, the meter's records, the gates and the active list are untouched.  An engine that never calls the enable allocates,
 * launches, returns and saves what it did before.  It is independent of the tone squelch, the tone search, the code squelch and
 * the noise squelch.  The arithmetic is csrc/rdsp_dtmf.h's (compiled with -ffp-contract=off, the fused operations written as
 * fmaf).  a[n] is the receiver's "demod" tap, in blocks of 128 samples counted from the detector's start.
 *   1. Tones.  t = 0 ... 3, the low group: 697, 770, 852, 941 Hz; t = 4 ... 7, the high group: 1209, 1336, 1477, 1633 Hz.  Fixed:
 *      there is no bank setter.  The step per DECIMATED sample is dphi_t = (uint32) llround(f_t 2^32 4 / 44100.0).
 *   2. Decimation by 4.  d[b][r] = (a0 + a1) + (a2 + a3) over samples 128 b + 4 r ... + 3, r = 0 ... 31: 11 025 Hz, no products.
 *   3. Correlation in eight sub-chains per tone.  A frame is K blocks.  Sub-chain j = 0 ... 7 of tone t takes the decimated
 *      samples r = 4 j ... 4 j + 3 of every block of the frame, blocks ascending, r ascending within a block: with m = 32 cnt + r
 *      (cnt the block's index in the frame), (c, s) = tune_phasor(tab, m dphi_t) (a wrapping uint32 product),
 *      re_tj = fmaf(d, c, re_tj), im_tj = fmaf(d, s, im_tj).  Beside them eight energy chains e_j = fmaf(d, d, e_j).
 *   4. Frame end (cnt == K).  RE_t, IM_t and E' are the sums over j by the tree ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).
 *      P_t = fmaf(RE_t, RE_t, IM_t IM_t) scale, scale = (float)(1 / (64 K)^2): a sine of amplitude A reads about A^2 (times
 *      rdsp_engine_dtmf_gain squared).  E = E' (float)(1 / (256 K)): a clean pair reads about A_L^2 + A_H^2.  In each group i is
 *      the lowest index of the largest P and `second` the largest of the other three; P_L, P_H the two maxima.  The frame's
 *      symbol is sym = 4 i_L + (i_H - 4) if all of
 *        P_L >= min2 and P_H >= min2 (min2 = min_amp min_amp);  P_L >= ratio second_L and P_H >= ratio second_H;
 *        P_L <= twist P_H and P_H <= twist P_L;  P_L + P_H >= share E
 *      hold (every product and the sum rounded floats), else 255.  The key is "123A456B789C*0#D"[sym] (rdsp_engine_dtmf_key).
 *      All chains and cnt go to 0.
 *   5. Digit logic, once per frame with the frame's symbol s; state last, run, cur, miss (255: none):
 *        run = (s != 255 && s == last) ? run + 1 : (s != 255);  last = s;
 *        if cur != 255: s == cur ? miss = 0 : (miss += 1, and miss >= off_frames: cur = 255);
 *        then if cur == 255 && run >= on_frames: cur = s, miss = 0, and a digit is emitted:
 *        ring[n_digits mod 16] = sym | (t_blocks & 0xFFFFFF) << 8, n_digits += 1; t_blocks counts the blocks since the detector's
 *        start, this one included.
 *   6. Records after block b of a call, each [ch][max_blocks]: key_rec = cur; new_rec = the symbol emitted by a frame that ended
 *      with this block, else 255; lo_rec, hi_rec = P_L, P_H of the last completed frame (0 before the first).  Receivers the
 *      kernel did not run on read 255 / 255 / 0 / 0.
 *   7. Everything is a function of whole blocks counted from the detector's start: a stream gives the same bits however it is
 *      cut into calls.
 * State: 168 words a channel (rdsp_dtmf.h: K, cnt, last + 1, run, cur + 1, miss, n_digits, t_blocks, P_L, P_H, six zeros,
 * ring[16], re[64], im[64], e[8]; last and cur are stored plus one modulo 256, so zeros are a detector that holds no key).  A
 * stored K that differs from the one the channel is run with, or the group's pending FM reset, starts the detector from zeros;
 * a change of thresholds does not.  The words are zeroed by rdsp_engine_reset, maintained only for NFM groups with K > 0 (a
 * group with K == 0 has its channels' words zeroed in the stream at every update, whatever its mode -- K == 0 is looked at
 * before the mode, as in the tone search; a group outside NFM with K > 0 leaves them alone), stay with the channel
 * through rdsp_engine_set_groups, and travel as a ninth optional part of the state blob (header flag 256): an engine without the
 * decoder writes the blob it always wrote and refuses one that carries the part (RDSP_ERR_NOT_READY); a blob without the part
 * zeroes the words.
 * - rdsp_engine_enable_dtmf works as rdsp_engine_enable_tone_search does: no stream, waits for the device, RDSP_ERR_NOT_READY
 *   before rdsp_engine_enable_fm, RDSP_ERR_NOMEM with the object unchanged, again a no-op.
 * - rdsp_engine_set_dtmf(e, K, min_amp, ratio, twist, share, on_frames, off_frames): settings of the selected group(s), copied
 *   by a new group, kept by reset, in no blob.  K 0 (off, the default) or 4 ... 32; 0 < min_amp <= 1 (0.015); 1 <= ratio <= 1e6
 *   (4); 1 <= twist <= 1e6 (16); 0 < share <= 1 (0.5); on_frames, off_frames 1 ... 16 (2, 2).  RDSP_ERR_INVALID otherwise (a NaN
 *   fails), nothing changed.  With K = 4 a frame is 11.6 ms: 40 ms of tone and 40 ms of pause always hold two whole frames each.
 * - rdsp_engine_read_dtmf copies the last call's four records, [ch][n_blocks] with the given strides (elements), into DEVICE
 *   buffers, stream-ordered; any pointer may be NULL.  RDSP_ERR_NOT_READY before rdsp_engine_enable_dtmf; RDSP_ERR_INVALID for
 *   n_blocks negative or above the last call's, a stride below n_blocks.
 * - rdsp_engine_read_dtmf_digits copies n_digits (d_count, [n_channels]) and the 16 ring words (d_ring, [n_channels][16]) of
 *   channels first_channel ... into DEVICE buffers, stream-ordered; either pointer may be NULL: a caller who polls rarely still
 *   gets the last 16 keys with their block stamps.  RDSP_ERR_INVALID for a range outside the object.
 * - rdsp_engine_dtmf_key(sym), host only: the key's character, 0 for anything above 15.
 * - rdsp_engine_dtmf_gain(hz, tau_us), host only, in double: what the boxcar of 4 samples and the de-emphasis leave of a sine,
 *   |sin(4 pi hz / 44100) / (4 sin(pi hz / 44100))| x rdsp_engine_tone_gain(hz, tau_us); 0.0 for what that refuses. */
int rdsp_engine_enable_dtmf(rdsp_engine_t *e);
int rdsp_engine_dtmf_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_dtmf(rdsp_engine_t *e, int K, float min_amp, float ratio, float twist, float share, int on_frames, int off_frames);
int rdsp_engine_read_dtmf(rdsp_engine_t *e, int n_blocks, uint8_t *d_key, size_t key_stride, uint8_t *d_new, size_t new_stride, float *d_lo,
                          size_t lo_stride, float *d_hi, size_t hi_stride, void *stream);
int rdsp_engine_read_dtmf_digits(rdsp_engine_t *e, int first_channel, int n_channels, uint32_t *d_count, uint32_t *d_ring, void *stream);
char rdsp_engine_dtmf_key(int sym);
double rdsp_engine_dtmf_gain(float hz, float tau_us);
/* AFSK 1200 packet decoder.  Of the signalling inside the voice band, Bell 202 AFSK at 1200 baud is the one that carries data:
 * AX.25 (APRS, packet BBS traffic, telemetry).  After rdsp_engine_enable_afsk(e) every NFM group with the decoder on runs one
 * more kernel behind its other detector kernels.  It only measures: it reads the "demod" tap and writes its own records and
 * state words, among them a ring of the last four frames whose frame check sequence held.  An engine that never calls the enable
 * allocates, launches, returns and saves what it did before.  The arithmetic is csrc/rdsp_afsk.h's (compiled with
 * -ffp-contract=off, the fused operations written as fmaf); its plain loop afsk_reference IS this definition.  a[n] is the
 * receiver's "demod" tap, in blocks of 128 samples counted from the detector's start.
 *   1. Decimation by 4.  d[m] = (a0 + a1) + (a2 + a3) over samples 4 m ... 4 m + 3: 32 samples a block at 11 025 Hz, 9.1875 a
 *      bit.  m = 32 t_blocks + r as uint32 (t_blocks: the blocks before this one); d is 0 before the start.
 *   2. Two correlators.  dphi_f = llround(f 2^32 4 / 44100) for f = 1200 (mark) and 2200 (space); (c, s) = tune_phasor(tab,
 *      m dphi_f); p_f[m] = (d c, d s), two rounded products.  Over a window of 12 samples S_f[m] = sum of p_f[m - 11 ... m], each
 *      component as (q0 + q1) + q2, q_i = (t0 + t1) + (t2 + t3) of terms 4 i ... 4 i + 3, oldest first; recomputed for every m.
 *      P_f = fmaf(S.x, S.x, S.y S.y); gp = g P_space (space_gain, rounded on its own); raw[m] = P_mark - gp > 0.
 *   3. Bit clock, integers only.  step = llround(2^32 1200 4 / 44100).  For each m: (a) raw != prev_raw: pll = (int32) pll -
 *      ((int32) pll >> pull), an arithmetic shift, and prev_raw = raw; (b) old = pll, pll += step (uint32); (int32) old >= 0 and
 *      (int32) pll < 0: a bit is sampled, bit = (raw == prev_sampled) (NRZI), prev_sampled = raw.
 *   4. HDLC, per sampled bit.  A one: ones = min(ones + 1, 7); ones >= 7 leaves the frame (inframe = 0), else inside a frame the
 *      bit is set in `byte` at nb, nb += 1.  A zero: behind six ones it is a flag's end -- inside a frame with nb == 7 and nbytes
 *      >= min_bytes the frame is emitted if its FCS holds (the running CRC-16/X-25, reflected 0x8408 from 0xFFFF, equals the
 *      residue 0xF0B8), else n_bad and the block's `bad` count it; either way a frame begins: inframe = 1, nbytes = byte = nb = 0,
 *      crc = 0xFFFF -- behind five ones it is a stuffed bit and dropped, else inside a frame nb += 1; then ones = 0.  Then
 *      inframe and nb == 8: buf[nbytes++] = byte, the crc takes the byte, byte = nb = 0, and nbytes > 330 leaves the frame.
 *   5. Emit.  ring[n_frames mod 4] = { len = nbytes - 2, t_blocks (the blocks since the detector's start, the one the flag ended
 *      in included), the len bytes packed little-endian into 82 words, the rest 0 }; n_frames += 1.
 *   6. Records after block b of a call, each [ch][max_blocks]: sync_rec = inframe, new_rec and bad_rec = the frames emitted and
 *      refused in the block (uint8), lvl_rec = the sum over the block's 32 m of P_mark + gp, by the pairwise tree over r, times
 *      (float)(1 / (32 24^2)): about A^2 of a present tone of amplitude A (before the boxcar's and the de-emphasis's gain).
 *      Receivers the kernel did not run on read zeros.
 *   7. Everything is a function of whole blocks counted from the detector's start: a stream gives the same bits however it is
 *      cut into calls.
 * State: 448 words a channel (rdsp_afsk.h: on, pll, prev_raw, prev_sampled, ones, inframe, byte, nb, nbytes, crc, n_frames,
 * n_bad, t_blocks, three zeros; the last 11 d and a zero; buf, 84 words; the ring, 4 x 84 words).  A stored `on` that differs
 * from the one the channel is run with, or the group's pending FM reset, starts the detector from zeros; a change of space_gain,
 * pull or min_bytes does not.  The words are zeroed by rdsp_engine_reset, maintained only for NFM groups with the decoder on
 * (an NFM group with it off has its channels' words zeroed in the stream, a group outside NFM leaves them alone), stay with the
 * channel through rdsp_engine_set_groups, and travel as a tenth optional part of the state blob (header flag 512): an engine
 * without the decoder writes the blob it always wrote and refuses one that carries the part (RDSP_ERR_NOT_READY); a blob
 * without the part zeroes the words.
 * - rdsp_engine_enable_afsk works as rdsp_engine_enable_dtmf does: no stream, waits for the device, RDSP_ERR_NOT_READY before
 *   rdsp_engine_enable_fm, RDSP_ERR_NOMEM with the object unchanged, again a no-op.
 * - rdsp_engine_set_afsk(e, on, space_gain, pull, min_bytes): settings of the selected group(s), copied by a new group, kept by
 *   reset, in no blob.  on 0 (the default) or 1; 1/16 <= space_gain <= 16 (1.0: a transmitter that pre-emphasises, the usual
 *   case, arrives level behind the de-emphasis); pull 1 ... 4 (2); min_bytes 9 ... 330 (17: two addresses, control, FCS).
 *   RDSP_ERR_INVALID otherwise (a NaN fails), nothing changed.
 * - rdsp_engine_read_afsk copies the last call's four records, [ch][n_blocks] with the given strides (elements), into DEVICE
 *   buffers, stream-ordered; any pointer may be NULL.  RDSP_ERR_NOT_READY before rdsp_engine_enable_afsk; RDSP_ERR_INVALID for
 *   n_blocks negative or above the last call's, a stride below n_blocks.
 * - rdsp_engine_read_afsk_frames copies n_frames (d_count, [n_channels]) and the ring (d_ring, [n_channels][4][84]) of channels
 *   first_channel ... into DEVICE buffers, stream-ordered; either pointer may be NULL.  RDSP_ERR_INVALID for a range outside the
 *   object.
 * - rdsp_engine_afsk_space_gain(tau_us), host only, in double: (rdsp_engine_dtmf_gain(1200, tau_us) / rdsp_engine_dtmf_gain(2200,
 *   tau_us))^2, the space_gain for a flat (not pre-emphasised) sender; 0.0 for a tau_us that refuses.
 * - rdsp_engine_afsk_fcs(bytes, n), host only: the X-25 frame check sequence AX.25 appends, low byte first. */
int rdsp_engine_enable_afsk(rdsp_engine_t *e);
int rdsp_engine_afsk_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_afsk(rdsp_engine_t *e, int on, float space_gain, int pull, int min_bytes);
int rdsp_engine_read_afsk(rdsp_engine_t *e, int n_blocks, uint8_t *d_sync, size_t sync_stride, uint8_t *d_new, size_t new_stride, uint8_t *d_bad,
                          size_t bad_stride, float *d_lvl, size_t lvl_stride, void *stream);
int rdsp_engine_read_afsk_frames(rdsp_engine_t *e, int first_channel, int n_channels, uint32_t *d_count, uint32_t *d_ring, void *stream);
double rdsp_engine_afsk_space_gain(float tau_us);
uint32_t rdsp_engine_afsk_fcs(const uint8_t *bytes, size_t n);
/* POCSAG pager decoder.  The other large class of traffic on the VHF/UHF bands is not audio: POCSAG paging is direct NRZ FSK
 * at 512, 1200 or 2400 baud on the discriminator's output.  After rdsp_engine_enable_pocsag(e) every NFM group whose baud is not
 * 0 runs one more kernel behind its other detector kernels.  It only measures: it reads the "demod" tap and writes its own
 * records and state words, among them a ring of the last four messages.  An engine that never calls the enable allocates,
 * launches, returns and saves what it did before.  The arithmetic is csrc/rdsp_pocsag.h's (compiled with -ffp-contract=off); its
 * plain loop pocsag_reference IS this definition.  a[n] is the receiver's "demod" tap, in blocks of 128 samples counted from the
 * detector's start.  Set a paging channel with rdsp_engine_set_fm(e, 2, 7500, 0): the usual +-4.5 kHz shift then reads +-0.6,
 * away from the clip at +-1, and no de-emphasis smears the NRZ (the decoder does not refuse one).
 *   1. Decimation by 4.  d[m] = (a0 + a1) + (a2 + a3) over samples 4 m ... 4 m + 3: 32 samples a block at 11 025 Hz, 21.53,
 *      9.19 and 4.59 a bit at 512, 1200 and 2400 baud; d is 0 before the start.
 *   2. Matched filter.  S[m] = the sum of d[m - W + 1 ... m], W = 20, 8 or 4, as q_i = (t0 + t1) + (t2 + t3) of terms 4 i ...
 *      4 i + 3, oldest first, folded from the left, ((q0 + q1) + q2) + ...; recomputed for every m, no running sum.
 *      raw[m] = S[m] < 0: POCSAG's 1 is the lower frequency.
 *   3. Bit clock, integers only, the AFSK decoder's.  step = llround(baud 2^32 4 / 44100).  For each m: (a) raw != prev_raw:
 *      pll = (int32) pll - ((int32) pll >> pull) and prev_raw = raw; (b) old = pll, pll += step (uint32); (int32) old >= 0 and
 *      (int32) pll < 0: the bit raw is sampled.
 *   4. Framing, per sampled bit.  sr = sr << 1 | bit (32 bits).  Hunting: popcount(sr ^ 0x7CD215D8) <= sync_errs goes in sync
 *      with polarity 0 (allowed by invert 0 and 2, tested first), the same test on ~sr with polarity 1 (invert 1 and 2); nbits =
 *      ncw = 0.  In sync: every 32nd bit closes a word, sr read through the polarity.  Words 0 ... 15 are codewords (5, 6); the
 *      17th must match the sync word within sync_errs at the latched polarity and starts the next batch; if it does not, the
 *      open message is closed with the flag `cut` and the machine hunts again from the next bit.
 *   5. Codeword.  pocsag_syndrome = the remainder of bits 31 ... 1 by x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1 (0x769); the error
 *      pattern is the one of weight <= 2 on those 31 bits with that syndrome (496 patterns; none: uncorrectable); an odd parity
 *      of the corrected 32 bits counts one more error, in bit 0.  With ne errors the corrected word is accepted iff ne <= (its
 *      bit 31 ? fix_data : fix_addr); a word not accepted is uncorrectable.
 *   6. Messages.  An accepted idle word (0x7A89C197) closes the open message; another accepted address word (bit 31 clear)
 *      closes it and opens a new one, address = bits 30 ... 13 << 3 | codeword index >> 1, function = bits 12 ... 11; an accepted
 *      message word (bit 31 set) is appended to the open message as 20 data bits (30 ... 11) | ne << 24, ignored if none is
 *      open; an uncorrectable word counts in n_bad and the block's `bad`, and is appended to an open message as received, bits
 *      30 ... 11 | 1 << 31.  A message holds 80 words; more are dropped and the message is flagged truncated.
 *   7. Ring.  A closed message goes to ring[n_msgs mod 4], n_msgs += 1.  A slot is 84 words: n_cw | flags << 8 | polarity << 16;
 *      t_blocks (the blocks since the detector's start, the one it closed in included); address | function << 21; corrected
 *      bits (the address word's among them) | uncorrectable words << 16; the n_cw words, the rest 0.  flags: 1 cut, 2
 *      truncated, 4 holds an uncorrectable word.
 *   8. Records after block b of a call, each [ch][max_blocks]: sync_rec = in sync, new_rec = messages closed in the block,
 *      bad_rec = uncorrectable codewords in the block, saturating at 255 (uint8), lvl_rec = the pairwise tree over the block's
 *      32 |S[m]| times (float)(1 / (32 4 W)), about the amplitude of a present signal, dc_rec = the tree over the block's d[m]
 *      times 1/128: the block's mean, the receiver's frequency offset in units of the deviation.  Receivers the kernel did not
 *      run on read zeros.
 *   9. Everything is a function of whole blocks counted from the detector's start: a stream gives the same bits however it is
 *      cut into calls.
 * State: 456 words a channel (rdsp_pocsag.h: baud, pll, prev_raw, sr, insync, pol, nbits, ncw, open, the open message's n_cw,
 * flags, address word and counts, n_msgs, n_bad, t_blocks; the last 19 d and a zero; the open message, four zeros and 80 words
 * (those of messages closed before are left in place); the ring, 4 x 84 words).  A stored baud that differs from the one the
 * channel is run with, or the group's pending FM reset, starts the detector from zeros; a change of the other settings does
 * not.  The words are zeroed by rdsp_engine_reset, maintained only for NFM groups with a baud (an NFM group with baud 0 has its
 * channels' words zeroed in the stream, a group outside NFM leaves them alone), stay with the channel through
 * rdsp_engine_set_groups, and travel as an eleventh optional part of the state blob (header flag 1024): an engine without the
 * decoder writes the blob it always wrote and refuses one that carries the part (RDSP_ERR_NOT_READY); a blob without the part
 * zeroes the words.
 * - rdsp_engine_enable_pocsag works as rdsp_engine_enable_afsk does: no stream, waits for the device, RDSP_ERR_NOT_READY before
 *   rdsp_engine_enable_fm, RDSP_ERR_NOMEM with the object unchanged, again a no-op.
 * - rdsp_engine_set_pocsag(e, baud, invert, pull, sync_errs, fix_addr, fix_data): settings of the selected group(s), copied by a
 *   new group, kept by reset, in no blob.  baud 0 (the default: off), 512, 1200 or 2400; invert 0, 1 or 2 (2); pull 1 ... 4 (3);
 *   sync_errs 0 ... 3 (2); fix_addr 0 ... 2 (1: in noise two-bit correction accepts a quarter of all random words as
 *   addresses); fix_data 0 ... 2 (2).  RDSP_ERR_INVALID otherwise, nothing changed.
 * - rdsp_engine_read_pocsag copies the last call's five records, [ch][n_blocks] with the given strides (elements), into DEVICE
 *   buffers, stream-ordered; any pointer may be NULL.  RDSP_ERR_NOT_READY before rdsp_engine_enable_pocsag; RDSP_ERR_INVALID for
 *   n_blocks negative or above the last call's, a stride below n_blocks.
 * - rdsp_engine_read_pocsag_messages copies n_msgs (d_count, [n_channels]) and the ring (d_ring, [n_channels][4][84]) of
 *   channels first_channel ... into DEVICE buffers, stream-ordered; either pointer may be NULL.  RDSP_ERR_INVALID for a range
 *   outside the object.
 * - rdsp_engine_pocsag_bch_table(), host only: 1024 entries by syndrome, b1 | b2 << 5 | ne << 10 (b: the word's bit 1 ... 31 to
 *   flip, 0 for none), 0xFFFF where no pattern of weight <= 2 has the syndrome.
 * - rdsp_engine_pocsag_codeword(data21), host only: the 21 data bits, their BCH(31,21) remainder and the even parity bit. */
int rdsp_engine_enable_pocsag(rdsp_engine_t *e);
int rdsp_engine_pocsag_enabled(const rdsp_engine_t *e);
int rdsp_engine_set_pocsag(rdsp_engine_t *e, int baud, int invert, int pull, int sync_errs, int fix_addr, int fix_data);
int rdsp_engine_read_pocsag(rdsp_engine_t *e, int n_blocks, uint8_t *d_sync, size_t sync_stride, uint8_t *d_new, size_t new_stride, uint8_t *d_bad,
                            size_t bad_stride, float *d_lvl, size_t lvl_stride, float *d_dc, size_t dc_stride, void *stream);
int rdsp_engine_read_pocsag_messages(rdsp_engine_t *e, int first_channel, int n_channels, uint32_t *d_count, uint32_t *d_ring, void *stream);
const uint16_t *rdsp_engine_pocsag_bch_table(void);
uint32_t rdsp_engine_pocsag_codeword(uint32_t data21);
/* Decoder events.  The three decoders above each keep a ring of results per receiver: 16 digits, 4 frames, 4 messages.  Their
 * read-outs are dense -- every channel's count and whole ring -- and say nothing of which items are new.
 * rdsp_engine_gather_events gathers, after an update, the items that update emitted into dense payload words with one record
 * each: on the device, without atomics, the same bytes every time.  It is opt-in by being called: an engine that never calls it
 * allocates, launches, returns and saves exactly what it does without.  It only reads the decoders' words and records.  The
 * plain loop events_reference of csrc/rdsp_events.h IS the definition; it is exported as rdsp_events_reference.
 *
 * 1. Kinds.  RDSP_EVENT_DTMF 0, RDSP_EVENT_AFSK 1, RDSP_EVENT_POCSAG 2.  A kind whose decoder is not enabled contributes
 *    nothing.
 * 2. Which items are new, per channel ch and kind.  Take the kind's record `new` of the last update exactly as the kind's read
 *    call (rdsp_engine_read_dtmf / _afsk / _pocsag) returns it for all of that update's blocks: receivers the decoder did not
 *    run on read 255 (DTMF) or 0 (AFSK, POCSAG), whatever the engine's buffers still hold of an earlier call.
 *      c = the count of blocks with new != 255 (DTMF), the sum of new (AFSK, POCSAG)
 *      n = the detector's count word: n_digits, n_frames, n_msgs;  R = the ring's size: 16, 4, 4
 *      take = min(c, R), lost = c - take
 *    The items are those with seq = n - take ... n - 1 (uint32), oldest first, item seq in ring slot seq mod R.  By the decoders'
 *    definitions c <= n holds behind every update (a detector that starts from zeros does so at the start of its launch).  Where
 *    it does not hold take is n, so a violated premise can misreport but never names an item the ring cannot have; lost stays
 *    c - min(c, R).
 * 3. Payload.  The used part of the item's slot, copied verbatim:
 *      DTMF    the ring word (sym | t_blocks << 8)                                        n_words = 1
 *      AFSK    slot words 0 ... 1 + ceil(len / 4) (len, t_blocks, the bytes)              n_words = 2 + (min(len, 328) + 3) / 4 <= 84
 *      POCSAG  slot words 0 ... 3 + n_cw (the four header words, then the words)          n_words = 4 + min(n_cw, 80) <= 84
 * 4. Sequence.  The events run by channel ascending, then kind ascending, then seq ascending.  needed_events is the sequence's
 *    length, needed_words the sum of its n_words, lost the sum of lost over channels and kinds.
 * 5. Output.  rdsp_event_record_t = {int32 channel; uint32 kind | n_words << 8; uint32 seq; uint32 offset}, offset the index of
 *    the payload's first word in d_words: the sum of n_words of all earlier events.  written_events is the length of the longest
 *    prefix of the sequence whose events k have k < capacity_events and offset_k + n_words_k <= capacity_words; written_words is
 *    the offset of the first event behind that prefix (needed_words when there is none).  The records and payloads of the
 *    prefix are written; nothing at or behind written_events in d_records, or at or behind written_words in d_words, is.
 *    d_counts[5] = {needed_events, written_events, needed_words, written_words, lost}, on the device.
 * 6. The call.  Stream-ordered behind the last update.  A sizing call is allowed: both capacities 0, both buffers NULL.  The call
 *    is repeatable, with another capacity too, and modifies nothing of the engine but its own scratch (16 + 3 bytes a channel),
 *    which its first call allocates: if that fails it returns RDSP_ERR_NOMEM and the engine is as it was.
 * 7. When the counts are all 0.  No update made yet; the last update had 0 blocks (or failed); and behind rdsp_engine_reset or
 *    rdsp_engine_load_state until the next update -- the words then no longer belong to the last call's records.  A host flag
 *    set by the update and cleared by those calls does this.  No other host call touches the detector words between updates:
 *    rdsp_engine_set_groups and the setters take effect in the next update, whose kernels zero or restart a detector at their
 *    start, and a decoder enabled between updates has no rows in the last call, so it contributes nothing.
 * 8. Refusals.  RDSP_ERR_NOT_READY with none of the three decoders enabled.  RDSP_ERR_INVALID, nothing written: d_counts NULL; a
 *    capacity above 0 with a NULL buffer; d_records or d_words not 16-byte aligned; a capacity above INT32_MAX; n_channels x 688
 *    above INT32_MAX (688 = 16 + 4 x 84 + 4 x 84 words, the most a channel contributes: every sum fits an int32).
 * 9. rdsp_events_reference, host only, is events_reference on host arrays: the three `new` records [n_channels][new_stride] and
 *    the three detector-word arrays [n_channels][168 / 448 / 456], a kind off where either of its two is NULL; the same refusals
 *    but for the alignment, and new_stride >= n_blocks >= 0.  It returns the number of (channel, kind) pairs with c > n -- 0
 *    behind every update -- or RDSP_ERR_INVALID. */
enum { RDSP_EVENT_DTMF = 0, RDSP_EVENT_AFSK = 1, RDSP_EVENT_POCSAG = 2 };
typedef struct {
  int32_t channel;
  uint32_t kind_words; /* kind | n_words << 8 */
  uint32_t seq, offset;
} rdsp_event_record_t;
int rdsp_engine_gather_events(rdsp_engine_t *e, rdsp_event_record_t *d_records, size_t capacity_events, uint32_t *d_words, size_t capacity_words,
                              int32_t *d_counts, void *stream);
int rdsp_events_reference(const uint8_t *new_dtmf, const uint8_t *new_afsk, const uint8_t *new_pocsag, size_t new_stride, const uint32_t *dtmf_words,
                          const uint32_t *afsk_words, const uint32_t *pocsag_words, int n_channels, int n_blocks, rdsp_event_record_t *records,
                          size_t capacity_events, uint32_t *words, size_t capacity_words, int32_t *counts);
/* Receiver groups.  The sketch has one receiver -- one mode, one audio filter, one AGC setting; an object of many
 * channels can be cut into groups of CONSECUTIVE channels that each carry their own settings.  first_channel[g] is group
 * g's first channel (ascending, first_channel[0] = 0; a new group starts as a copy of the group its first channel was in).
 * The setters above address the group chosen with rdsp_engine_select_group (-1, the default: every group);
 * rdsp_engine_setDemodMode returns the offset of the selected group (of group 0 for -1).  Regrouping in mid-stream:
 * - a new group's settings are copied from the old group its first channel was in;
 * - signal state stays with the channel (filters, oscillator, AGC, side-band lines, blanker, ALS): a channel continues as
 *   it would have in its old group with the new group's settings from the next update on; so do its station and tuning
 *   phase (rdsp_engine_update_sources below), and its step follows the new group's mode from the next call on;
 * - pending resets (setDemodMode / setAudioFilter / enableALSfilter made since the last update) are settings too: a new
 *   group whose channels come from old groups with different pending resets is refused (RDSP_ERR_UNSUPPORTED, "call
 *   rdsp_engine_update first") and nothing changes;
 * - the call takes no stream: before it moves a channel's side-band lines it waits for everything queued on the engine's
 *   device, and the lines have moved when it returns. */
int rdsp_engine_set_groups(rdsp_engine_t *e, int n_groups, const int *first_channel);
int rdsp_engine_groups(const rdsp_engine_t *e);
int rdsp_engine_select_group(rdsp_engine_t *e, int group);
/* The signal state of a channel range as data (resume; receivers moved between objects or GPUs): filter states, oscillator
 * and detector scalars, AGC, the last 512 samples of the side-band network's lines in time order (independent of either
 * object's ring size), blanker and ALS lines and taps.  Settings are not part of it.  A loaded range continues bit for bit. */
size_t rdsp_engine_state_bytes(const rdsp_engine_t *e, int n_channels);
int rdsp_engine_save_state(rdsp_engine_t *e, int first_channel, int n_channels, void *host_buf, size_t bytes, void *stream);
int rdsp_engine_load_state(rdsp_engine_t *e, int first_channel, const void *host_buf, size_t bytes, void *stream);
int rdsp_engine_channels(const rdsp_engine_t *e);
int rdsp_engine_device(const rdsp_engine_t *e);
int rdsp_engine_max_blocks(const rdsp_engine_t *e);
/* [n_channels][8]: oscillator phase, AGC gain, AGC envelope, hang counter, AGC-active flag, PLL frequency estimate (Hz),
 * PLL lock flag, blanker-hit flag */
int rdsp_engine_get_scalars(rdsp_engine_t *e, float *host_out, void *stream);
const float *rdsp_engine_agc_curve(const rdsp_engine_t *e); /* host copy, 130 entries (the engine uses 129) */
const float *rdsp_engine_sine_table(const rdsp_engine_t *e); /* host copy, 257 entries */

/* ---- `AudioSDRpreProcessor preProcessor;` (INO:53; wired INO:71-72) as the reference's engine library computes it -------
 * (image ::update 0xee88): finds and repairs a one-sample slip between the rails with a 128-point FFT per block while
 * detection is on, and swaps the rails on request.  The chain's own rdsp_pre_* calls above are a different mechanism
 * (a slip set by the host, an estimator on a recording); this object is the reference's. */
typedef struct rdsp_preproc rdsp_preproc_t;
int rdsp_preproc_create(int n_channels, int device, rdsp_preproc_t **out);
void rdsp_preproc_destroy(rdsp_preproc_t *p);
int rdsp_preproc_startAutoI2SerrorDetection(rdsp_preproc_t *p); /* INO:117; takes effect at the next update */
int rdsp_preproc_swapIQ(rdsp_preproc_t *p, int on);             /* INO:118 */
int rdsp_preproc_reset(rdsp_preproc_t *p, void *stream); /* state as constructed (not detecting); swapIQ kept, a pending start dropped */
int rdsp_preproc_update(rdsp_preproc_t *p, const int16_t *d_iq, size_t in_stride, int n_blocks, int16_t *d_out,
                        size_t out_stride, void *stream);      /* [ch][t] int16 pairs (I, Q) in and out; in place allowed */
int rdsp_preproc_get_state(rdsp_preproc_t *p, int16_t *host_out, void *stream); /* [ch][4]: remedy (0, 1 = I later, -1 = Q later), bad count, counted blocks, detecting */
int rdsp_preproc_channels(const rdsp_preproc_t *p);
int rdsp_preproc_device(const rdsp_preproc_t *p);

/* the two objects as nodes of the block graph (two inputs I / Q, two outputs, one block per tick): INO:71-72, :81-86 */
rdsp_node_t *rdsp_preproc_node_create(rdsp_graph_t *g, rdsp_preproc_t *p);
rdsp_node_t *rdsp_engine_node_create(rdsp_graph_t *g, rdsp_engine_t *e);
int rdsp_engine_node_status(rdsp_node_t *n); /* either kind */

/* The sketch as shipped inside ONE chain: a chain created as the bare CONV stage (decim 1, 44.1 kHz, RDSP_DEMOD_IQ, no
 * mixer offset, unit gains, AGC / ALS / spectral stage off -- what loop() runs, INO:198) takes the reference's own
 * pre-processor and engine in front of it.  rdsp_chain_process then is INO:71-86 + :198 (preProcessor -> SDR ->
 * doConvolutionalProcessing), rdsp_sdr_node_create wires exactly that into the graph, and the rdsp_sdr_* / rdsp_pre_*
 * setters above reach rdsp_engine_t / rdsp_preproc_t (the image's arithmetic) instead of this build's stand-ins; mode and
 * filter arguments stay rdsp_demod_t / rdsp_audio_filter_t and are translated to the engine's numbers.  Switching on is
 * refused (RDSP_ERR_UNSUPPORTED) while the chain's own stand-ins are on -- rdsp_sdr_enableNoiseBlanker, rdsp_pre_swapIQ(1),
 * a non-zero rdsp_pre_setIQslip -- since those setters reach the engine's objects afterwards and could not turn them off:
 * turn them off first, make the calls again after the switch.  rdsp_chain_reset resets both objects;
 * rdsp_chain_save_state / load_state are refused (see there). */
int rdsp_sdr_set_engine_literal(rdsp_chain_t *c, int on);
int rdsp_sdr_load_engine_tables(rdsp_chain_t *c, const float *biquad_sets15x20, const float *hilbert64);
rdsp_engine_t *rdsp_chain_engine(rdsp_chain_t *c);   /* the objects themselves (NULL unless engine-literal) */
rdsp_preproc_t *rdsp_chain_preproc(rdsp_chain_t *c);

#ifdef __cplusplus
}
#endif
#endif
