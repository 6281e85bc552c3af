// scan_frame_core.h -- the per-pixel arithmetic of scan's output frame (scan/scan.c:366-375,389-404,429-441,461-491,508-526), shared by
// the HIP kernels (scan_frame.hip) and host code (engine.cpp's argument checks, the CPU tests compile it with g++).
//
// The frame is what scan hands to its encoder: AV_PIX_FMT_GBRPF32LE, three planes of W' = w (1 + visualize) by H' = h (1 + intermediates)
// floats in plane order G, B, R.  Panels: top-left the reconstruction `sum`, top-right every visited coefficient (1.0, or its spectrogram
// value with -s), bottom-left this frame's inverse plus DC (-i, normalised by 0..1 or by its own min / max with -M), bottom-right this
// frame's coefficients alone (-v -i).
//
// Types and operation order are the reference's with COEFF_PRECISION=F INTERMEDIATE_PRECISION=D; nothing may be contracted into an FMA
// (the product library is built with -ffp-contract=on), hence SF_NO_CONTRACT in every function below.
#pragma once
#include <math.h>
#include <stdint.h>
#include "radix.h"

#if defined(__clang__)
#define SF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SF_NO_CONTRACT
#endif

namespace dspfft {

// speclib.h:11-21 (keyed_enum: `none` is 0 and means the first case of spec_create's switch)
enum { SF_SCALE_NONE = 0, SF_SCALE_LINEAR = 1, SF_SCALE_LOG = 2 };
enum { SF_SIGN_NONE = 0, SF_SIGN_ABS = 1, SF_SIGN_SHIFT = 2, SF_SIGN_SATURATE = 3 };

// libavutil's comp[] table of the GBRP formats: R (z = 0) is plane 2, G plane 0, B plane 1
DSP_HD int sf_plane_of(int z) { return z == 0 ? 2 : z - 1; }

// element (x, y) of channel z in a frame of W' x H' planes; 64-bit (a full 8K frame with -v -i holds 398 M floats)
DSP_HD uint64_t sf_frame_offset(uint64_t fw, uint64_t fh, uint64_t x, uint64_t y, int z)
{
	return ((uint64_t)sf_plane_of(z) * fh + y) * fw + x;
}

// speclib.c:79-85 via speclib.h:48-49: spec_normalization(!!x + !!y)
DSP_HD double sf_normalization_2d(uint32_t x, uint32_t y)
{
	const int n = (x != 0) + (y != 0);
	return n == 0 ? 1.0 : n == 1 ? 1.41421356237309504880 : 2.0;      // (size_t)1 << 0 times M_SQRT2, 1 << 1
}

// speclib.c:104-106 (log) / :101-103 (linear)
DSP_HD double sf_scale(int scaletype, double c)
{
	SF_NO_CONTRACT
	return scaletype == SF_SCALE_LINEAR ? c : copysign(log1p(fabs(c)), c);
}
// speclib.c:110-127
DSP_HD double sf_sign(int signtype, double c)
{
	SF_NO_CONTRACT
	if (signtype == SF_SIGN_SHIFT) return (c / 2 + 0.5) * 254 / 255;
	if (signtype == SF_SIGN_SATURATE) return (double)!signbit(c);
	return fabs(c);
}

struct SfScaler { double gain, max; int scaletype, signtype; };
// scan.c:366-375 + speclib.c:129-160.  spec_create takes `coeff` (float) arguments: the gain (a double: 127.5 sqrt(4wh) or --spec-gain) and
// max * spec_normalization_2d(0,0) are rounded to float before max = scale(gain * max) is taken in double.  dc0..2: the DC pixel's channels.
DSP_HD SfScaler sf_scaler(int scaletype, int signtype, double gain, float dc0, float dc1, float dc2)
{
	SF_NO_CONTRACT
	float mx = dc0;
	if (dc1 > mx) mx = dc1;
	if (dc2 > mx) mx = dc2;
	SfScaler s;
	s.scaletype = scaletype; s.signtype = signtype;
	s.gain = (double)(float)gain;
	s.max = sf_scale(scaletype, s.gain * (double)(float)((double)mx * sf_normalization_2d(0, 0)));
	return s;
}
// the default gain, scan.c:367-368 (in double; spec_create then rounds it to float)
DSP_HD double sf_default_gain(uint32_t w, uint32_t h)
{
	SF_NO_CONTRACT
	return 127.5 * sqrt((double)((uint64_t)w * h * 4));
}
// scan.c:398-400 / :429-431: spec_scale(sp, c * normalization) = sign(scale(v * gain) / max), stored as float
DSP_HD float sf_spec_value(const SfScaler &s, float c, double norm)
{
	SF_NO_CONTRACT
	const double v = (double)c * norm;
	return (float)sf_sign(s.signtype, sf_scale(s.scaletype, v * s.gain) / s.max);
}
// the value a visited coefficient lights in the top-right panel (-v: 1.0, -s: the spectrogram value)
DSP_HD float sf_mark_value(bool spec, const SfScaler &s, float c, uint32_t x, uint32_t y)
{
	return spec ? sf_spec_value(s, c, sf_normalization_2d(x, y)) : 1.0f;
}

// scan.c:486: ((image + dc) - min) / (max - min), all float; without -M min = 0, max = 1
DSP_HD float sf_intermediate(float image, float dc, float mn, float mx)
{
	SF_NO_CONTRACT
	return ((image + dc) - mn) / (mx - mn);
}

// scan.c:508-526: true when the pixel has NOT reached parity.  depth < 32: lroundf(orig * s) != lroundf(sum * s), s = (float)(2^depth - 1)
// (a uint16_t in the reference); depth 32: the floats differ.  roundf rounds halves away from zero as lroundf does, so the two integers
// differ exactly when the rounded floats do (for finite products below 2^63, which 16-bit scales of pixel values are).
DSP_HD bool sf_parity_differs(float orig, float sum, int depth)
{
	SF_NO_CONTRACT
	if (depth >= 32) return orig != sum;
	const float s = (float)(uint16_t)((1u << depth) - 1);
	return roundf(orig * s) != roundf(sum * s);
}

// -M's min / max (scan.c:465-478): the reference keeps the FIRST element (raster order) among equal extremes, which only shows for +-0;
// a (value, index) pair with the lower index winning ties makes the reduction independent of the order its parts are combined in.
DSP_HD bool sf_min_wins(float a, uint64_t ia, float b, uint64_t ib) { return a < b || (a == b && ia < ib); }
DSP_HD bool sf_max_wins(float a, uint64_t ia, float b, uint64_t ib) { return a > b || (a == b && ia < ib); }

// device state of one dspfft_scanframes handle (scan_frame.hip)
struct SfState {
	double gain, max;                       // the scaler (begin)
	float mn[3], mx[3];                     // -M: this frame's min / max plus DC (compose)
	uint32_t reached;                       // -P: parity reached, later frames skip the comparison
	uint64_t parity_frame;                  // -P: the first frame at parity, UINT64_MAX while not reached
};

// one call of scan_frame.hip's launcher (engine.cpp reaches it through a weak reference)
enum { SF_OP_ALLOC, SF_OP_FREE, SF_OP_BEGIN, SF_OP_MARK_RANGE, SF_OP_MARK_COORDS, SF_OP_SAVE_COORDS, SF_OP_COMPOSE, SF_OP_PARITY };
struct SfOp {
	int op;
	uint32_t w, h;                          // image extent; the frame is w (1 + visualize) x h (1 + intermediates) per plane
	int visualize, spectrogram, intermediates, max_intermediates, parity_depth, scaletype, signtype;
	int trc;                                // COMPOSE: the transfer characteristic the left-hand panels are encoded with (trc_core.h), 0 none
	double gain;                            // spectrogram gain before spec_create's float rounding
	float *frame;
	const float *coeffs, *original;
	float *sum, *image;
	const uint32_t *owner, *lin;            // MARK_RANGE: owner index; MARK_COORDS / SAVE_COORDS: y*w+x list (0xFFFFFFFF slots skipped)
	uint64_t nslots;
	uint32_t lo, hi;                        // MARK_RANGE: light [lo, hi)
	uint32_t clo, chi;                      // MARK_RANGE: clear [clo, chi) in the bottom-right panel (unless also lit)
	int top, bottom;                        // write the top-right / bottom-right panel; MARK_COORDS with top = bottom = 0 writes 0 (clears)
	uint64_t frame_no;
	SfState *state;                         // ALLOC: receives both buffers; every other op: the handle's
	void *partials;
	uint32_t *flags;                        // -P: one per compose workgroup (this frame has a differing pixel there)
	uint32_t **saved;                       // SAVE_COORDS: the handle's copy of the last list, grown in place
	uint64_t *saved_cap;
	uint64_t *parity_out;                   // PARITY: host result
	void *stream;
};

}  // namespace dspfft
