// spec_image_core.h -- the sample arithmetic of dspfft_execute_spec_u8 / dspfft_execute_ispec_u8 (include/dspfft.h): spec's display encoding
// with its 8-bit store (spec/spec.c:81-139 and the writer's clamp(lround(255 e))) and ispec's 8-bit load with its decoding
// (spec/ispec.c:84-151), one function per sample.  Shared by the HIP kernels (spec_image.hip) and the CPU tests, which compile it with g++.
//
// Every line restates pointwise.hip's spec_divisors / spec_encode_one / ispec_decode_kernel / ispec_signmap_kernel and backend_hip.hip's
// u8_to_f32_kernel / f32_to_u8_kernel operation for operation: the fused calls give the bytes of the five-step composition, not bytes
// close to them.  Scalar math follows the reference's `intermediate` = double.
//
// Log scale evaluates libm's double log1p once per sample, as dspfft_spec_encode does.  A single-precision evaluation that decides the byte
// away from rounding boundaries (motion_filter.h's motion_store_u8_fast) is NOT built here: the divisor differs per channel and per image, so
// the written bound would have to hold for every (gain, range) pair a caller can pass, and the sweep is one of three in a call whose other
// two are transforms.  Its measured cost is in profiles/r12_spec_u8.txt.
#pragma once
#include <math.h>
#include <stdint.h>
#include "elementwise_core.h"

namespace dspfft {

enum { SPEC_RANGE_ONE = 0, SPEC_RANGE_DC = 1, SPEC_RANGE_DCS = 2 };
enum { SPEC_SCALE_LOG = 0, SPEC_SCALE_LINEAR = 1 };
enum { SPEC_SIGN_ABS = 0, SPEC_SIGN_SHIFT = 1, SPEC_SIGN_SATURATE = 2, SPEC_SIGN_RETAIN = 3 };
enum { SPEC_IMAGE_MAX_CH = 4 };       // what the decode handles (dspfft_ispec_decode's limit); both calls refuse more

// spec.c:92-110 (+ :115): the divisor of every channel from the first pixel's (uniform-range) coefficients f[0 .. d), as `coeff` = float
DSP_HD void spec_image_divisors(float *m, const float *f, int d, double gain, int rangetype, int scaletype)
{
	if (rangetype == SPEC_RANGE_ONE) for (int z = 0; z < d; z++) m[z] = (float)gain;
	else if (rangetype == SPEC_RANGE_DC) {
		float best = (float)(f[0] * gain);
		for (int z = 1; z < d; z++) { const float v = (float)(f[z] * gain); if (v > best) best = v; }
		for (int z = 0; z < d; z++) m[z] = best;
	} else for (int z = 0; z < d; z++) m[z] = (float)(f[z] * gain);
	if (scaletype == SPEC_SCALE_LOG) for (int z = 0; z < d; z++) m[z] = (float)(double)log1pf(m[z]);
}
// spec.c:88-136 for one sample: the float the spectrogram image holds.  first: the sample belongs to the first pixel (:135 leaves it alone)
DSP_HD float spec_image_encode(float fi, bool first, float m, double gain, int scaletype, int signtype)
{
	float v = (float)(fi * gain);
	if (scaletype == SPEC_SCALE_LOG) v = (float)(copysign(log1p((double)fabsf(v)), (double)v) / m);
	else v = v / m;
	if (signtype == SPEC_SIGN_ABS) v = fabsf(v);
	else if (signtype == SPEC_SIGN_SHIFT) v = (float)(((double)v / 2. + 0.5) * 254 / 255);
	else if (signtype == SPEC_SIGN_SATURATE) { if (!first) v = !signbit(v); }
	return v;
}
// the 8-bit writer: clamp(lround(255 e)), as dspfft_f32_to_u8 with mul = 255
DSP_HD uint8_t spec_image_byte(float e) { return quantise_u8((double)e * 255.0); }
// the `sign` preset's byte (spec.h:75: linear, saturate, range one, custom gain 1): the encoded float is f itself in the first pixel and
// !signbit(f) everywhere else -- the sign map ispec -m reads
DSP_HD uint8_t spec_image_sign_byte(float fi, bool first) { return first ? spec_image_byte(fi) : (uint8_t)(signbit(fi) ? 0 : 255); }

// ispec.c:118-139: max[] from the spectrogram's DC values, as dspfft_ispec_decode builds it on the host (max[] is `coeff`; log1p in double)
inline void spec_image_decode_max(double *mx, const double *dc, int d, double gain, int rangetype, int scaletype)
{
	float m[SPEC_IMAGE_MAX_CH];
	if (rangetype == SPEC_RANGE_ONE) for (int z = 0; z < d; z++) m[z] = (float)gain;
	else if (rangetype == SPEC_RANGE_DC) {
		float best = (float)(dc[0] * gain);
		for (int z = 1; z < d; z++) if (dc[z] * gain > best) best = (float)(dc[z] * gain);
		for (int z = 0; z < d; z++) m[z] = best;
	} else for (int z = 0; z < d; z++) m[z] = (float)(dc[z] * gain);
	for (int z = 0; z < d; z++) mx[z] = scaletype == SPEC_SCALE_LOG ? (double)(float)log1p((double)m[z]) : (double)m[z];
}
// ispec.c:84-151 for one sample: the byte as the reader hands it over, the companion sign map (:91-95; has_map), unsign, unscale, / gain
// and the DC restore (:161-163; `dc` is consulted for the first pixel only)
DSP_HD float spec_image_decode(uint8_t byte, bool has_map, uint8_t map, bool first, double m, double gain, int scaletype, int signtype, bool restore_dc, double dc)
{
	float v = (float)((double)byte / 255.0);
	if (has_map && !first) v = copysignf(v, (float)((int)map - 128));
	if (signtype == SPEC_SIGN_SHIFT) v = (float)(((double)v * 255. / 254 - 0.5) * 2);
	else if (signtype == SPEC_SIGN_SATURATE) { if (!first) v = v * 2 - 1; }
	if (scaletype == SPEC_SCALE_LOG) v = (float)copysign(expm1((double)fabsf((float)(v * m))), (double)v);
	else v = (float)(v * m);
	v = (float)(v / gain);
	if (restore_dc && first) v = (float)dc;
	return v;
}

// one launch of each sweep (spec_image.hip; engine.cpp reaches the launchers through weak references)
struct SpecImageEnc {
	const float *f; uint8_t *out, *signmap; double *dc;      // signmap, dc: nullptr = not asked for
	uint64_t len; int d;
	double gain; int rangetype, scaletype, signtype;
};
struct SpecImageDec {
	const uint8_t *in, *signmap; float *f;                   // signmap: nullptr = none
	uint64_t len; int d;
	double gain, mx[SPEC_IMAGE_MAX_CH], dc[SPEC_IMAGE_MAX_CH];
	int scaletype, signtype, restore_dc;
};

// sample i of a sweep (what a lane does per sample; the CPU tests loop over it)
DSP_HD void spec_image_encode_at(const SpecImageEnc &a, const float *m, uint64_t i, int z, uint8_t &byte, uint8_t &sbyte)
{
	const float fi = a.f[i];
	const bool first = i < (uint64_t)a.d;
	byte = spec_image_byte(spec_image_encode(fi, first, m[z], a.gain, a.scaletype, a.signtype));
	sbyte = spec_image_sign_byte(fi, first);
}
DSP_HD float spec_image_decode_at(const SpecImageDec &a, uint64_t i, int z, uint8_t byte, uint8_t map)
{
	return spec_image_decode(byte, a.signmap != nullptr, map, i < (uint64_t)a.d, a.mx[z], a.gain, a.scaletype, a.signtype, a.restore_dc != 0, a.dc[z]);
}

}  // namespace dspfft
