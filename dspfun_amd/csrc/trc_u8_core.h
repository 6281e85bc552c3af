// trc_u8_core.h -- motion --linear on 8-BIT pixels (motion/motion.c:625,632-633 on load, :767-769,776 on store), folded into two tables.
// Shared by the HIP kernels (motion_ops.hip, motion_dither.hip), engine.cpp and the CPU tests, which compile it with g++.
//
//  * load: a byte k becomes ONE of 256 floats, lut[k] -- what the reference's default build (COEFF_PRECISION=F, INTERMEDIATE_PRECISION=L,
//    transfer functions double -> double) stores for it.  trc_u8_decode_lut evaluates the reference's own expression on the host, with the
//    host's long double and libm's pow.
//  * store: encode, clamp and lround together are a monotone step function of the linear value pel, so a byte is the number of steps at
//    or below pel: thr[k], k = 1..255, is the least double whose byte is >= k (thr[0] = -inf).  trc_u8_thresholds finds each by bisection
//    over the double's bit pattern, evaluating the reference's lines in double (the bar the 8-bit and dithered stores already meet).
//  * trc_u8_byte decides by comparisons with that table and by nothing else: the bytes are those of the host's exact evaluation, and the
//    device library's pow takes no part in them.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "elementwise_core.h"
#include "trc_core.h"

namespace dspfft {

// the two tables as they lie on the device: 3 KB
struct TrcU8Tab { double thr[256]; float lut[256]; };

// number of k >= 1 with pel >= thr[k]: eight comparisons.  NaN compares false everywhere: 0, as quantise_u8 gives on the device.
DSP_HD uint32_t trc_u8_byte(const double *thr, double pel)
{
	uint32_t k = 0;
#pragma unroll
	for (uint32_t step = 128; step; step >>= 1) if (pel >= thr[k + step]) k += step;
	return k;
}

// The same count from a guess: stepped up and down until thr[k] <= pel < thr[k + 1].  Any seed gives the same byte; a seed within one of it
// costs two or three table reads instead of eight dependent ones.
DSP_HD uint32_t trc_u8_byte_from(const double *thr, double pel, uint32_t seed)
{
	if (!(pel == pel)) return 0;
	uint32_t k = seed > 255u ? 255u : seed;
	while (k < 255u && pel >= thr[k + 1]) k++;
	while (k > 0u && !(pel >= thr[k])) k--;
	return k;
}

// A cheap single-precision estimate of the byte: only ever a seed for trc_u8_byte_from, so on the device the power is the bare v_log_f32 /
// v_exp_f32 pair (no denormal handling: a wrong guess costs table reads, never a byte); the host uses libm's.
DSP_HD float trc_u8_seed_pow(float x, float e)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(x) * e);
#else
	return exp2f(log2f(x) * e);
#endif
}
DSP_HD uint32_t trc_u8_seed(const TrcParams &p, double pel)
{
	const float L = (float)pel * (1.0f / 255.0f);
	float e;
	if (!(L > 0.f)) e = p.shape == 3 ? (L > -(float)p.b ? (float)p.slope * L : -1.f) : 0.f;
	else if (p.shape == 0) e = L;
	else if (p.shape != 1 && L < (float)p.b) e = (float)p.slope * L;
	else e = (float)p.a * trc_u8_seed_pow(L, (float)p.g_enc) - (float)(p.a - 1);
	const float b = e * 255.f + 0.5f;
	return b >= 255.f ? 255u : b > 0.f ? (uint32_t)b : 0u;
}

// ---- host side: the tables ----
// motion.c:625,633,637 for the bytes 0..255: pel is the build's long double, the function takes and returns a double, `* 255` is then a
// double product, and the store into the float coefficient rounds once more
inline void trc_u8_decode_lut(float lut[256], int trc)
{
	TRC_NO_CONTRACT
	const TrcParams p = trc_params(trc);
	for (int k = 0; k < 256; k++) {
		long double pel = (long double)(unsigned char)k;
		pel = trc_exact(p, 1, (double)(pel / 255)) * 255;
		lut[k] = (float)pel;
	}
}

// motion.c:769,776 in double
inline uint8_t trc_u8_encode_exact(const TrcParams &p, double pel)
{
	TRC_NO_CONTRACT
	return quantise_u8(trc_exact(p, 0, pel / 255) * 255);
}

// doubles on a line of integers in their own order (-0.0 just below +0.0); its own inverse
inline int64_t trc_u8_key(int64_t bits) { return bits < 0 ? bits ^ INT64_MAX : bits; }

inline void trc_u8_thresholds(double thr[256], int trc)
{
	const TrcParams p = trc_params(trc);
	thr[0] = -INFINITY;
	for (int k = 1; k < 256; k++) {
		if (k > 1 && trc_u8_encode_exact(p, thr[k - 1]) >= k) { thr[k] = thr[k - 1]; continue; }     // (the byte steps over k - 1)
		double lo_d = thr[k - 1], hi_d = INFINITY;
		if (trc_u8_encode_exact(p, hi_d) < k) { thr[k] = INFINITY; continue; }                        // never reached
		int64_t lo, hi;
		memcpy(&lo, &lo_d, 8); memcpy(&hi, &hi_d, 8);
		lo = trc_u8_key(lo); hi = trc_u8_key(hi);
		// byte(lo) < k <= byte(hi)
		while ((uint64_t)hi - (uint64_t)lo > 1) {
			const int64_t mid = lo + (int64_t)(((uint64_t)hi - (uint64_t)lo) >> 1), mb = trc_u8_key(mid);
			double m;
			memcpy(&m, &mb, 8);
			if (trc_u8_encode_exact(p, m) >= k) hi = mid; else lo = mid;
		}
		hi = trc_u8_key(hi);
		memcpy(&thr[k], &hi, 8);
	}
}
inline void trc_u8_tab_build(TrcU8Tab &t, int trc) { trc_u8_thresholds(t.thr, trc); trc_u8_decode_lut(t.lut, trc); }

}  // namespace dspfft
