// trc_core.h -- transfer characteristics: the per-sample encode E = f(L) and decode L = f^-1(E) behind scan -g, zoom -g and
// motion --linear (scan/scan.c:412-414,455-457,486-488, zoom/zoom.c:393-399, motion/motion.c:632-633,768-769), shared by the HIP kernels
// (pointwise.hip, scan_frame.hip, zoom_anim.hip, motion_ops.hip), engine.cpp and the CPU tests, which compile it with g++.
//
// The reference takes these functions from libavutil (av_csp_trc_func_from_id / av_csp_trc_func_inv_from_id).  libavutil is not in the
// reference tree: the table below is written from the standards (BT.709, SMPTE 240M, IEC 61966-2-1 and -2-4, BT.470's pure gammas) and
// from recollection of libavutil's csp.c, its treatment of inputs outside [0, 1] included -- parity with libavutil is unpinned, as
// SURVEY.md 8c says of FFTW.  Ids are AVColorTransferCharacteristic's values, names av_color_transfer_name's.  The first matching
// condition decides (a709 = 1.099296826809442, b709 = 0.018053968510807):
//
//   1, 6, 14, 15  bt709 smpte170m bt2020-10 bt2020-12   encode  0 > L: 0;  b709 > L: 4.5 L;  else a709 pow(L, 0.45) - (a709 - 1)
//                                                       decode  0 > E: 0;  4.5 b709 > E: E / 4.5;  else pow((E + (a709 - 1)) / a709, 1 / 0.45)
//   4, 5          gamma22 gamma28 (g = 2.2, 2.8)        encode  0 > L: 0;  else pow(L, 1 / g)          decode  0 > E: 0;  else pow(E, g)
//   7             smpte240m                             as bt709 with a = 1.1115, b = 0.0228, slope 4
//   8             linear                                the identity
//   11            iec61966-2-4                          encode  -b709 >= L: -(a709 pow(-L, 0.45) - (a709 - 1));  b709 > L: 4.5 L;  else as bt709
//                                                       decode  -4.5 b709 >= E: -pow((-E + (a709 - 1)) / a709, 1 / 0.45);  4.5 b709 > E: E / 4.5;
//                                                               else as bt709
//   13            iec61966-2-1                          as bt709 with a = 1.055, b = 0.0031308, slope 12.92, exponents 1 / 2.4 and 2.4
//
// -0.0 passes the first test and comes out as -0.0 on the linear segment (+0.0 from the pure gammas' pow); NaN fails every comparison,
// reaches pow and stays NaN; +inf stays +inf.  log100, log316, bt1361e, smpte2084, smpte428 and arib-std-b67 are not built.
//
// Two evaluations:
//  * trc_exact: double in, double out, every operation in double in the order written, nothing contracted into an FMA, libm's / the
//    device library's pow.  What the reference computes; motion's load and store use it (their divisions by 255 sit outside the function
//    and the reference keeps the double).
//  * trc_eval_f32: float in, float out, the production evaluation of the frame kernels and dspfft_trc_apply_f32.  The same comparisons
//    and affine pieces in double around trc_pow_lean, a pow that spends only what a float result needs (relative error below 2^-40, where
//    a float ulp is 2^-23): the result is (float)trc_exact((double)x) or its neighbour, and bit-equal where that is +-0, NaN or +-inf.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "radix.h"

#if defined(__clang__)
#define TRC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TRC_NO_CONTRACT
#endif

namespace dspfft {

enum { TRC_NONE = 0, TRC_BT709 = 1, TRC_GAMMA22 = 4, TRC_GAMMA28 = 5, TRC_SMPTE170M = 6, TRC_SMPTE240M = 7, TRC_LINEAR = 8,
       TRC_IEC61966_2_4 = 11, TRC_IEC61966_2_1 = 13, TRC_BT2020_10 = 14, TRC_BT2020_12 = 15 };

// av_color_transfer_name's names of the ids that are built; NULL otherwise (0, `none` here, is no function: it means "leave as is")
inline const char *trc_name(int id)
{
	switch (id) {
	case TRC_BT709: return "bt709";
	case TRC_GAMMA22: return "gamma22";
	case TRC_GAMMA28: return "gamma28";
	case TRC_SMPTE170M: return "smpte170m";
	case TRC_SMPTE240M: return "smpte240m";
	case TRC_LINEAR: return "linear";
	case TRC_IEC61966_2_4: return "iec61966-2-4";
	case TRC_IEC61966_2_1: return "iec61966-2-1";
	case TRC_BT2020_10: return "bt2020-10";
	case TRC_BT2020_12: return "bt2020-12";
	}
	return nullptr;
}
inline int trc_from_name(const char *name)
{
	if (!name) return -1;
	for (int id = 1; id <= TRC_BT2020_12; id++) {
		const char *n = trc_name(id);
		if (n && !strcmp(n, name)) return id;
	}
	return -1;
}
inline bool trc_built(int id) { return trc_name(id) != nullptr; }

// shape 0: identity; 1: pure gamma; 2: linear toe + offset power; 3: the same, odd-symmetric (iec61966-2-4)
struct TrcParams { int shape; double a, b, slope, g_enc, g_dec; };
DSP_HD TrcParams trc_params(int id)
{
	TRC_NO_CONTRACT
	TrcParams p = {0, 1.0, 0.0, 1.0, 1.0, 1.0};
	switch (id) {
	case TRC_GAMMA22: p.shape = 1; p.g_enc = 1 / 2.2; p.g_dec = 2.2; break;
	case TRC_GAMMA28: p.shape = 1; p.g_enc = 1 / 2.8; p.g_dec = 2.8; break;
	case TRC_BT709: case TRC_SMPTE170M: case TRC_BT2020_10: case TRC_BT2020_12: case TRC_IEC61966_2_4:
		p.shape = id == TRC_IEC61966_2_4 ? 3 : 2;
		p.a = 1.099296826809442; p.b = 0.018053968510807; p.slope = 4.5; p.g_enc = 0.45; p.g_dec = 1 / 0.45; break;
	case TRC_SMPTE240M: p.shape = 2; p.a = 1.1115; p.b = 0.0228; p.slope = 4.0; p.g_enc = 0.45; p.g_dec = 1 / 0.45; break;
	case TRC_IEC61966_2_1: p.shape = 2; p.a = 1.055; p.b = 0.0031308; p.slope = 12.92; p.g_enc = 1 / 2.4; p.g_dec = 2.4; break;
	default: break;
	}
	return p;
}

struct TrcPowLibm { DSP_HD double operator()(double x, double e) const { return pow(x, e); } };

// pow(x, e) for the calls the table makes (x >= 0 or NaN, 0 < e < 3, results a float can hold or that round to 0 / inf as a float):
// x = 2^k m, m in (sqrt 1/2, sqrt 2]; log2 m = (2 / ln 2) atanh t, t = (m - 1) / (m + 1), |t| <= 0.1716, nine terms (the tenth is below
// 2^-49 of the sum); 2^(n + f), |f| <= 1/2, by the Taylor series of exp(f ln 2) to degree 11 (the next term is below 2^-47).  With the
// roundings of y = e (k + log2 m), |y| < 1100, the relative error stays below 2^-40.  Specials as pow's: +-0 -> +0, +inf -> +inf,
// NaN -> itself, negative x -> NaN.  Contraction is left to the build here: the library (-ffp-contract=on) fuses the Horner steps into
// FMAs, the CPU tests' g++ build (-ffp-contract=off) does not, so the two differ in the last places of the double -- inside the 2^-40
// either way (tests/test_trc_cpu.py bounds the host build against libm's pow directly; the GPU sweep covers the device's).
DSP_HD double trc_pow_lean(double x, double e)
{
	if (!(x > 0.0)) return x == 0.0 ? 0.0 : x != x ? x : NAN;
	if (!(x < INFINITY)) return x;
	uint64_t u;
	memcpy(&u, &x, 8);
	int k = (int)(u >> 52) - 1023;
	if (k == -1023) {                       // a subnormal double (never a converted float): normalise
		x *= 0x1p64;
		memcpy(&u, &x, 8);
		k = (int)(u >> 52) - 1023 - 64;
	}
	u = (u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
	double m;
	memcpy(&m, &u, 8);
	if (m > 1.41421356237309504880) { m *= 0.5; k++; }
	const double t = (m - 1.0) / (m + 1.0), t2 = t * t;
	double s = 2.8853900817779268 / 17;
	s = s * t2 + 2.8853900817779268 / 15;
	s = s * t2 + 2.8853900817779268 / 13;
	s = s * t2 + 2.8853900817779268 / 11;
	s = s * t2 + 2.8853900817779268 / 9;
	s = s * t2 + 2.8853900817779268 / 7;
	s = s * t2 + 2.8853900817779268 / 5;
	s = s * t2 + 2.8853900817779268 / 3;
	s = s * t2 + 2.8853900817779268;
	double y = e * ((double)k + t * s);
	if (y > 1100.0) y = 1100.0;
	if (y < -1100.0) y = -1100.0;
	const double n = rint(y), z = (y - n) * 0.69314718055994530942;
	double r = 1.0 / 39916800;
	r = r * z + 1.0 / 3628800;
	r = r * z + 1.0 / 362880;
	r = r * z + 1.0 / 40320;
	r = r * z + 1.0 / 5040;
	r = r * z + 1.0 / 720;
	r = r * z + 1.0 / 120;
	r = r * z + 1.0 / 24;
	r = r * z + 1.0 / 6;
	r = r * z + 0.5;
	r = r * z + 1.0;
	r = r * z + 1.0;
	// 2^n in two factors: n reaches -1100 and 1100, past a double's exponents, and the product then rounds to 0 or inf as it should
	const int ni = (int)n, n1 = ni / 2, n2 = ni - n1;
	const uint64_t b1 = (uint64_t)(n1 + 1023) << 52, b2 = (uint64_t)(n2 + 1023) << 52;
	double f1, f2;
	memcpy(&f1, &b1, 8);
	memcpy(&f2, &b2, 8);
	return r * f1 * f2;
}
struct TrcPowLean { DSP_HD double operator()(double x, double e) const { return trc_pow_lean(x, e); } };

// the table, over a pow
template <class POW>
DSP_HD double trc_encode_with(const TrcParams &p, double L, POW pw)
{
	TRC_NO_CONTRACT
	if (p.shape == 0) return L;
	if (p.shape == 1) return 0 > L ? 0.0 : pw(L, p.g_enc);
	if (p.shape == 3 && -p.b >= L) return -(p.a * pw(-L, p.g_enc) - (p.a - 1));
	if (p.shape == 2 && 0 > L) return 0.0;
	if (p.b > L) return p.slope * L;
	return p.a * pw(L, p.g_enc) - (p.a - 1);
}
template <class POW>
DSP_HD double trc_decode_with(const TrcParams &p, double E, POW pw)
{
	TRC_NO_CONTRACT
	if (p.shape == 0) return E;
	if (p.shape == 1) return 0 > E ? 0.0 : pw(E, p.g_dec);
	if (p.shape == 3 && -(p.slope * p.b) >= E) return -pw((-E + (p.a - 1)) / p.a, p.g_dec);
	if (p.shape == 2 && 0 > E) return 0.0;
	if (p.slope * p.b > E) return E / p.slope;
	return pw((E + (p.a - 1)) / p.a, p.g_dec);
}

// the exact evaluation
DSP_HD double trc_exact(const TrcParams &p, int inverse, double v)
{
	return inverse ? trc_decode_with(p, v, TrcPowLibm()) : trc_encode_with(p, v, TrcPowLibm());
}
DSP_HD double trc_exact(int id, int inverse, double v) { return trc_exact(trc_params(id), inverse, v); }

// the production evaluation
DSP_HD float trc_eval_f32(const TrcParams &p, int inverse, float v)
{
	return (float)(inverse ? trc_decode_with(p, (double)v, TrcPowLean()) : trc_encode_with(p, (double)v, TrcPowLean()));
}
DSP_HD float trc_eval_f32(int id, int inverse, float v) { return trc_eval_f32(trc_params(id), inverse, v); }

}  // namespace dspfft
