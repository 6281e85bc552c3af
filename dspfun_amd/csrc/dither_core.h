// dither_core.h -- motion's Floyd-Steinberg 8-bit store (motion/motion.c:756-788 with -d: spec none, 8-bit pixels; TRC = true: --linear,
// the byte is the encoded one, trc_u8_core.h, while the error stays the reference's c - byte / (normalization^2 scalefactor), :780) as the
// arithmetic of ONE pixel, shared by the HIP kernels (motion_dither.hip) and host code (the CPU tests compile it with g++).
//
// The reference walks a plane in raster order and adds each pixel's error into four float neighbours.  Every `+=` rounds back to float
// (`coeff` is float, COEFF_PRECISION=F), so the order of the four additions into a coefficient is part of the result.  Pixel (y, x)
// receives, in this order: dp(y-1, x-1) / 16, dp(y-1, x) * 5 / 16, dp(y-1, x+1) * 3 / 16, dp(y, x-1) * 7 / 16 (each term present when its
// source pixel exists).  dither_pel applies them at the receiving pixel, which is the same sequence of roundings: the coefficient buffer
// itself is never written, and the only state a pixel hands on is its error dp.
//
// Arithmetic in double (`intermediate`; byte-identical to the reference's lines built with INTERMEDIATE_PRECISION=D; the tool's default
// long double differs by +-1 on a few per cent of the pixels of a large plane, see include/dspfft.h).  Nothing may be contracted into an
// FMA: the product library is built with -ffp-contract=on, hence DITHER_NO_CONTRACT in every function below.
#pragma once
#include <math.h>
#include <stdint.h>
#include "radix.h"
#include "trc_u8_core.h"

#if defined(__clang__)
#define DITHER_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DITHER_NO_CONTRACT
#endif

namespace dspfft {

// motion.c:778  p / (normalization * normalization * scalefactor) for the 256 byte values, correctly rounded (p is an integer)
DSP_HD double dither_table_entry(int p, double scalefactor, double norm)
{
	DITHER_NO_CONTRACT
	const double k = norm * norm * scalefactor;
	return (double)p / k;
}
DSP_HD void dither_table(double *tab, double scalefactor, double norm)
{
	for (int p = 0; p < 256; p++) tab[p] = dither_table_entry(p, scalefactor, norm);
}

// (float)(c + term): a float coefficient += an intermediate (motion.c:779-784)
DSP_HD float dither_add(float c, double term)
{
	DITHER_NO_CONTRACT
	return (float)((double)c + term);
}

// One pixel.  c: the inverse transform's float; up: the row above exists; xm / xp: columns x-1 / x+1 exist; dm, d0, dq: dp of the pixels
// (y-1, x-1), (y-1, x), (y-1, x+1); dl: dp of (y, x-1).  Returns the byte (motion.c:759-776) and its error in dp (:778).
// TRC: thr is the function's threshold table and tp its parameters (they only seed the search in thr).
template <bool TRC = false>
DSP_HD uint8_t dither_pel(float c, bool up, bool xm, bool xp, double dm, double d0, double dq, double dl, double scalefactor, double norm,
                          const double *tab, double &dp, const double *thr = nullptr, const TrcParams *tp = nullptr)
{
	DITHER_NO_CONTRACT
	if (up) {
		if (xm) c = dither_add(c, dm / 16);
		c = dither_add(c, d0 * 5 / 16);
		if (xp) c = dither_add(c, dq * 3 / 16);
	}
	if (xm) c = dither_add(c, dl * 7 / 16);
	double pel = (double)c * scalefactor * norm;
	pel *= norm;
	uint8_t p;
	if constexpr (TRC) p = (uint8_t)trc_u8_byte_from(thr, pel, trc_u8_seed(*tp, pel));   // :769,776
	else p = pel > 255 ? 255 : pel < 0 ? 0 : (uint8_t)round(pel);              // lround: halves away from zero
	dp = (double)c - tab[p];
	return p;
}

// One h x w plane in raster order, as the reference walks it.  dprow: w doubles of scratch at stride dstride (the previous row's errors,
// overwritten as the row advances); in and out are addressed (y * pitch + x).
template <bool TRC = false>
DSP_HD void dither_plane_serial(uint8_t *out, const float *in, long long pitch, int h, int w, double scalefactor, double norm, const double *tab,
                                double *dprow, int dstride, const double *thr = nullptr, const TrcParams *tp = nullptr)
{
	for (int y = 0; y < h; y++) {
		const bool up = y > 0;
		double dm = 0, d0 = 0, dq = up ? dprow[0] : 0.0, dl = 0;
		for (int x = 0; x < w; x++) {
			dm = d0; d0 = dq;
			const bool xp = x + 1 < w;
			dq = (up && xp) ? dprow[(long long)(x + 1) * dstride] : 0.0;
			double dp;
			out[(long long)y * pitch + x] = dither_pel<TRC>(in[(long long)y * pitch + x], up, x > 0, xp, dm, d0, dq, dl, scalefactor, norm, tab, dp, thr, tp);
			if (x > 0) dprow[(long long)(x - 1) * dstride] = dl;       // (y-1, x-1) is not read again in this row
			dl = dp;
		}
		dprow[(long long)(w - 1) * dstride] = dl;
	}
}

// The raster walk once more, over a plane that is not a dense run of floats beside a dense run of bytes: get(y, x) is the pixel's float and
// put(y, x, byte) takes its byte.  A pixel's float is read once, by that pixel and before its put, so put may overwrite what get reads.
template <bool TRC = false, class Get, class Put>
DSP_HD void dither_plane_raster(Get get, Put put, int h, int w, double scalefactor, double norm, const double *tab, double *dprow, int dstride,
                                const double *thr = nullptr, const TrcParams *tp = nullptr)
{
	DITHER_NO_CONTRACT
	for (int y = 0; y < h; y++) {
		const bool up = y > 0;
		double dm = 0, d0 = 0, dq = up ? dprow[0] : 0.0, dl = 0;
		for (int x = 0; x < w; x++) {
			dm = d0; d0 = dq;
			const bool xp = x + 1 < w;
			dq = (up && xp) ? dprow[(long long)(x + 1) * dstride] : 0.0;
			double dp;
			put(y, x, dither_pel<TRC>(get(y, x), up, x > 0, xp, dm, d0, dq, dl, scalefactor, norm, tab, dp, thr, tp));
			if (x > 0) dprow[(long long)(x - 1) * dstride] = dl;
			dl = dp;
		}
		dprow[(long long)(w - 1) * dstride] = dl;
	}
}
// ... a component's plane of packed pixels: columns `step` elements apart in `in` and `out` alike (step 1 is dither_plane_serial)
template <bool TRC = false>
DSP_HD void dither_plane_step(uint8_t *out, const float *in, long long pitch, int step, int h, int w, double scalefactor, double norm, const double *tab,
                              double *dprow, int dstride, const double *thr = nullptr, const TrcParams *tp = nullptr)
{
	DITHER_NO_CONTRACT
	dither_plane_raster<TRC>([=](int y, int x) { return in[(long long)y * pitch + (long long)x * step]; },
	                         [=](int y, int x, uint8_t b) { out[(long long)y * pitch + (long long)x * step] = b; }, h, w, scalefactor, norm, tab, dprow, dstride, thr, tp);
}
// ... a plane of a fused block kernel's LDS tile, in place: the float at (y, x) makes way for its byte, held as a 32-bit integer in the same slot
// (dither_tile_byte reads it back)
template <bool TRC = false>
DSP_HD void dither_plane_tile(float *tile, int pitch, int h, int w, double scalefactor, double norm, const double *tab, double *dprow, int dstride,
                              const double *thr = nullptr, const TrcParams *tp = nullptr)
{
	DITHER_NO_CONTRACT
	dither_plane_raster<TRC>([=](int y, int x) { return tile[y * pitch + x]; },
	                         [=](int y, int x, uint8_t b) { const uint32_t v = b; __builtin_memcpy(tile + y * pitch + x, &v, 4); }, h, w, scalefactor, norm, tab, dprow, dstride, thr, tp);
}
DSP_HD uint32_t dither_tile_byte(const float *slot)
{
	uint32_t v;
	__builtin_memcpy(&v, slot, 4);
	return v;
}

// The same plane in the device kernel's wavefront order: every pixel with the same x + 2y at once (a pixel depends on (y, x-1) and
// (y-1, x-1 .. x+1), all on earlier anti-diagonals).  dp: h * w doubles of scratch.  Host-side check that the order does not change a byte.
DSP_HD void dither_plane_wavefront(uint8_t *out, const float *in, long long pitch, int h, int w, double scalefactor, double norm, const double *tab,
                                   double *dp)
{
	for (long long t = 0; t < (long long)w + 2LL * (h - 1); t++)
		for (int y = 0; y < h; y++) {
			const long long x = t - 2LL * y;
			if (x < 0 || x >= w) continue;
			const bool up = y > 0, xm = x > 0, xp = x + 1 < w;
			const double *a = dp + (long long)(y - 1) * w;
			out[(long long)y * pitch + x] = dither_pel(in[(long long)y * pitch + x], up, xm, xp, up && xm ? a[x - 1] : 0.0, up ? a[x] : 0.0,
			                                           up && xp ? a[x + 1] : 0.0, xm ? dp[(long long)y * w + x - 1] : 0.0, scalefactor, norm, tab,
			                                           dp[(long long)y * w + x]);
		}
}

}  // namespace dspfft
