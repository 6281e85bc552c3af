// zoom_anim_core.h -- per-frame scalars and the per-pixel rule of zoom's animation loop (zoom/zoom.c:320-410), shared by engine.cpp
// (dspfft_zoomanim_*), the HIP kernel that finishes a frame (zoom_anim.hip) and the CPU tests, which compile it with g++.
//
// --showsamples (zoom.c:377-390), applied only when xscale > 1 && yscale > 1 (the frame's own scales, not clamped):
//     for (size_t y = yscale - (size_t)vy % (int)yscale; y < vh; y += yscale)          (and the columns alike with vx, xscale, vw)
//         memcpy(icoeffs + (y * vh + x) * 3, {0, 1, 0}, ...)
// The loop variable is an integer, so `y += yscale` truncates to y + floor-step: the rows are y0 + k dy, with dy the first step
// (size_t)(y0 + yscale) - y0 taken in long double.  The linear index is y * vh + x -- vh, not vw, a quirk of the reference that is kept --
// into the vw x vh interleaved frame: output pixel L = row * vw + col shows (0, 1, 0) when L = y vh + x for a marked (y, x).  When
// vh <= vw every write lands in the frame; when vh > vw the reference writes past its buffer, and here indices >= vw vh are dropped.
// Negative vx / vy are undefined in the reference ((size_t) of a negative value); here the offset is converted through long long
// (two's complement, x86's behaviour for values in range), so the remainder is that of 2^64 + trunc(v).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "radix.h"

namespace dspfft {

// the overlay of one frame: rows y0 + k dy < vh, columns x0 + k dx < vw; mode 0 none, 1 point, 2 grid
struct ZaOverlay {
	int mode, vw, vh;
	long long x0, dx, y0, dy;
};

DSP_HD bool za_on(long long p, long long p0, long long dp) { return p >= p0 && (p - p0) % dp == 0; }

// is output pixel L (< vw vh) written by zoom.c:377-390?  The (y, x) with y vh + x = L, x < vw, y < vh: y from ceil((L - vw + 1) / vh)
// to floor(L / vh) (at most vw / vh + 1 of them)
DSP_HD bool za_overlay_hit(const ZaOverlay &o, long long L)
{
	if (!o.mode) return false;
	const long long lo = L - o.vw + 1 <= 0 ? 0 : (L - o.vw + o.vh) / o.vh;
	long long hi = L / o.vh;
	if (hi > o.vh - 1) hi = o.vh - 1;
	for (long long y = lo; y <= hi; y++) {
		const long long x = L - y * o.vh;
		const bool row = za_on(y, o.y0, o.dy), col = za_on(x, o.x0, o.dx);
		if (o.mode == 1 ? (row && col) : (row || col)) return true;
	}
	return false;
}

// libavutil's comp[] table of GBRPF32: R (z = 0) is plane 2, G plane 0, B plane 1
DSP_HD int za_plane_of(int z) { return z == 0 ? 2 : z - 1; }

// ---- host-side scalars of a frame ----
// one axis's start and step of the overlay loop, in the reference's long double (INTERMEDIATE_PRECISION=L)
inline void za_overlay_axis(long double scale, double v, long long &p0, long long &dp)
{
	const size_t r = (size_t)(long long)v % (size_t)(int)scale;
	const size_t first = (size_t)(scale - (long double)r);
	p0 = (long long)first;
	dp = (long long)((size_t)((long double)first + scale) - first);
}
inline ZaOverlay za_overlay(int mode, double xnum, double xden, double ynum, double yden, double vx, double vy, int vw, int vh)
{
	ZaOverlay o = {0, vw, vh, 0, 1, 0, 1};
	const long double xs = (long double)xnum / (long double)xden, ys = (long double)ynum / (long double)yden;
	if (!mode || !(xs > 1 && ys > 1)) return o;
	o.mode = mode;
	za_overlay_axis(xs, vx, o.x0, o.dx);
	za_overlay_axis(ys, vy, o.y0, o.dy);
	return o;
}

// zoom.c:37-41 and the chirp-z (omega, phi) of an axis (dct_czt.h: out[b] = sum'_n C[n] cos(n (omega b + phi))).  zoom.c:49-61: sample b
// sits at k = alpha (b + offset) on a basis of N points: interpolated alpha = den / num, N = len; native alpha = 1, N = len num / den;
// centered alpha = (len - 1) den / (len num - den), N = len.  Returns the number of components, 0 when the centered basis is degenerate
// (len num - den <= 0 after the clamp).  Double arithmetic, as dspfft_zoom_ncomponents and dspfft_zoomczt_*.
inline int za_axis(int type, double num, double den, int len, double off, double &omega, double &phi)
{
	const double pi = 3.14159265358979323846;
	if (len * num / den < 1) { num = 1; den = (double)len; }
	const double want = round(len * num / den);
	const int nc = want < (double)len ? (int)want : len;
	double alpha, N;
	if (type == 2) { alpha = 1.0; N = len * num / den; }
	else if (type == 0) { alpha = den / num; N = len; }
	else {
		if (!(len * num - den > 0)) return 0;
		alpha = (len - 1) * den / (len * num - den); N = len;
	}
	omega = pi * alpha / N;
	phi = pi * (alpha * off + 0.5) / N;
	return nc;
}

}  // namespace dspfft
