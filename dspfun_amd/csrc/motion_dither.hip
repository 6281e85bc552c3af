// motion_dither.hip -- motion's Floyd-Steinberg 8-bit store (motion/motion.c:756-788 with -d) on the device.  The per-pixel arithmetic and
// the order of the four error additions are dither_core.h's; this file only schedules pixels.
//
// A pixel depends on its left neighbour and on the three pixels above it, so every pixel with the same x + 2y can be computed at once:
// a plane takes w + 2(h - 1) dependent steps instead of w h.  Planes (z planes of a block, and blocks) are independent.  Two regimes,
// chosen from the plane size in dither_launch:
//  * small planes (w <= 64 and h w <= 1024: --blocksize 8x8x8, 16x16 ...): ONE LANE per plane, raster order (dither_plane_serial), the
//    previous row's errors in LDS.  A 64-pixel plane is 64 steps; the clip supplies millions of planes.
//  * large planes (whole frames): a WORKGROUP per plane.  Lane l of a wave owns row 64 b + l of band b and handles column t - 2 l at
//    step t, receiving the fresh error of the row above from lane l - 1 (__shfl_up) each step.  Bands go to the nw waves of the workgroup
//    in turn, band b starting D steps after band b - 1 (D >= 128 + C: the band's top row needs the row above two columns ahead, which
//    lane 63 of the band above produces 126 steps after its lane 0).  The band's last row hands its errors to the next band through a
//    ring in LDS.  The waves step in lockstep chunks of C steps with a barrier between chunks: a ring slot written in one chunk is read
//    in a later one, and is not overwritten until a later chunk still (ring length R = D - 126 + C, nw + 1 rings).
//    One wave per plane (bands one after another) is the same kernel with nw = 1; DESIGN.md appendix has both measured.
// Each lane reads its row C floats at a time (the next chunk's while it computes this one) and stores C bytes at the end of a chunk.  d_coeffs is only read.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

#include "../../include/dspfft.h"
#include "dither_core.h"

using namespace dspfft;

extern "C" int dspfft_motion_set_error(const char *m);     // motion_ops.hip: the message dspfft_motion_last_error returns
extern "C" const void *dspfft_u8_trc_cached_tab(int trc);  // motion_ops.hip: this device's tables of a transfer characteristic (NULL: upload failed)

namespace {

constexpr int kChunk = 16;            // C: steps between barriers
constexpr int kMaxWaves = 16;
constexpr size_t kMaxLds = 64 << 10;

struct Geom {
	int d, h, w;
	long long row, plane;
	int nb[3];
	long long step[3];
};

__device__ inline long long plane_base(const Geom &g, long long p)
{
	const long long z = p % g.d;
	long long q = p / g.d;
	const long long b2 = q % g.nb[2]; q /= g.nb[2];
	const long long b1 = q % g.nb[1], b0 = q / g.nb[1];
	return b0 * g.step[0] + b1 * g.step[1] + b2 * g.step[2] + z * g.plane;
}

// Packed pixels (dspfft_motion_dither_u8_packed): every component of a pixel plane is a plane of its own, its columns `es` elements apart.  row,
// plane and step count ELEMENTS here (the caller's pixels times es); plane index p = es * (pixel plane) + component.  The planar kernels are
// the instantiations on Geom, whose element step is the constant 1.
struct GeomP : Geom { int es; };
__device__ inline long long plane_base(const GeomP &g, long long p) { return plane_base(static_cast<const Geom &>(g), p / g.es) + p % g.es; }
__device__ constexpr int elem_step(const Geom &) { return 1; }
__device__ inline int elem_step(const GeomP &g) { return g.es; }

// --linear (TRC): the function's 256 thresholds lie in LDS behind the error table, and the rings / row errors behind them
struct TrcArg { const TrcU8Tab *tab; int id; };
constexpr int kTrcDoubles = 256;

// one lane per plane; 64 lanes per workgroup, their previous-row errors interleaved in LDS (lane-major: no bank conflicts)
template <bool TRC, class G>
__device__ __forceinline__ void dither_serial_body(uint8_t *pix, const float *co, G g, long long nplanes, double sf, double norm, TrcArg t)
{
	extern __shared__ double lds[];
	double *tab = lds, *thr = lds + 256, *dprow = lds + 256 + (TRC ? kTrcDoubles : 0);
	for (int i = threadIdx.x; i < 256; i += blockDim.x) { tab[i] = dither_table_entry(i, sf, norm); if constexpr (TRC) thr[i] = t.tab->thr[i]; }
	__syncthreads();
	const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= nplanes) return;
	const long long base = plane_base(g, p);
	TrcParams tp;
	if constexpr (TRC) tp = trc_params(t.id);
	if constexpr (std::is_same<G, GeomP>::value) dither_plane_step<TRC>(pix + base, co + base, g.row, g.es, g.h, g.w, sf, norm, tab, dprow + threadIdx.x, blockDim.x, thr, &tp);
	else dither_plane_serial<TRC>(pix + base, co + base, g.row, g.h, g.w, sf, norm, tab, dprow + threadIdx.x, blockDim.x, thr, &tp);
}
template <class G>
__global__ __launch_bounds__(64) void dither_serial_kernel(uint8_t *pix, const float *co, G g, long long nplanes, double sf, double norm)
{
	dither_serial_body<false>(pix, co, g, nplanes, sf, norm, TrcArg{nullptr, 0});
}
template <class G>
__global__ __launch_bounds__(64) void dither_serial_trc_kernel(uint8_t *pix, const float *co, G g, long long nplanes, double sf, double norm, TrcArg t)
{
	dither_serial_body<true>(pix, co, g, nplanes, sf, norm, t);
}

struct WaveSched { int nw, D, R, L; };   // waves, band-to-band offset, ring length, steps per band (a multiple of kChunk)

template <bool TRC, class G>
__device__ __forceinline__ void dither_wave_body(uint8_t *pix, const float *co, G g, WaveSched s, double sf, double norm, TrcArg t)
{
	extern __shared__ double lds[];
	double *tab = lds, *thr = lds + 256, *rings = lds + 256 + (TRC ? kTrcDoubles : 0);
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (int i = threadIdx.x; i < 256; i += blockDim.x) { tab[i] = dither_table_entry(i, sf, norm); if constexpr (TRC) thr[i] = t.tab->thr[i]; }
	__syncthreads();
	TrcParams tp;
	if constexpr (TRC) tp = trc_params(t.id);
	const long long base = plane_base(g, blockIdx.x);
	const int h = g.h, w = g.w, nbands = (h + 63) >> 6, es = elem_step(g);
	const long long total = (long long)(nbands - 1) * s.D + s.L;
	int band = -1;
	// lane state: the window dp(r-1, x-1 .. x+1), the error handed down for the next step, the left neighbour's error, ring slots
	double a = 0, b0 = 0, c = 0, nxt = 0, left = 0;
	int ws = 0, rs = 0;
	float vn[kChunk];
	bool have_next = false;
	long long rowoff = 0;
	bool rowok = false, up = false;
	double *ring_w = rings, *ring_r = rings;
	for (long long T0 = 0; T0 < total; T0 += kChunk) {
		// this wave's band at T0: b = wave (mod nw), b D <= T0 < b D + L
		const long long kb = T0 / s.D;
		const long long b = kb - (((kb - wave) % s.nw) + s.nw) % s.nw;
		if (b >= 0 && b < nbands && T0 < b * s.D + s.L) {
			const int t0 = (int)(T0 - b * s.D);
			if (b != band) {
				band = (int)b;
				have_next = false;
				const int r = band * 64 + lane;
				rowok = r < h; up = r > 0;
				rowoff = base + (long long)(rowok ? r : 0) * g.row;
				ring_w = rings + (long long)(band % (s.nw + 1)) * s.R;
				ring_r = rings + (long long)((band + s.nw) % (s.nw + 1)) * s.R;        // band - 1's
				a = b0 = c = nxt = left = 0;
				ws = ((-126 % s.R) + s.R) % s.R;                                        // lane 63 writes column t - 126
				rs = 2 % s.R;                                                            // lane 0 reads column t + 2
				if (lane == 0 && band > 0) { c = ring_r[0]; nxt = w > 1 ? ring_r[1 % s.R] : 0.0; }
			}
			const int x0 = t0 - 2 * lane;
			float v[kChunk];
			uint8_t ob[kChunk];
			// this chunk's samples were loaded during the previous one (measured: no change, the step chain sets the pace -- DESIGN.md section 5)
#pragma unroll
			for (int i = 0; i < kChunk; i++) {
				const int x = x0 + i;
				v[i] = have_next ? vn[i] : (rowok && x >= 0 && x < w) ? co[rowoff + (long long)x * es] : 0.f;
			}
			have_next = t0 + kChunk < s.L;
			if (have_next) {
#pragma unroll
				for (int i = 0; i < kChunk; i++) {
					const int x = x0 + kChunk + i;
					vn[i] = (rowok && x >= 0 && x < w) ? co[rowoff + (long long)x * es] : 0.f;
				}
			}
#pragma unroll
			for (int i = 0; i < kChunk; i++) {
				const int x = x0 + i;
				a = b0; b0 = c; c = nxt;
				const bool act = rowok && x >= 0 && x < w;
				double dp;
				ob[i] = dither_pel<TRC>(v[i], up, x > 0, x + 1 < w, a, b0, c, left, sf, norm, tab, dp, thr, &tp);
				if (!act) dp = 0;
				left = dp;
				if (lane == 63 && act) ring_w[ws] = dp;
				ws = ws + 1 == s.R ? 0 : ws + 1;
				nxt = __shfl_up(dp, 1);
				if (lane == 0) nxt = (band > 0 && x + 2 < w) ? ring_r[rs] : 0.0;
				rs = rs + 1 == s.R ? 0 : rs + 1;
			}
#pragma unroll
			for (int i = 0; i < kChunk; i++) {
				const int x = x0 + i;
				if (rowok && x >= 0 && x < w) pix[rowoff + (long long)x * es] = ob[i];
			}
		}
		__syncthreads();
	}
}
template <class G>
__global__ __launch_bounds__(kMaxWaves * 64) void dither_wave_kernel(uint8_t *pix, const float *co, G g, WaveSched s, double sf, double norm)
{
	dither_wave_body<false>(pix, co, g, s, sf, norm, TrcArg{nullptr, 0});
}
template <class G>
__global__ __launch_bounds__(kMaxWaves * 64) void dither_wave_trc_kernel(uint8_t *pix, const float *co, G g, WaveSched s, double sf, double norm, TrcArg t)
{
	dither_wave_body<true>(pix, co, g, s, sf, norm, t);
}

bool small_plane(int h, int w) { return w <= 64 && (long long)h * w <= 1024; }

WaveSched wave_sched(int h, int w, int nw_max)
{
	WaveSched s;
	const int nbands = (h + 63) / 64;
	s.nw = nbands < nw_max ? nbands : nw_max;
	s.L = (w + 126 + kChunk - 1) / kChunk * kChunk;
	const int per = ((s.L + s.nw - 1) / s.nw + kChunk - 1) / kChunk * kChunk;    // a wave's next band starts after its last one ended
	s.D = per > 128 + kChunk ? per : 128 + kChunk;
	s.R = s.D - 126 + kChunk;                   // (lane 0 takes columns 0 and 1 at its band's first step, two steps later than the rest)
	return s;
}

int wave_limit()
{
	static const int v = []() { const char *e = getenv("DSPFFT_DITHER_WAVES"); const int n = e ? atoi(e) : kMaxWaves; return n < 1 ? 1 : n > kMaxWaves ? kMaxWaves : n; }();
	return v;
}

int dbad(char *err, size_t len, const char *m) { if (err && len) snprintf(err, len, "%s", m); return -1; }

}  // namespace

// the two regimes' launches on a geometry: Geom (planar) or GeomP (packed pixels)
template <class G>
static void dither_launch_serial(uint8_t *d_pix, const float *d_coeffs, const G &g, long long nplanes, size_t lds, double sf, double norm, const TrcArg &ta, hipStream_t st)
{
	const unsigned nwg = (unsigned)((nplanes + 63) / 64);
	if (ta.id) hipLaunchKernelGGL(dither_serial_trc_kernel<G>, dim3(nwg), dim3(64), lds, st, d_pix, d_coeffs, g, nplanes, sf, norm, ta);
	else hipLaunchKernelGGL(dither_serial_kernel<G>, dim3(nwg), dim3(64), lds, st, d_pix, d_coeffs, g, nplanes, sf, norm);
}
template <class G>
static void dither_launch_wave(uint8_t *d_pix, const float *d_coeffs, const G &g, long long nplanes, const WaveSched &s, size_t lds, double sf, double norm, const TrcArg &ta,
                               hipStream_t st)
{
	if (ta.id) hipLaunchKernelGGL(dither_wave_trc_kernel<G>, dim3((unsigned)nplanes), dim3(64 * s.nw), lds, st, d_pix, d_coeffs, g, s, sf, norm, ta);
	else hipLaunchKernelGGL(dither_wave_kernel<G>, dim3((unsigned)nplanes), dim3(64 * s.nw), lds, st, d_pix, d_coeffs, g, s, sf, norm);
}

// trc = 0: the plain store; else tab points at the function's tables on the device.  comps = 0: planar buffers; 2..4: packed pixels, *gp in
// pixels.  dry: every check, no launch (the buffers are then not looked at).
static int dither_launch(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *gp, int comps, double scalefactor, double normalization, int trc, const void *tab,
                         void *stream, char *err, size_t errlen, bool dry = false)
{
	if ((!dry && (!d_pix || !d_coeffs)) || !gp) return dbad(err, errlen, "dither: null pointer");
	const dspfft_dither_geom &q = *gp;
	if (q.n[0] < 1 || q.n[1] < 1 || q.n[2] < 1 || q.nblocks[0] < 1 || q.nblocks[1] < 1 || q.nblocks[2] < 1) return dbad(err, errlen, "dither: extents and block counts must be >= 1");
	if ((q.n[1] > 1 && q.row_pitch < q.n[2]) || (q.n[0] > 1 && q.plane_pitch < 1) || q.row_pitch < 0 || q.plane_pitch < 0 ||
	    q.block_step[0] < 0 || q.block_step[1] < 0 || q.block_step[2] < 0)
		return dbad(err, errlen, "dither: row pitch below the row length, or a negative pitch / block step");
	if (!(scalefactor > 0) || !(normalization > 0) || !isfinite(scalefactor) || !isfinite(normalization)) return dbad(err, errlen, "dither: scalefactor and normalization must be finite and > 0");
	Geom g;
	g.d = q.n[0]; g.h = q.n[1]; g.w = q.n[2]; g.row = q.n[1] > 1 ? q.row_pitch : q.n[2]; g.plane = q.plane_pitch;
	for (int i = 0; i < 3; i++) { g.nb[i] = q.nblocks[i]; g.step[i] = q.block_step[i]; }
	const int es = comps ? comps : 1;
	const long long nplanes = (long long)g.d * g.nb[0] * g.nb[1] * g.nb[2] * es;
	GeomP gq;
	static_cast<Geom &>(gq) = g;
	gq.es = es; gq.row *= es; gq.plane *= es;
	for (int i = 0; i < 3; i++) gq.step[i] *= es;
	hipStream_t st = (hipStream_t)stream;
	const TrcArg ta = {(const TrcU8Tab *)tab, trc};
	if (small_plane(g.h, g.w)) {
		const size_t lds = (256 + (trc ? kTrcDoubles : 0) + 64 * (size_t)g.w) * sizeof(double);
		if ((nplanes + 63) / 64 >= (1ll << 31)) return dbad(err, errlen, "dither: too many planes");
		if (dry) return 0;
		if (comps) dither_launch_serial(d_pix, d_coeffs, gq, nplanes, lds, scalefactor, normalization, ta, st);
		else dither_launch_serial(d_pix, d_coeffs, g, nplanes, lds, scalefactor, normalization, ta, st);
	} else {
		const WaveSched s = wave_sched(g.h, g.w, wave_limit());
		const size_t lds = (256 + (trc ? kTrcDoubles : 0) + (size_t)(s.nw + 1) * s.R) * sizeof(double);
		if (lds > kMaxLds) return dbad(err, errlen, "dither: plane too wide for the wavefront kernel's LDS rings (w above about 9000)");
		if (nplanes >= (1ll << 31)) return dbad(err, errlen, "dither: too many planes");
		if (dry) return 0;
		if (comps) dither_launch_wave(d_pix, d_coeffs, gq, nplanes, s, lds, scalefactor, normalization, ta, st);
		else dither_launch_wave(d_pix, d_coeffs, g, nplanes, s, lds, scalefactor, normalization, ta, st);
	}
	return hipGetLastError() == hipSuccess ? 0 : dbad(err, errlen, "dither: kernel launch failed");
}

// The launchers behind the entry points (engine.cpp reaches them through weak references: absent from the CPU emulation build).
extern "C" __attribute__((visibility("hidden"))) int dspfft_dither_launch(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *gp,
                                                                           double scalefactor, double normalization, void *stream, char *err, size_t errlen)
{
	return dither_launch(d_pix, d_coeffs, gp, 0, scalefactor, normalization, 0, nullptr, stream, err, errlen);
}
// --linear: trc is a built id (engine.cpp has checked it); tab: a plan's device tables, or NULL for motion_ops.hip's own
extern "C" __attribute__((visibility("hidden"))) int dspfft_dither_trc_launch(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *gp, double scalefactor,
                                                                               double normalization, int trc, const void *tab, void *stream, char *err, size_t errlen)
{
	if (!tab) tab = dspfft_u8_trc_cached_tab(trc);
	if (!tab) return dbad(err, errlen, "dither: the transfer characteristic's tables could not be uploaded");
	return dither_launch(d_pix, d_coeffs, gp, 0, scalefactor, normalization, trc, tab, stream, err, errlen);
}
// packed pixels (dspfft_motion_dither_u8_packed; engine.cpp has checked comps and trc).  trc = 0: plain; tab as above.  dry: the checks alone,
// for a caller that must refuse before it launches anything
extern "C" __attribute__((visibility("hidden"))) int dspfft_dither_packed_launch(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *gp, int comps, double scalefactor,
                                                                                  double normalization, int trc, const void *tab, int dry, void *stream, char *err, size_t errlen)
{
	if (trc && !tab && !dry) tab = dspfft_u8_trc_cached_tab(trc);
	if (trc && !tab && !dry) return dbad(err, errlen, "dither: the transfer characteristic's tables could not be uploaded");
	return dither_launch(d_pix, d_coeffs, gp, comps, scalefactor, normalization, trc, tab, stream, err, errlen, dry != 0);
}

extern "C" int dspfft_motion_dither_u8(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, double scalefactor, double normalization, void *stream)
{
	char err[256];
	const int rc = dspfft_dither_launch(d_pix, d_coeffs, g, scalefactor, normalization, stream, err, sizeof err);
	if (rc) dspfft_motion_set_error(err);
	return rc;
}

extern "C" int dspfft_motion_dither_u8_trc(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, double scalefactor, double normalization, int trc, void *stream)
{
	if (!trc_built(trc)) { dspfft_motion_set_error("dither: the transfer characteristic is not built"); return -1; }
	char err[256];
	const int rc = dspfft_dither_trc_launch(d_pix, d_coeffs, g, scalefactor, normalization, trc, nullptr, stream, err, sizeof err);
	if (rc) dspfft_motion_set_error(err);
	return rc;
}
