// motion_ops.hip -- the remaining elementwise / selection stages of motion's block loop (motion/motion.c) as device kernels:
//   :617-640  pixel load with the inverse-spectrogram decodes (--ispec shift / flat / copy)
//   :652-668  keep the N coefficients of largest magnitude (--coeff-limit): radix select, no full sort
//   :755-776  output scaling (scalefactor, normalization), spectrogram encodes (--spec abs / shift / flat), clamp + lround
//   :632-633, :768-769  --linear on float pixels: the transfer characteristic's decode on load, encode on store
//   :625,633, :769,776   --linear on 8-bit pixels: the decode is a 256-entry table, encode + clamp + lround a search in 255 thresholds (trc_u8_core.h)
// Scalar math in double (`intermediate` of the reference's motion build, motion/Makefile:1-2).
#include <hip/hip_runtime.h>
#include <string.h>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <math.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <mutex>

#include "../../include/dspfft.h"
#include "motion_filter.h"
#include "trc_core.h"
#include "trc_u8_core.h"
#include "topn_core.h"

static_assert(dspfft::MOTION_MODE_NONE == DSPFFT_MOTION_NONE && dspfft::MOTION_MODE_ABS == DSPFFT_MOTION_ABS && dspfft::MOTION_MODE_SHIFT == DSPFFT_MOTION_SHIFT &&
              dspfft::MOTION_MODE_FLAT == DSPFFT_MOTION_FLAT && dspfft::MOTION_MODE_COPY == DSPFFT_MOTION_COPY, "motion_filter.h's modes are dspfft.h's");

namespace {

thread_local char g_merr[256] = "";
int mbad(const char *m) { snprintf(g_merr, sizeof g_merr, "%s", m); return -1; }
inline int mgrid(size_t n) { size_t b = (n + 255) / 256; return (int)(b < 1 ? 1 : b > 8192 ? 8192 : b); }

struct Reg { int n[3]; long long mh, mw; };
__device__ inline size_t reg_off(const Reg &r, size_t i) { const size_t x = i % r.n[2], y = (i / r.n[2]) % r.n[1], z = i / ((size_t)r.n[2] * r.n[1]); return (z * r.mh + y) * r.mw + x; }

// PIX = uint8_t (the tool's default) or float (float_pixels: motion.c:623 reads sample * 255, :774 stores pel / 255)
template <class PIX>
__global__ void motion_load_kernel(float *c, const PIX *pix, Reg r, int mode, double ic, double norm)
{
	const size_t total = (size_t)r.n[0] * r.n[1] * r.n[2];
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
		const size_t o = reg_off(r, i);
		double pel;
		if constexpr (sizeof(PIX) == 1) pel = (double)pix[o]; else pel = (double)(pix[o] * 255.0f) ;   // :623 float * int: a float product
		c[o] = (float)dspfft::motion_load_pel(pel, mode, ic, norm);                                     // :627-637
	}
}

template <class PIX>
__global__ void motion_store_kernel(PIX *pix, const float *c, Reg r, int mode, double scalefactor, double norm, double cc)
{
	const size_t total = (size_t)r.n[0] * r.n[1] * r.n[2];
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
		const size_t o = reg_off(r, i);
		const double pel = dspfft::motion_store_pel((double)c[o], mode, scalefactor, norm, cc);         // :759-771
		if constexpr (sizeof(PIX) == 1) pix[o] = pel > 255 ? 255 : pel < 0 ? 0 : (uint8_t)lround(pel);  // :776
		else pix[o] = (float)(pel / 255);                                                               // :774
	}
}

// ---- motion --spectrogram / --ispectrogram over all blocks of a batch (dspfft_motion_spec_blocks_*, dspfft_motion_ispec_blocks_*) ----
// Block b (blockIdx.y, striding) lies at b * stride; its element (z, y, x) at (z mh + y) mw + x, in the pixel and the coefficient buffer alike.
// A thread moves W = 4 consecutive samples of a row where rows and pitches are multiples of 4 and the buffers aligned, else one.
struct SpecReg { int n[3]; long long mh, mw, stride; unsigned int nblocks; };
__device__ inline void coded_add(unsigned long long mine, unsigned long long *coded)
{
	unsigned int m = (unsigned int)mine;
	for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(coded, (unsigned long long)m);
}
// motion.c:650,683-744,755-776: c is read only -- the block's element 0 is still its DC from before the filter when abs asks for it (:755)
template <class PIX, int W>
__global__ void __launch_bounds__(256) motion_spec_blocks_kernel(PIX *pix, const float *c, SpecReg r, dspfft::MotionSpec sp, dspfft::MotionFilter f, unsigned long long *coded)
{
	const uint32_t qx = (uint32_t)r.n[2] / W, per = (uint32_t)r.n[0] * r.n[1] * qx;
	unsigned long long mine = 0;
	for (uint32_t b = blockIdx.y; b < r.nblocks; b += gridDim.y) {
		const float *cb = c + (long long)b * r.stride;
		PIX *pb = pix + (long long)b * r.stride;
		const double cc = sp.mode == dspfft::MOTION_MODE_ABS ? dspfft::motion_abs_c(cb[0], sp.scalefactor, sp.norm) : sp.c;
		const dspfft::MotionFast fast = dspfft::motion_fast_of(sp.mode, sp.scalefactor, sp.norm, cc);
		for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x) {
			const uint32_t row = e / qx, x = (e - row * qx) * W, z = row / (uint32_t)r.n[1], y = row - z * (uint32_t)r.n[1];
			const long long o = ((long long)z * r.mh + y) * r.mw + x;
			float v[W];
			if constexpr (W == 4) { const float4 t = *reinterpret_cast<const float4 *>(cb + o); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
			else v[0] = cb[o];
#pragma unroll
			for (int k = 0; k < W; k++)
				if (f.enabled && (int)(x + k) < f.aw && (int)y < f.ah && (int)z < f.ad) v[k] = dspfft::motion_filter_at(f, (int)z, (int)y, (int)(x + k), v[k], mine);
			if constexpr (sizeof(PIX) == 1) {                                                                       // :759-776
				uint32_t w4 = 0;
#pragma unroll
				for (int k = 0; k < W; k++) w4 |= dspfft::motion_spec_byte(v[k], sp.mode, sp.scalefactor, sp.norm, cc, fast) << (8 * k);
				if constexpr (W == 4) *reinterpret_cast<uint32_t *>(pb + o) = w4; else pb[o] = (uint8_t)w4;
			} else {                                                                                                // :774
				double pel[W];
#pragma unroll
				for (int k = 0; k < W; k++) pel[k] = dspfft::motion_store_pel((double)v[k], sp.mode, sp.scalefactor, sp.norm, cc);
				if constexpr (W == 4) {
					float4 t; t.x = (float)(pel[0] / 255); t.y = (float)(pel[1] / 255); t.z = (float)(pel[2] / 255); t.w = (float)(pel[3] / 255);
					*reinterpret_cast<float4 *>(pb + o) = t;
				} else pb[o] = (float)(pel[0] / 255);
			}
		}
	}
	if (coded && f.enabled) coded_add(mine, coded);
}
// motion.c:621-637,650,683-744: pixel -> the coefficient it stands for -> filtered (the DC the filter keeps is the decoded one, :650)
template <class PIX, int W>
__global__ void __launch_bounds__(256) motion_ispec_blocks_kernel(float *c, const PIX *pix, SpecReg r, dspfft::MotionSpec sp, dspfft::MotionFilter f, unsigned long long *coded)
{
	const uint32_t qx = (uint32_t)r.n[2] / W, per = (uint32_t)r.n[0] * r.n[1] * qx;
	unsigned long long mine = 0;
	for (uint32_t b = blockIdx.y; b < r.nblocks; b += gridDim.y) {
		float *cb = c + (long long)b * r.stride;
		const PIX *pb = pix + (long long)b * r.stride;
		for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x) {
			const uint32_t row = e / qx, x = (e - row * qx) * W, z = row / (uint32_t)r.n[1], y = row - z * (uint32_t)r.n[1];
			const long long o = ((long long)z * r.mh + y) * r.mw + x;
			double pel[W];
			if constexpr (sizeof(PIX) == 1) {
				if constexpr (W == 4) { const uint32_t w4 = *reinterpret_cast<const uint32_t *>(pb + o); for (int k = 0; k < 4; k++) pel[k] = (double)((w4 >> (8 * k)) & 0xffu); }
				else pel[0] = (double)pb[o];
			} else {                                                                                                // :623 float * int: a float product
				if constexpr (W == 4) { const float4 t = *reinterpret_cast<const float4 *>(pb + o); pel[0] = (double)(t.x * 255.0f); pel[1] = (double)(t.y * 255.0f); pel[2] = (double)(t.z * 255.0f); pel[3] = (double)(t.w * 255.0f); }
				else pel[0] = (double)(pb[o] * 255.0f);
			}
			float v[W];
#pragma unroll
			for (int k = 0; k < W; k++) {
				v[k] = (float)dspfft::motion_load_pel(pel[k], sp.mode, sp.c, sp.norm);                                  // :627-637
				if (f.enabled && (int)(x + k) < f.aw && (int)y < f.ah && (int)z < f.ad) v[k] = dspfft::motion_filter_at(f, (int)z, (int)y, (int)(x + k), v[k], mine);
			}
			if constexpr (W == 4) { float4 t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; *reinterpret_cast<float4 *>(cb + o) = t; }
			else cb[o] = v[0];
		}
	}
	if (coded && f.enabled) coded_add(mine, coded);
}

// motion --linear with float pixels (--ispec / --spec none; copy stores alike).  The reference feeds the function a double, keeps the double
// it returns and divides by 255 outside it, so these two use trc_core.h's exact evaluation (double, the device library's pow) and not the
// production one, whose 1-ulp statement is about a float argument and a float result.
__global__ void motion_linear_kernel(float *dst, const float *src, Reg r, int store, double scalefactor, double norm, int trc)
{
	TRC_NO_CONTRACT
	const dspfft::TrcParams tp = dspfft::trc_params(trc);
	const size_t total = (size_t)r.n[0] * r.n[1] * r.n[2];
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
		const size_t o = reg_off(r, i);
		if (!store) {
			double pel = (double)(src[o] * 255.0f);                                 // :623 float * int: a float product
			pel = dspfft::trc_exact(tp, 1, pel / 255) * 255;                        // :633
			dst[o] = (float)pel;                                                    // :637
		} else {
			double pel = (double)src[o] * scalefactor * norm;                       // :759
			pel *= norm;                                                            // :767
			pel = dspfft::trc_exact(tp, 0, pel / 255) * 255;                        // :769
			dst[o] = (float)(pel / 255);                                            // :774
		}
	}
}

// motion --linear with 8-bit pixels (trc_u8_core.h): both tables lie in LDS.  The byte of a linear value is found by comparisons with the
// threshold table alone, from a single-precision guess (trc_u8_seed), so no pow runs here and the bytes are the host's exact evaluation's.
// Strided 3-D regions (the block inside its embedding; the scaled region of a `scaled != block` roundtrip) ...
struct Reg3 { int n[3]; long long sd[3], ss[3]; };
__global__ void __launch_bounds__(256) u8_trc_region_load_kernel(float *dst, const uint8_t *src, Reg3 r, const dspfft::TrcU8Tab *tab)
{
	__shared__ float lut[256];
	lut[threadIdx.x] = tab->lut[threadIdx.x];
	__syncthreads();
	const size_t total = (size_t)r.n[0] * r.n[1] * r.n[2];
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
		const long long x = (long long)(i % r.n[2]), y = (long long)((i / r.n[2]) % r.n[1]), z = (long long)(i / ((size_t)r.n[2] * r.n[1]));
		dst[z * r.sd[0] + y * r.sd[1] + x * r.sd[2]] = lut[src[z * r.ss[0] + y * r.ss[1] + x * r.ss[2]]];       // :625,633,637
	}
}
// pel = c * m0 * m1; pel *= m2: the reference's order with (scalefactor, normalization, normalization), a plain product with (mul, 1, 1)
__global__ void __launch_bounds__(256) u8_trc_region_store_kernel(uint8_t *dst, const float *src, Reg3 r, double m0, double m1, double m2, int trc, const dspfft::TrcU8Tab *tab)
{
	TRC_NO_CONTRACT
	__shared__ double thr[256];
	thr[threadIdx.x] = tab->thr[threadIdx.x];
	__syncthreads();
	const dspfft::TrcParams tp = dspfft::trc_params(trc);
	const size_t total = (size_t)r.n[0] * r.n[1] * r.n[2];
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
		const long long x = (long long)(i % r.n[2]), y = (long long)((i / r.n[2]) % r.n[1]), z = (long long)(i / ((size_t)r.n[2] * r.n[1]));
		double pel = (double)src[z * r.ss[0] + y * r.ss[1] + x * r.ss[2]] * m0 * m1;                              // :759
		pel *= m2;                                                                                                // :767
		dst[z * r.sd[0] + y * r.sd[1] + x * r.sd[2]] = (uint8_t)dspfft::trc_u8_byte_from(thr, pel, dspfft::trc_u8_seed(tp, pel));   // :769,776
	}
}
// ... and the flat pair beside dspfft_u8_to_f32 / dspfft_f32_to_u8.  vec: src is 4-byte (16-byte) and dst 16-byte (4-byte) aligned, and a
// thread moves four samples at a time; the len % 4 samples at the end, and everything of an unaligned call, go one by one.
__global__ void __launch_bounds__(256) u8_to_f32_trc_kernel(float *dst, const uint8_t *src, uint64_t len, int vec, const dspfft::TrcU8Tab *tab)
{
	__shared__ float lut[256];
	lut[threadIdx.x] = tab->lut[threadIdx.x];
	__syncthreads();
	const uint64_t nq = vec ? len / 4 : 0, stride = (uint64_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
	for (uint64_t q = t0; q < nq; q += stride) {
		const uint32_t w4 = reinterpret_cast<const uint32_t *>(src)[q];
		float4 v;
		v.x = lut[w4 & 0xffu]; v.y = lut[(w4 >> 8) & 0xffu]; v.z = lut[(w4 >> 16) & 0xffu]; v.w = lut[w4 >> 24];
		reinterpret_cast<float4 *>(dst)[q] = v;
	}
	for (uint64_t i = 4 * nq + t0; i < len; i += stride) dst[i] = lut[src[i]];
}
__global__ void __launch_bounds__(256) f32_to_u8_trc_kernel(uint8_t *dst, const float *src, double mul, uint64_t len, int vec, int trc, const dspfft::TrcU8Tab *tab)
{
	TRC_NO_CONTRACT
	__shared__ double thr[256];
	thr[threadIdx.x] = tab->thr[threadIdx.x];
	__syncthreads();
	const dspfft::TrcParams tp = dspfft::trc_params(trc);
	auto byte = [&](float c) { const double pel = (double)c * mul; return dspfft::trc_u8_byte_from(thr, pel, dspfft::trc_u8_seed(tp, pel)); };
	const uint64_t nq = vec ? len / 4 : 0, stride = (uint64_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
	for (uint64_t q = t0; q < nq; q += stride) {
		const float4 v = reinterpret_cast<const float4 *>(src)[q];
		reinterpret_cast<uint32_t *>(dst)[q] = byte(v.x) | (byte(v.y) << 8) | (byte(v.z) << 16) | (byte(v.w) << 24);
	}
	for (uint64_t i = 4 * nq + t0; i < len; i += stride) dst[i] = (uint8_t)byte(src[i]);
}

// The tables of the calls that come without a plan: built on the host once per device and function, uploaded (synchronously) on first use
// and kept for the life of the process (3 KB each).  A plan that has been given a function (dspfft_plan_set_u8_trc) brings its own.
const dspfft::TrcU8Tab *cached_tab(int trc)
{
	static std::mutex mu;
	static std::map<std::pair<int, int>, dspfft::TrcU8Tab *> cache;
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) return nullptr;
	std::lock_guard<std::mutex> lock(mu);
	auto it = cache.find({dev, trc});
	if (it != cache.end()) return it->second;
	dspfft::TrcU8Tab host, *d = nullptr;
	dspfft::trc_u8_tab_build(host, trc);
	if (hipMalloc((void **)&d, sizeof host) != hipSuccess) return nullptr;
	if (hipMemcpy(d, &host, sizeof host, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
	cache[{dev, trc}] = d;
	return d;
}

// ---- top-N by magnitude: radix select on the bits of |c| (monotone for non-negative floats) ----
// Runs too long for a workgroup's LDS (a 1920 x 1080 frame).  blockIdx.y is the run: one SelState and one histogram per run; the flag and
// rank arrays hold the runs of a launch back to back.
struct SelState { uint32_t prefix, mask, remaining, pad; };       // keys matching (key & mask) == prefix are still candidates
__global__ void topn_init_kernel(SelState *st, uint32_t *hist, uint32_t runs, uint32_t keep)
{
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)runs * 256; i += (size_t)gridDim.x * blockDim.x) {
		hist[i] = 0;
		if (i < runs) st[i] = SelState{0u, 0u, keep, 0u};
	}
}
__global__ void topn_hist_kernel(uint32_t *hist, const float *c, size_t n, long long stride, const SelState *st, int shift)
{
	__shared__ uint32_t h[256];
	h[threadIdx.x] = 0;
	__syncthreads();
	c += (long long)blockIdx.y * stride; hist += (size_t)blockIdx.y * 256; st += blockIdx.y;
	const uint32_t prefix = st->prefix, mask = st->mask;
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		const uint32_t k = __float_as_uint(fabsf(c[i]));
		if ((k & mask) == prefix) atomicAdd(&h[(k >> shift) & 255], 1u);
	}
	__syncthreads();
	if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
// one thread per run: walk the 256 bins from the top, find the bin holding the `remaining`-th largest candidate
__global__ void topn_pick_kernel(uint32_t *hist, SelState *st, int shift)
{
	if (threadIdx.x) return;
	hist += (size_t)blockIdx.y * 256; st += blockIdx.y;
	uint32_t rem = st->remaining;
	int b = 255;
	for (; b > 0; b--) { if (hist[b] >= rem) break; rem -= hist[b]; }
	st->prefix |= (uint32_t)b << shift;
	st->mask |= 255u << shift;
	st->remaining = rem;                      // how many of the candidates in bin b (and, after the last pass, equal to the threshold) to keep
	for (int i = 0; i < 256; i++) hist[i] = 0;
}
__global__ void topn_flag_kernel(uint32_t *tie, const float *c, size_t n, long long stride, const SelState *st)
{
	c += (long long)blockIdx.y * stride; tie += (size_t)blockIdx.y * n;
	const uint32_t T = st[blockIdx.y].prefix;
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
		tie[i] = __float_as_uint(fabsf(c[i])) == T ? 1u : 0u;
}
// rank: the exclusive scan of ALL the launch's flags; a tie's rank within its run is that minus the value at the run's start
__global__ void topn_apply_kernel(float *c, const uint32_t *rank, size_t n, long long stride, const SelState *st)
{
	c += (long long)blockIdx.y * stride; rank += (size_t)blockIdx.y * n;
	const uint32_t T = st[blockIdx.y].prefix, keep_ties = st[blockIdx.y].remaining, rank0 = rank[0];
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		const uint32_t k = __float_as_uint(fabsf(c[i]));
		if (!(k > T || (k == T && rank[i] - rank0 < keep_ties))) c[i] = 0.f;
	}
}
// element 0 of every run aside (restore = 0) and back (restore = 1): the roundtrip's preserve_dc = dc (motion.c:650,734)
__global__ void topn_dc_kernel(float *c, long long stride, float *save, size_t nblocks, int restore)
{
	for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < nblocks; r += (size_t)gridDim.x * blockDim.x) {
		if (restore) c[(long long)r * stride] = save[r]; else save[r] = c[(long long)r * stride];
	}
}

// Runs of up to TOPN_LDS_MAX floats: topn_core.h's selection, the code the fused block kernel runs (block_topn.hip).  A wave owns a run
// (runs below 64 floats: 64 / L of them share a wave) in an LDS area of its own; every lane loads, selects over and stores the elements
// e = sl, sl + L, ... of its run, so no lane reads what another wrote and the kernel needs no barrier.
// LDS is here a per-lane staging area only, and at 4096 floats a run it is 64 KB a workgroup (two workgroups per CU): the price of running
// the one selection routine the fused kernel runs, which takes its keys from and zeroes its losers in LDS.
enum { TOPN_LDS_MAX = 4096, TOPN_THREADS = 256 };
template <int K>
__global__ void __launch_bounds__(TOPN_THREADS) topn_blocks_lds_kernel(float *c, int count, size_t nblocks, long long stride, uint32_t keep, int L, int restore_dc)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char topn_lds_raw[];
	const int lane = threadIdx.x & 63, sl = lane & (L - 1), per_wave = 64 / L, slot = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * per_wave + lane / L;
	const size_t per_wg = (size_t)(TOPN_THREADS / 64) * per_wave;
	float *mine = reinterpret_cast<float *>(topn_lds_raw) + (size_t)slot * count;
	for (size_t r0 = blockIdx.x * per_wg; r0 < nblocks; r0 += gridDim.x * per_wg) {       // (uniform over the workgroup)
		const size_t r = r0 + slot;
		const bool active = r < nblocks;
		float *g = c + (long long)(active ? r : r0) * stride;
		if (active) for (int e = sl; e < count; e += L) mine[e] = g[e];
		const bool lead = restore_dc && active && sl == 0;
		float dc = 0.f;
		if (lead) dc = mine[0];
		dspfft::topn_select_lds<K, 0>(mine, 0, count, keep, L, active);
		if (lead) mine[0] = dc;
		if (active) for (int e = sl; e < count; e += L) g[e] = mine[e];
	}
}

size_t scan_temp(size_t n)
{
	size_t b = 0;
	uint32_t *p = nullptr;
	(void)rocprim::exclusive_scan(nullptr, b, p, p, 0u, n, rocprim::plus<uint32_t>(), (hipStream_t)nullptr);
	return b + 256;
}

}  // namespace

extern "C" const char *dspfft_motion_last_error(void) { return g_merr; }
extern "C" __attribute__((visibility("hidden"))) int dspfft_motion_set_error(const char *m) { return mbad(m); }   // (motion_dither.hip)
extern "C" __attribute__((visibility("hidden"))) const void *dspfft_u8_trc_cached_tab(int trc) { return cached_tab(trc); }   // (motion_dither.hip, block_trc.hip)

extern "C" int dspfft_motion_load_u8(float *d_coeffs, const uint8_t *d_pix, const int n[3], const int minbuf_hw[2], int ispec_mode, double ic, double normalization, void *stream)
{
	if (!d_coeffs || !d_pix || !n || !minbuf_hw || n[0] < 1 || n[1] < 1 || n[2] < 1 || minbuf_hw[0] < n[1] || minbuf_hw[1] < n[2]) return mbad("bad arguments");
	if (ispec_mode != DSPFFT_MOTION_NONE && ispec_mode != DSPFFT_MOTION_SHIFT && ispec_mode != DSPFFT_MOTION_FLAT && ispec_mode != DSPFFT_MOTION_COPY) return mbad("ispec mode: none, shift, flat or copy");
	Reg r; r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2]; r.mh = minbuf_hw[0]; r.mw = minbuf_hw[1];
	hipLaunchKernelGGL(motion_load_kernel<uint8_t>, dim3(mgrid((size_t)n[0] * n[1] * n[2])), dim3(256), 0, (hipStream_t)stream, d_coeffs, d_pix, r, ispec_mode, ic, normalization);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int dspfft_motion_load_f32(float *d_coeffs, const float *d_pix, const int n[3], const int minbuf_hw[2], int ispec_mode, double ic, double normalization, void *stream)
{
	if (!d_coeffs || !d_pix || !n || !minbuf_hw || n[0] < 1 || n[1] < 1 || n[2] < 1 || minbuf_hw[0] < n[1] || minbuf_hw[1] < n[2]) return mbad("bad arguments");
	if (ispec_mode != DSPFFT_MOTION_NONE && ispec_mode != DSPFFT_MOTION_SHIFT && ispec_mode != DSPFFT_MOTION_FLAT && ispec_mode != DSPFFT_MOTION_COPY) return mbad("ispec mode: none, shift, flat or copy");
	Reg r; r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2]; r.mh = minbuf_hw[0]; r.mw = minbuf_hw[1];
	hipLaunchKernelGGL(motion_load_kernel<float>, dim3(mgrid((size_t)n[0] * n[1] * n[2])), dim3(256), 0, (hipStream_t)stream, d_coeffs, d_pix, r, ispec_mode, ic, normalization);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int dspfft_motion_store_u8(uint8_t *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], int spec_mode,
                                      double scalefactor, double normalization, double c, void *stream)
{
	if (!d_coeffs || !d_pix || !n || !minbuf_hw || n[0] < 1 || n[1] < 1 || n[2] < 1 || minbuf_hw[0] < n[1] || minbuf_hw[1] < n[2]) return mbad("bad arguments");
	if (spec_mode < DSPFFT_MOTION_NONE || spec_mode > DSPFFT_MOTION_COPY) return mbad("spec mode: none, abs, shift, flat or copy");
	Reg r; r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2]; r.mh = minbuf_hw[0]; r.mw = minbuf_hw[1];
	hipLaunchKernelGGL(motion_store_kernel<uint8_t>, dim3(mgrid((size_t)n[0] * n[1] * n[2])), dim3(256), 0, (hipStream_t)stream, d_pix, d_coeffs, r, spec_mode, scalefactor, normalization, c);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int dspfft_motion_store_f32(float *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], int spec_mode,
                                       double scalefactor, double normalization, double c, void *stream)
{
	if (!d_coeffs || !d_pix || !n || !minbuf_hw || n[0] < 1 || n[1] < 1 || n[2] < 1 || minbuf_hw[0] < n[1] || minbuf_hw[1] < n[2]) return mbad("bad arguments");
	if (spec_mode < DSPFFT_MOTION_NONE || spec_mode > DSPFFT_MOTION_COPY) return mbad("spec mode: none, abs, shift, flat or copy");
	Reg r; r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2]; r.mh = minbuf_hw[0]; r.mw = minbuf_hw[1];
	hipLaunchKernelGGL(motion_store_kernel<float>, dim3(mgrid((size_t)n[0] * n[1] * n[2])), dim3(256), 0, (hipStream_t)stream, d_pix, d_coeffs, r, spec_mode, scalefactor, normalization, c);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

namespace {
template <class PIX, int W>
void spec_blocks_launch(bool inverse, void *pix, void *c, const SpecReg &r, const dspfft::MotionSpec &sp, const dspfft::MotionFilter &f, unsigned long long *coded, hipStream_t s)
{
	const size_t per = (size_t)r.n[0] * r.n[1] * (r.n[2] / W);
	const dim3 grid((unsigned)std::min<size_t>((per + 255) / 256, 4096), std::min(r.nblocks, 65535u));
	if (inverse) hipLaunchKernelGGL((motion_ispec_blocks_kernel<PIX, W>), grid, dim3(256), 0, s, (float *)c, (const PIX *)pix, r, sp, f, coded);
	else hipLaunchKernelGGL((motion_spec_blocks_kernel<PIX, W>), grid, dim3(256), 0, s, (PIX *)pix, (const float *)c, r, sp, f, coded);
}
int spec_blocks_call(bool inverse, bool u8, void *d_pix, void *d_coeffs, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                     const dspfft_motion_spec_params *spp, const dspfft_motion_filter_params *fp, unsigned long long *d_coded, void *stream)
{
	if (!d_coeffs || !d_pix || !n || !minbuf_hw || !spp || !nblocks || n[0] < 1 || n[1] < 1 || n[2] < 1 || minbuf_hw[0] < n[1] || minbuf_hw[1] < n[2]) return mbad("bad arguments");
	const int m = spp->mode;
	if (m < DSPFFT_MOTION_NONE || m > DSPFFT_MOTION_COPY || (inverse && m == DSPFFT_MOTION_ABS)) return mbad(inverse ? "ispec mode: none, shift, flat or copy" : "spec mode: none, abs, shift, flat or copy");
	if ((unsigned long long)n[0] * n[1] * n[2] >= (1ull << 32) || nblocks >= (1ull << 32)) return mbad("a block of 2^32 samples or more, or 2^32 blocks or more");
	SpecReg r; r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2]; r.mh = minbuf_hw[0]; r.mw = minbuf_hw[1]; r.stride = nblocks > 1 ? block_stride : 0; r.nblocks = (unsigned int)nblocks;
	if (nblocks > 1 && block_stride < ((long long)(n[0] - 1) * r.mh + n[1] - 1) * r.mw + n[2]) return mbad("the blocks overlap (block_stride < a block's span)");
	if (fp && (fp->preserve_dc < 0 || fp->preserve_dc > 2 || fp->minbuf_hw[0] < 1 || fp->minbuf_hw[1] < 1 || fp->block_depth < 1)) return mbad("bad filter parameters");
	dspfft::MotionFilter f;
	memset((void *)&f, 0, sizeof f);
	if (fp) dspfft::motion_filter_from(*fp, f);
	const dspfft::MotionSpec sp = {m, spp->scalefactor, spp->normalization, spp->c};
	const bool vec = n[2] % 4 == 0 && r.mw % 4 == 0 && r.stride % 4 == 0 && !((uintptr_t)d_pix & (u8 ? 3u : 15u)) && !((uintptr_t)d_coeffs & 15u);
	hipStream_t s = (hipStream_t)stream;
	if (u8) { if (vec) spec_blocks_launch<uint8_t, 4>(inverse, d_pix, d_coeffs, r, sp, f, d_coded, s); else spec_blocks_launch<uint8_t, 1>(inverse, d_pix, d_coeffs, r, sp, f, d_coded, s); }
	else { if (vec) spec_blocks_launch<float, 4>(inverse, d_pix, d_coeffs, r, sp, f, d_coded, s); else spec_blocks_launch<float, 1>(inverse, d_pix, d_coeffs, r, sp, f, d_coded, s); }
	return hipGetLastError() == hipSuccess ? 0 : -4;
}
}  // namespace

extern "C" int dspfft_motion_spec_blocks_u8(uint8_t *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                            const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_blocks_call(false, true, d_pix, (void *)d_coeffs, n, minbuf_hw, nblocks, block_stride, sp, filter, d_coeffs_coded, stream);
}
extern "C" int dspfft_motion_spec_blocks_f32(float *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                             const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_blocks_call(false, false, d_pix, (void *)d_coeffs, n, minbuf_hw, nblocks, block_stride, sp, filter, d_coeffs_coded, stream);
}
extern "C" int dspfft_motion_ispec_blocks_u8(float *d_coeffs, const uint8_t *d_pix, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                             const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_blocks_call(true, true, (void *)d_pix, d_coeffs, n, minbuf_hw, nblocks, block_stride, sp, filter, d_coeffs_coded, stream);
}
extern "C" int dspfft_motion_ispec_blocks_f32(float *d_coeffs, const float *d_pix, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                              const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_blocks_call(true, false, (void *)d_pix, d_coeffs, n, minbuf_hw, nblocks, block_stride, sp, filter, d_coeffs_coded, stream);
}

/* the same for dspfft_execute_spectrogram_* / _ispectrogram_* (engine.cpp reaches this through a weak reference); the error text is
 * dspfft_motion_last_error's */
extern "C" __attribute__((visibility("hidden"))) int dspfft_spec_blocks_launch(int inverse, int u8, void *d_pix, void *d_coeffs, const int n[3], const int minbuf_hw[2], size_t nblocks,
                                                                                long long block_stride, const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter,
                                                                                unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_blocks_call(inverse != 0, u8 != 0, d_pix, d_coeffs, n, minbuf_hw, nblocks, block_stride, sp, filter, d_coeffs_coded, stream);
}

/* dspfft_motion_{load,store}_f32_linear's body (engine.cpp has checked the arguments and reaches this through a weak reference) */
extern "C" __attribute__((visibility("hidden"))) int dspfft_motion_linear_launch(float *d_dst, const float *d_src, const int n[3], const int minbuf_hw[2], int store,
                                                                                  double scalefactor, double normalization, int trc, void *stream)
{
	Reg r; r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2]; r.mh = minbuf_hw[0]; r.mw = minbuf_hw[1];
	hipLaunchKernelGGL(motion_linear_kernel, dim3(mgrid((size_t)n[0] * n[1] * n[2])), dim3(256), 0, (hipStream_t)stream, d_dst, d_src, r, store, scalefactor, normalization, trc);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

/* The 8-bit --linear launchers (engine.cpp has checked the arguments and reaches these through weak references).  tab: the device tables of
 * a plan (dspfft_plan_set_u8_trc), or NULL for this file's own.  store = 0: dst floats = lut[src bytes]; 1: dst bytes from src floats. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_u8_trc_flat_launch(void *d_dst, const void *d_src, double mul, uint64_t len, int store, int trc, const void *tab, void *stream)
{
	const dspfft::TrcU8Tab *t = tab ? (const dspfft::TrcU8Tab *)tab : cached_tab(trc);
	if (!t) return -4;
	if (!len) return 0;
	const uintptr_t p8 = (uintptr_t)(store ? d_dst : d_src), pf = (uintptr_t)(store ? d_src : d_dst);
	const int vec = !(p8 & 3u) && !(pf & 15u);
	const dim3 grid(mgrid(vec ? (len + 3) / 4 : len));
	if (store) hipLaunchKernelGGL(f32_to_u8_trc_kernel, grid, dim3(256), 0, (hipStream_t)stream, (uint8_t *)d_dst, (const float *)d_src, mul, len, vec, trc, t);
	else hipLaunchKernelGGL(u8_to_f32_trc_kernel, grid, dim3(256), 0, (hipStream_t)stream, (float *)d_dst, (const uint8_t *)d_src, len, vec, t);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}
extern "C" __attribute__((visibility("hidden"))) int dspfft_u8_trc_region_launch(void *d_dst, const void *d_src, const int n[3], const long long sdst[3], const long long ssrc[3], int store,
                                                                                  double m0, double m1, double m2, int trc, const void *tab, void *stream)
{
	const dspfft::TrcU8Tab *t = tab ? (const dspfft::TrcU8Tab *)tab : cached_tab(trc);
	if (!t) return -4;
	Reg3 r;
	for (int k = 0; k < 3; k++) { r.n[k] = n[k]; r.sd[k] = sdst[k]; r.ss[k] = ssrc[k]; }
	const dim3 grid(mgrid((size_t)n[0] * n[1] * n[2]));
	if (store) hipLaunchKernelGGL(u8_trc_region_store_kernel, grid, dim3(256), 0, (hipStream_t)stream, (uint8_t *)d_dst, (const float *)d_src, r, m0, m1, m2, trc, t);
	else hipLaunchKernelGGL(u8_trc_region_load_kernel, grid, dim3(256), 0, (hipStream_t)stream, (float *)d_dst, (const uint8_t *)d_src, r, t);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

namespace {
// ---- the global path's work area: [R SelStates | R histograms] rounded to 4 KB, R * count flags, R * count ranks, the scan's storage ----
// R runs go through one set of launches: as many as 2^26 elements' worth (512 MB of flags and ranks), at most 65535 (gridDim.y)
size_t topn_runs_per_launch(size_t count, size_t nblocks) { return std::max<size_t>(1, std::min(std::min<size_t>(nblocks, 65535), ((size_t)1 << 26) / count)); }
size_t topn_head_bytes(size_t R) { return (((R * sizeof(SelState) + 255) & ~(size_t)255) + R * 1024 + 4095) & ~(size_t)4095; }
size_t topn_slab_bytes(size_t count, size_t R) { return (R * count * 4 + 255) & ~(size_t)255; }
size_t topn_global_bytes(size_t count, size_t R) { return topn_head_bytes(R) + 2 * topn_slab_bytes(count, R) + scan_temp(R * count); }

int topn_global(float *c, size_t count, size_t nblocks, long long stride, size_t keep, char *base, hipStream_t s)
{
	const size_t R = topn_runs_per_launch(count, nblocks);
	const size_t slab = topn_slab_bytes(count, R);
	SelState *st = (SelState *)base;
	uint32_t *hist = (uint32_t *)(base + ((R * sizeof(SelState) + 255) & ~(size_t)255));
	uint32_t *tie = (uint32_t *)(base + topn_head_bytes(R)), *rank = (uint32_t *)(base + topn_head_bytes(R) + slab);
	void *temp = base + topn_head_bytes(R) + 2 * slab;
	size_t tb = scan_temp(R * count);
	for (size_t r0 = 0; r0 < nblocks; r0 += R) {
		const uint32_t runs = (uint32_t)std::min(R, nblocks - r0);
		float *c0 = c + (long long)r0 * stride;
		const dim3 grid(mgrid(count), runs);
		hipLaunchKernelGGL(topn_init_kernel, dim3(mgrid((size_t)runs * 256)), dim3(256), 0, s, st, hist, runs, (uint32_t)keep);
		for (int shift = 24; shift >= 0; shift -= 8) {
			hipLaunchKernelGGL(topn_hist_kernel, grid, dim3(256), 0, s, hist, c0, count, stride, st, shift);
			hipLaunchKernelGGL(topn_pick_kernel, dim3(1, runs), dim3(64), 0, s, hist, st, shift);
		}
		// elements equal to the threshold: the first `remaining` of them in buffer order are kept (the reference leaves ties to qsort)
		hipLaunchKernelGGL(topn_flag_kernel, grid, dim3(256), 0, s, tie, c0, count, stride, st);
		if (rocprim::exclusive_scan(temp, tb, tie, rank, 0u, (size_t)runs * count, rocprim::plus<uint32_t>(), s) != hipSuccess) return -4;
		hipLaunchKernelGGL(topn_apply_kernel, grid, dim3(256), 0, s, c0, rank, count, stride, st);
	}
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

template <int K>
int topn_lds_launch(float *c, size_t count, size_t nblocks, long long stride, size_t keep, int L, int restore_dc, hipStream_t s)
{
	const size_t per_wg = (size_t)(TOPN_THREADS / 64) * (64 / L), lds = per_wg * count * sizeof(float);
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(topn_blocks_lds_kernel<K>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return -4;
	const size_t nwg = std::min<size_t>((nblocks + per_wg - 1) / per_wg, 1u << 20);
	hipLaunchKernelGGL(topn_blocks_lds_kernel<K>, dim3((unsigned)nwg), dim3(TOPN_THREADS), lds, s, c, (int)count, nblocks, stride, (uint32_t)keep, L, restore_dc);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

size_t topn_blocks_bytes(size_t count, size_t nblocks)
{
	if (count <= TOPN_LDS_MAX) return 0;
	return topn_global_bytes(count, topn_runs_per_launch(count, nblocks)) + ((nblocks * 4 + 255) & ~(size_t)255);
}

// the arguments have been checked; 0 < keep < count
int topn_blocks_run(float *c, size_t count, size_t nblocks, long long stride, size_t keep, void *d_work, int restore_dc, hipStream_t s)
{
	if (count <= TOPN_LDS_MAX) {
		int L = 64;
		while (L / 2 >= (int)count) L /= 2;
		const size_t k = (count + 63) / 64;
		if (k <= 1) return topn_lds_launch<1>(c, count, nblocks, stride, keep, L, restore_dc, s);
		if (k <= 4) return topn_lds_launch<4>(c, count, nblocks, stride, keep, L, restore_dc, s);
		if (k <= 8) return topn_lds_launch<8>(c, count, nblocks, stride, keep, L, restore_dc, s);
		if (k <= 16) return topn_lds_launch<16>(c, count, nblocks, stride, keep, L, restore_dc, s);
		if (k <= 32) return topn_lds_launch<32>(c, count, nblocks, stride, keep, L, restore_dc, s);
		return topn_lds_launch<64>(c, count, nblocks, stride, keep, L, restore_dc, s);
	}
	const size_t R = topn_runs_per_launch(count, nblocks);
	float *dcs = (float *)((char *)d_work + topn_global_bytes(count, R));
	if (restore_dc) hipLaunchKernelGGL(topn_dc_kernel, dim3(mgrid(nblocks)), dim3(256), 0, s, c, stride, dcs, nblocks, 0);
	if (int rc = topn_global(c, count, nblocks, stride, keep, (char *)d_work, s)) return rc;
	if (restore_dc) hipLaunchKernelGGL(topn_dc_kernel, dim3(mgrid(nblocks)), dim3(256), 0, s, c, stride, dcs, nblocks, 1);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace

extern "C" size_t dspfft_motion_topn_work_bytes(size_t count) { return 2 * ((count * 4 + 255) & ~(size_t)255) + 4096 + scan_temp(count); }

extern "C" int dspfft_motion_topn(float *d_coeffs, size_t count, size_t keep, void *d_work, size_t work_bytes, void *stream)
{
	if (!d_coeffs || !d_work || !count) return mbad("bad arguments");
	if (work_bytes < dspfft_motion_topn_work_bytes(count)) return mbad("work buffer too small: dspfft_motion_topn_work_bytes");
	if (count >= (1ull << 32)) return mbad("top-N select addresses the buffer with 32-bit counts");
	hipStream_t s = (hipStream_t)stream;
	if (keep >= count) return 0;
	if (!keep) return hipMemsetAsync(d_coeffs, 0, count * 4, s) == hipSuccess ? 0 : -4;
	return topn_global(d_coeffs, count, 1, (long long)count, keep, (char *)d_work, s);     // one run: the work area is the one this call has always had
}

extern "C" size_t dspfft_motion_topn_blocks_work_bytes(size_t count, size_t nblocks)
{
	if (!count || !nblocks || count >= (1ull << 32)) return 0;
	return topn_blocks_bytes(count, nblocks);
}

static int topn_blocks_checked(float *d_coeffs, size_t count, size_t nblocks, long long block_stride, size_t keep, void *d_work, size_t work_bytes, int restore_dc, void *stream)
{
	if (!d_coeffs || !count || !nblocks) return mbad("bad arguments");
	if (count >= (1ull << 32)) return mbad("top-N select addresses a run with 32-bit counts");
	if (nblocks > 1 && (block_stride < 0 || (unsigned long long)block_stride < count)) return mbad("top-N select: the runs overlap (block_stride < count)");
	hipStream_t s = (hipStream_t)stream;
	if (keep >= count) return 0;
	if (!keep) return hipMemset2DAsync(d_coeffs, (nblocks > 1 ? (size_t)block_stride : count) * 4, 0, count * 4, nblocks, s) == hipSuccess ? 0 : -4;
	const size_t need = topn_blocks_bytes(count, nblocks);
	if (need && !d_work) return mbad("bad arguments: runs of this length need a work buffer (dspfft_motion_topn_blocks_work_bytes)");
	if (work_bytes < need) return mbad("work buffer too small: dspfft_motion_topn_blocks_work_bytes");
	return topn_blocks_run(d_coeffs, count, nblocks, nblocks > 1 ? block_stride : (long long)count, keep, d_work, restore_dc, s);
}

extern "C" int dspfft_motion_topn_blocks(float *d_coeffs, size_t count, size_t nblocks, long long block_stride, size_t keep, void *d_work, size_t work_bytes, void *stream)
{
	return topn_blocks_checked(d_coeffs, count, nblocks, block_stride, keep, d_work, work_bytes, 0, stream);
}

/* the roundtrip's selection stage (engine.cpp reaches the two through weak references): restore_dc puts every run's element 0 back as it was
 * before the selection.  The error text is dspfft_motion_last_error's. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_topn_blocks_launch(float *d_coeffs, size_t count, size_t nblocks, long long block_stride, size_t keep,
                                                                                void *d_work, size_t work_bytes, int restore_dc, void *stream)
{
	return topn_blocks_checked(d_coeffs, count, nblocks, block_stride, keep, d_work, work_bytes, restore_dc, stream);
}
extern "C" __attribute__((visibility("hidden"))) size_t dspfft_topn_blocks_bytes(size_t count, size_t nblocks) { return dspfft_motion_topn_blocks_work_bytes(count, nblocks); }
