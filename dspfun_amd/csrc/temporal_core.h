// temporal_core.h -- motion -b 1x1xD (with -s 1x1xD'): blocks that exist only along time (motion/README.md:87-89, `--blocksize 1x1x0`;
// motion/motion.c:488-499,535-552,613-776 with block = {D, 1, 1}), the phases of temporal_rt.hip's kernel.  Every pixel of every run of D
// frames of a [frames][H][W] plane is a 1-D block: REDFT10 over D, the filter by z, REDFT01 over D' = `scaled`, all at stride P = H W.
//
// One workgroup takes one block in time and K consecutive pixel columns.  Its LDS tile is max(D, D') x K floats, seen as max(D, D') rows of
// B = K / 2 complex slots: two neighbouring pixel columns are one complex signal, as in the runtime-geometry column pass (dct_core.h, COL),
// whose arithmetic and stage tables these phases use for every length from 2 up:
//   load       D rows from the INPUT layout (float4, or four packed bytes, plain or through motion --linear's decode table), even/odd
//              reordered along time (col_load2)
//   stages     the forward plan's FFT stages, in place (fft_stage)
//   post       two real transforms out of one complex one, quarter-sample twiddle, the plan's scales (col_post2), then the filter at
//              (z, 0, 0) for z < min(D, D') -- back into the tile in NATURAL row order.  An item reads slots pos[k], pos[D - k] and writes
//              rows k, D - k, which other items still have to read: every thread first reads all its items into registers
//              (temporal_post_read), the workgroup meets at a barrier, then it computes and writes (temporal_post_write)
//   pre        rows k, D' - k -> the conjugate spectrum of the inverse (col_pre3); rows at or beyond min(D, D') read as zeros (upscaling:
//              zero padding, :619; downscaling never asks for them).  In place: an item writes the two slots it has read
//   stages     the inverse plan's FFT stages
//   store      both real signals, un-reordered, scaled (col_unpack3), four samples per thread into the OUTPUT layout: float4, the
//              quantised bytes (value x mul8, clamp, lround: :776) or the encoded bytes of motion --linear
// The last tile of a frame is short (P is a multiple of 4, so a group of four columns is whole or absent): absent columns load as zeros,
// are never filtered -- a grey DC would count as coded -- and never stored.
// Plain C++17 for device (hipcc) and host (g++: tests/test_motion_temporal_cpu.py runs the phases thread by thread).
#pragma once
#include "block_core.h"

namespace dspfft {

enum {
	TEMPORAL_TILE_BYTES = 64 * 1024,   // the tile's budget: with the tables behind it two workgroups share a CU's 160 KB
	TEMPORAL_BATCH = 8,                // global loads a thread issues before it uses the first
	TEMPORAL_HOLD = 9                  // post items a thread holds across the barrier: (D / 2 + 1) B <= TEMPORAL_HOLD x threads
};

struct TemporalArgs {
	int D, S;                     // forward / inverse lengths (`block`, `scaled` along time)
	int K, B;                     // tile width in samples (a multiple of 4) and in complex slots
	int P, ntiles;                // samples per frame; ceil(P / K)
	long long blk_in, blk_out;    // between blocks in time: D P, S P
	const float *in;
	float *out;
	const uint8_t *in8;           // replace in / out when set (8-bit samples in the same element layout)
	uint8_t *out8;
	double mul8;
	FftDesc ff, fi;               // the two complex FFTs (lengths D and S) ...
	const cx<float> *Tf, *Wf, *Ti, *Wi;     // ... their tables (PassArgsT's T and W) ...
	const uint32_t *posf, *posi;  // ... and digit reversals
	float f_scale, f_in0, f_out0, i_scale, i_in0, i_out0;   // the plans' scales
	MotionFilter filt;            // filt.enabled = 0: none
	unsigned long long *coded;
	const TrcU8Tab *tab_in, *tab_out;       // motion --linear at the 8-bit ends (NULL: that end converts plainly)
	int trc_out;
	FastDiv divB, divQ, div_tiles;          // divide by B, by K / 4, by ntiles
};

DSP_HD size_t temporal_tile_bytes(const TemporalArgs &a) { return (size_t)(a.D > a.S ? a.D : a.S) * a.K * sizeof(float); }
// tile width and threads for a pair of lengths (engine.cpp and the tests): the widest K of 128, 64, 32, 16 within the budget; 0: too long
DSP_HD int temporal_tile_k(int m) { int k = 128; while (k > 16 && (size_t)m * k * sizeof(float) > TEMPORAL_TILE_BYTES) k >>= 1; return (size_t)m * k * sizeof(float) > TEMPORAL_TILE_BYTES ? 0 : k; }
DSP_HD int temporal_threads(int m, int k) { return m * k > 8192 ? 512 : 256; }

// workgroup -> (block in time, tile of the frame)
DSP_HD void temporal_base(const TemporalArgs &a, uint32_t wg, long long &bin, long long &bout, int &valid)
{
	const uint32_t blk = a.div_tiles.div_exact(wg), t = wg - blk * (uint32_t)a.ntiles;
	bin = (long long)blk * a.blk_in + (long long)t * a.K;
	bout = (long long)blk * a.blk_out + (long long)t * a.K;
	valid = a.P - (int)t * a.K;
	if (valid > a.K) valid = a.K;
}

// ---- load: item = (frame y, four columns q) ----
template <bool U8, bool TRC>
DSP_HD void temporal_load(const TemporalArgs &a, cx<float> *buf, long long bin, int valid, int tid, int nthr, const float *lut)
{
	const int Q = a.K >> 2, total = a.D * Q;
	float *bf = reinterpret_cast<float *>(buf);
	for (int it0 = tid; it0 < total; it0 += TEMPORAL_BATCH * nthr) {
		float4 v[TEMPORAL_BATCH];
		uint32_t w[TEMPORAL_BATCH];
		// all of a batch's loads before the first use
#pragma unroll
		for (int u = 0; u < TEMPORAL_BATCH; u++) {
			const int it = it0 + u * nthr;
			w[u] = 0; v[u].x = v[u].y = v[u].z = v[u].w = 0.f;
			if (it < total) {
				const int y = (int)a.divQ.div((uint32_t)it), q = it - y * Q;
				if (4 * q < valid) {
					const long long off = bin + (long long)y * a.P + 4 * q;
					if constexpr (U8) __builtin_memcpy(&w[u], a.in8 + off, 4);
					else v[u] = *reinterpret_cast<const float4 *>(a.in + off);
				}
			}
		}
#pragma unroll
		for (int u = 0; u < TEMPORAL_BATCH; u++) {
			const int it = it0 + u * nthr;
			if (it < total) {
				const int y = (int)a.divQ.div((uint32_t)it), q = it - y * Q;
				float4 x = v[u];
				if constexpr (U8) {
					if (4 * q < valid) {
						if constexpr (TRC) { x.x = lut[w[u] & 0xffu]; x.y = lut[(w[u] >> 8) & 0xffu]; x.z = lut[(w[u] >> 16) & 0xffu]; x.w = lut[w[u] >> 24]; }
						else { x.x = (float)(w[u] & 0xffu); x.y = (float)((w[u] >> 8) & 0xffu); x.z = (float)((w[u] >> 16) & 0xffu); x.w = (float)(w[u] >> 24); }
					}
				}
				if (y == 0) { x.x *= a.f_in0; x.y *= a.f_in0; x.z *= a.f_in0; x.w *= a.f_in0; }
				*reinterpret_cast<float4 *>(bf + (size_t)makhoul_dst(y, a.D) * a.K + 4 * q) = x;
			}
		}
	}
}
// lut: the decode table of motion --linear (8-bit input only), or NULL
DSP_HD void temporal_phase_load(const TemporalArgs &a, cx<float> *buf, long long bin, int valid, int tid, int nthr, const float *lut)
{
	if (!a.in8) temporal_load<false, false>(a, buf, bin, valid, tid, nthr, lut);
	else if (lut) temporal_load<true, true>(a, buf, bin, valid, tid, nthr, lut);
	else temporal_load<true, false>(a, buf, bin, valid, tid, nthr, lut);
}

DSP_HD void temporal_stage(const TemporalArgs &a, cx<float> *buf, bool inverse, int s, int tid, int nthr)
{
	if (inverse) fft_stage(buf, a.S, a.fi.st[s], a.B, a.divB, a.Wi, tid, nthr);
	else fft_stage(buf, a.D, a.ff.st[s], a.B, a.divB, a.Wf, tid, nthr);
}

// ---- post: item = (k in [0, D / 2], column pair j) ----
struct TemporalHeld { cx<float> zk[TEMPORAL_HOLD], zm[TEMPORAL_HOLD]; };

DSP_HD void temporal_post_read(const TemporalArgs &a, const cx<float> *buf, int valid, int tid, int nthr, TemporalHeld &h)
{
	const int total = (a.D / 2 + 1) * a.B;
#pragma unroll
	for (int u = 0; u < TEMPORAL_HOLD; u++) {
		const int it = tid + u * nthr;
		h.zk[u] = h.zm[u] = cmk<float>(0.f, 0.f);
		if (it < total) {
			const int k = (int)a.divB.div((uint32_t)it), j = it - k * a.B;
			if (2 * j < valid) {
				h.zk[u] = buf[a.posf[k] * a.B + j];
				h.zm[u] = buf[a.posf[k ? a.D - k : 0] * a.B + j];
			}
		}
	}
}
// the filter over the two pixels of a slot at row z (motion.c:683-744 at (z, 0, 0))
DSP_HD cx<float> temporal_filter(const MotionFilter &f, int z, cx<float> v, unsigned long long &coded)
{
	v.x = motion_filter_at(f, z, 0, 0, v.x, coded);
	v.y = motion_filter_at(f, z, 0, 0, v.y, coded);
	return v;
}
DSP_HD void temporal_post_write(const TemporalArgs &a, cx<float> *buf, int valid, int tid, int nthr, const TemporalHeld &h, unsigned long long &coded)
{
	typedef cx<float> C_;
	const int total = (a.D / 2 + 1) * a.B;
	// rows the filter sees: the active corner (motion.c:644-647 onwards work on min(block, scaled))
	int act = a.D < a.S ? a.D : a.S;
	if (a.filt.enabled && a.filt.ad < act) act = a.filt.ad;
	const bool filt = a.filt.enabled && a.filt.ah > 0 && a.filt.aw > 0;
#pragma unroll
	for (int u = 0; u < TEMPORAL_HOLD; u++) {
		const int it = tid + u * nthr;
		if (it < total) {
			const int k = (int)a.divB.div((uint32_t)it), j = it - k * a.B;
			if (2 * j < valid) {
				const int km = k ? a.D - k : 0;
				const C_ zk = h.zk[u], zm = cconj(h.zm[u]);
				const C_ A2 = cadd(zk, zm);                   // 2 A[k]
				const C_ B2 = cmul_mi(csub(zk, zm));          // 2 B[k]
				const C_ t = a.Tf[k];
				const C_ wa = cmul(t, A2), wb = cmul(t, B2);
				const float sc = a.f_scale, s0 = (k == 0) ? sc * a.f_out0 : sc;
				C_ rk = cmk<float>(wa.x * s0, wb.x * s0);
				if (filt && k < act) rk = temporal_filter(a.filt, k, rk, coded);
				buf[k * a.B + j] = rk;
				if (k > 0 && km != k) {
					C_ rm = cmk<float>(-wa.y * sc, -wb.y * sc);
					if (filt && km < act) rm = temporal_filter(a.filt, km, rm, coded);
					buf[km * a.B + j] = rm;
				}
			}
		}
	}
}

// ---- pre: item = (k in [0, S / 2], column pair j); in place ----
DSP_HD void temporal_pre(const TemporalArgs &a, cx<float> *buf, int valid, int tid, int nthr)
{
	typedef cx<float> C_;
	const int S = a.S, B = a.B, total = (S / 2 + 1) * B, act = a.D < S ? a.D : S;
	for (int it = tid; it < total; it += nthr) {
		const int k = (int)a.divB.div((uint32_t)it), j = it - k * B;
		if (2 * j >= valid) continue;
		const int km = k ? S - k : 0;
		C_ xk = k < act ? buf[k * B + j] : cmk<float>(0.f, 0.f);
		const C_ xm = (k && km < act) ? buf[km * B + j] : cmk<float>(0.f, 0.f);
		if (k == 0) { xk.x *= a.i_in0; xk.y *= a.i_in0; }
		const C_ t = a.Ti[k];
		const C_ Va = cmulc(cmk<float>(xk.x, -xm.x), t);     // conj(T[k]) (Xa[k] - i Xa[S-k])
		const C_ Vb = cmulc(cmk<float>(xk.y, -xm.y), t);
		buf[k * B + j] = cmk<float>(Va.x - Vb.y, -Va.y - Vb.x);            // conj(Va) - i conj(Vb)
		if (k > 0) buf[km * B + j] = cmk<float>(Va.x + Vb.y, Va.y - Vb.x); // Va - i Vb
	}
}

// ---- store: item = (frame y, four columns q) ----
template <bool U8, bool TRC>
DSP_HD void temporal_store(const TemporalArgs &a, const cx<float> *buf, long long bout, int valid, int tid, int nthr, const double *thr, const TrcParams &tp)
{
	const int Q = a.K >> 2, total = a.S * Q;
	const float *bf = reinterpret_cast<const float *>(buf);
	const float mulf = (float)a.mul8;
	for (int it = tid; it < total; it += nthr) {
		const int y = (int)a.divQ.div((uint32_t)it), q = it - y * Q;
		if (4 * q >= valid) continue;
		const float4 F = *reinterpret_cast<const float4 *>(bf + (size_t)a.posi[makhoul_dst(y, a.S)] * a.K + 4 * q);
		const float sc = (y == 0) ? a.i_scale * a.i_out0 : a.i_scale;
		const float o[4] = {F.x * sc, -F.y * sc, F.z * sc, -F.w * sc};
		const long long off = bout + (long long)y * a.P + 4 * q;
		if constexpr (U8) {
			uint32_t w4 = 0;
#pragma unroll
			for (int e = 0; e < 4; e++) {
				if constexpr (TRC) { const double pel = (double)o[e] * a.mul8; w4 |= trc_u8_byte_from(thr, pel, trc_u8_seed(tp, pel)) << (8 * e); }
				else w4 |= quantise_u8_of(o[e], a.mul8, mulf) << (8 * e);
			}
			__builtin_memcpy(a.out8 + off, &w4, 4);
		} else {
			float4 r; r.x = o[0]; r.y = o[1]; r.z = o[2]; r.w = o[3];
			*reinterpret_cast<float4 *>(a.out + off) = r;
		}
	}
}
// thr: the threshold table of the transfer characteristic `trc` (8-bit output only), or NULL
DSP_HD void temporal_phase_store(const TemporalArgs &a, const cx<float> *buf, long long bout, int valid, int tid, int nthr, const double *thr, int trc)
{
	if (!a.out8) temporal_store<false, false>(a, buf, bout, valid, tid, nthr, thr, TrcParams());
	else if (thr) temporal_store<true, true>(a, buf, bout, valid, tid, nthr, thr, trc_params(trc));
	else temporal_store<true, false>(a, buf, bout, valid, tid, nthr, thr, TrcParams());
}

}  // namespace dspfft
