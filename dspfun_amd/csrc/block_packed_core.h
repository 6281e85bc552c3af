// block_packed_core.h -- the fused small-block roundtrip (block_core.h, block_rt.h) on PACKED 8-bit pixels: rgb24, rgba and their like, C = 2, 3
// or 4 bytes per pixel, every byte a component (motion -c pixel_format=rgb24, motion/motion.c:155-156; the reference reads component `comp` of a
// pixel at its byte offset with the pixel's step, include/ffapi.h:61-66, and every component of every pixel block is a block of its own,
// motion.c:613-615).  What is new here are the two ENDS of a line and the filter's knowledge of a block's component; the y / z lines, the top-N
// selection, the tables of motion --linear and the coded count are block_core.h's, topn_core.h's and block_rt.h's as they stand.
//   tile      [NZ][NY][C * cnt * NX] floats: a workgroup takes cnt <= G pixel blocks, each C component blocks.  Component-major in the row: tile
//             block c * cnt + g is component c of pixel block g, so in the x phases neighbouring lanes (neighbouring pixel blocks) are NX floats
//             apart in LDS exactly as in the planar kernel (pixel-major they would be C * NX apart: 32 floats for 8-point rgba lines, every lane of a
//             wave on the same banks), and the y / z phases still give neighbouring threads neighbouring columns
//   load      thread = one x line of one PIXEL block: NX * C contiguous bytes = NX * C / 4 whole dwords (NX is a multiple of 4 and every stride a
//             multiple of 4 pixels).  The raw dwords stay in registers (at most 32); per component its NX bytes are picked out of them -- after
//             unrolling, dword (C p + c) >> 2 and shift 8 ((C p + c) & 3) are constants --, converted (through the decode table when one is set),
//             transformed (tiny_dct) and written to that component's slot of the tile
//   store     the mirror image: per component the line out of the tile, tiny_dct, quantise (or the threshold table), OR into the packed dwords;
//             the dwords are stored once
//   filter    component c has its own damp, boost and grey_add (motion -D / -B r:g:b:a, motion.c:235-236,736); the other fields are shared (packed
//             formats have no subsampling).  A line's filter is made once, ahead of its unrolled body.
// BlockGeom's strides and offsets are in BYTES here (the planar plan's pixel strides times C), G counts PIXEL blocks and pitch = G C NX.
// Plain C++17 for device (hipcc) and the CPU emulation of the phases (g++, tests/test_motion_packed_cpu.py).
#pragma once
#include "block_core.h"
#include "dither_core.h"
#include "topn_core.h"

namespace dspfft {

enum { PACKED_MAX_COMPS = 4 };

struct BlockPackedArgs : BlockRtTopnArgs {       // in / out are NULL; keep = 0: no coefficient limit; filt.damp / boost / grey_add are not read
	int comps;                                   // C
	float damp[PACKED_MAX_COMPS], boost[PACKED_MAX_COMPS], grey_add[PACKED_MAX_COMPS];   // by byte position inside the pixel
	const TrcU8Tab *tab_in, *tab_out;            // the 8-bit ends' tables (a plan's device tables; NULL: that end converts plainly)
	int trc_out;                                 // the id behind tab_out (its parameters seed the threshold search)
};

// Pixel blocks per workgroup.  build_block's rule with the C-fold tile (4096 samples, rows of at most 1 KB) left the ends short of lines: they
// run one thread per line of a PIXEL block, and two 8x8x8 rgb24 blocks are 128 lines for 256 threads.  Measured on 1920x1080x64
// (tools/bench_motion_packed.py --block ... --g ..., profiles/r16_motion_packed.txt): tiles of about 6144 samples (24 KB, six workgroups per
// CU) are the fastest for 8x8x8, 1x8x8, 4x4x4, 1x4x4 and 8x16x4 blocks at three and four components, long rows cost nothing, and where the lines
// exceed the workgroup's threads whole rounds of them beat a ragged last round.  Large 2-D blocks have few lines each (1x32x32 rgba at one
// pixel block: 32 lines, 3.66 ms against 2.07 ms at two): they take pixel blocks up to 128 lines while the tile stays within 32 KB.  At
// least one pixel block.
DSP_HD int packed_group_of(int nx, int ny, int nz, int comps, int nxb)
{
	const int e = nx * ny * nz * comps, lines = ny * nz;
	int G = 6144 / e;
	int want = (128 + lines - 1) / lines;
	if (want > 8192 / e) want = 8192 / e;
	if (G < want) G = want;
	const int per = BLOCK_THREADS / lines;              // pixel blocks whose lines fill the workgroup's threads once
	if (per > 0 && G > per) G -= G % per;
	if (G > nxb) G = nxb;
	return G < 1 ? 1 : G;
}

// the component of tile block gb (component-major: gb = c * cnt + g), without a division
template <int C>
DSP_HD int packed_comp_of(int gb, int cnt)
{
	int c = 0;
#pragma unroll
	for (int k = 1; k < C; k++) c += gb >= k * cnt;
	return c;
}
template <int C>
DSP_HD float packed_pick(const float (&v)[PACKED_MAX_COMPS], int c)
{
	float r = v[0];
#pragma unroll
	for (int k = 1; k < C; k++) r = c == k ? v[k] : r;
	return r;
}
// the call's filter as component c sees it; quant_only depends on damp and boost (motion_filter_set_divs) and goes with them.  Args: whatever
// holds the three per-byte arrays; shared: every other field (block_rs_packed_core.h keeps them in its tile's scalars)
template <int C, class Args>
DSP_HD MotionFilter packed_filter_of(const Args &a, int c, const MotionFilter &shared)
{
	MotionFilter f = shared;
	f.damp = packed_pick<C>(a.damp, c); f.boost = packed_pick<C>(a.boost, c); f.grey_add = packed_pick<C>(a.grey_add, c);
	f.quant_only = f.quantizer > 0.f && f.damp == 1.f && f.boost == 1.f && !(f.thr_hi > 0.f) && (f.preserve_dc == 0 || !(f.b0d || f.b0h || f.b0w));
	return f;
}
template <int C>
DSP_HD MotionFilter packed_filter_of(const BlockPackedArgs &a, int c) { return packed_filter_of<C>(a, c, a.filt); }

// component c of the NX pixels held in w: the bytes as floats, or (TRC) through the decode table
template <int NX, int C, bool TRC>
DSP_HD void packed_line_pick(const uint32_t (&w)[NX * C / 4], int c, const float *lut, float (&x)[NX])
{
#pragma unroll
	for (int p = 0; p < NX; p++) {
		const int i = C * p + c;
		const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
		if constexpr (TRC) x[p] = lut[b];
		else x[p] = (float)b;
	}
}
// ... and back: the bytes of o (motion.c:760-776, or (TRC) the encoded byte found in the threshold table) into component c's places of w
template <int NX, int C, bool TRC>
DSP_HD void packed_line_put(const float (&o)[NX], int c, double mul8, const double *thr, const TrcParams &tp, uint32_t (&w)[NX * C / 4])
{
#pragma unroll
	for (int p = 0; p < NX; p++) {
		const int i = C * p + c;
		uint32_t b;
		if constexpr (TRC) { const double pel = (double)o[p] * mul8; b = trc_u8_byte_from(thr, pel, trc_u8_seed(tp, pel)); }
		else b = quantise_u8_of(o[p], mul8, (float)mul8);
		w[i >> 2] |= b << (8 * (i & 3));
	}
}

// phase x, forward side: the packed line of a pixel block, per component conversion + x transform into the tile
template <int NX, int NY, int NZ, int C>
DSP_HD void packed_load_x(const BlockGeom &a, const TinyArgs &tx, const uint8_t *in8, float *lds, long long bin, int cnt, int tid, const float *lut)
{
	constexpr int W = NX * C / 4;
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
		const int z = row / NY, y = row - z * NY;
		const long long off = bin + (long long)g * a.sxb_in + (long long)z * a.sz_in + (long long)y * a.sy_in;
		uint32_t w[W];
#pragma unroll
		for (int j = 0; j < W; j++) __builtin_memcpy(&w[j], in8 + off + 4 * j, 4);
#pragma unroll
		for (int c = 0; c < C; c++) {
			float x[NX], o[NX];
			if (lut) packed_line_pick<NX, C, true>(w, c, lut, x);
			else packed_line_pick<NX, C, false>(w, c, nullptr, x);
			tiny_dct<NX, KIND_REDFT10>(tx, x, o);
			float4 *q = reinterpret_cast<float4 *>(lds + row * a.pitch + (c * cnt + g) * NX);
#pragma unroll
			for (int j = 0; j < NX / 4; j++) { float4 v; v.x = o[4 * j]; v.y = o[4 * j + 1]; v.z = o[4 * j + 2]; v.w = o[4 * j + 3]; q[j] = v; }
		}
	}
}
// phase x, inverse side: per component x transform out of the tile + quantisation into the packed line, stored once
template <int NX, int NY, int NZ, int C>
DSP_HD void packed_store_x(const BlockGeom &a, const TinyArgs &tx, uint8_t *out8, double mul8, const float *lds, long long bout, int cnt, int tid, const double *thr,
                           const TrcParams &tp)
{
	constexpr int W = NX * C / 4;
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
		const int z = row / NY, y = row - z * NY;
		const long long off = bout + (long long)g * a.sxb_out + (long long)z * a.sz_out + (long long)y * a.sy_out;
		uint32_t w[W];
#pragma unroll
		for (int j = 0; j < W; j++) w[j] = 0;
#pragma unroll
		for (int c = 0; c < C; c++) {
			float x[NX], o[NX];
			const float4 *q = reinterpret_cast<const float4 *>(lds + row * a.pitch + (c * cnt + g) * NX);
#pragma unroll
			for (int j = 0; j < NX / 4; j++) { const float4 v = q[j]; x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w; }
			tiny_dct<NX, KIND_REDFT01>(tx, x, o);
			if (thr) packed_line_put<NX, C, true>(o, c, mul8, thr, tp, w);
			else packed_line_put<NX, C, false>(o, c, mul8, nullptr, tp, w);
		}
#pragma unroll
		for (int j = 0; j < W; j++) __builtin_memcpy(out8 + off + 4 * j, &w[j], 4);
	}
}
// block_lines_mid (the last forward axis, the filter and the same axis of the inverse on one line in registers) over the cnt * C blocks of
// the tile, with the filter of the line's component
template <int NX, int NY, int NZ, int C, bool ZAXIS>
DSP_HD void packed_lines_mid(const BlockPackedArgs &a, const TinyArgs &tf, const TinyArgs &ti, float *lds, int cnt, int tid, unsigned long long &coded)
{
	constexpr int N = ZAXIS ? NZ : NY, OUTER = ZAXIS ? NY : NZ;
	const int cols = cnt * C * NX;
	const int stride = ZAXIS ? NY * a.pitch : a.pitch;
	for (int l = tid; l < OUTER * cols; l += BLOCK_THREADS) {
		const int o = l / cols, c = l - o * cols;
		float *p = lds + (ZAXIS ? o * a.pitch : o * NY * a.pitch) + c;
		float x[N], y[N];
#pragma unroll
		for (int j = 0; j < N; j++) x[j] = p[j * stride];
		tiny_dct<N, KIND_REDFT10>(tf, x, y);
		if (a.filt.enabled) {
			const MotionFilter f = packed_filter_of<C>(a, packed_comp_of<C>(c / NX, cnt));
			const int bx = c % NX;
#pragma unroll
			for (int j = 0; j < N; j++) {
				const int bz = ZAXIS ? j : o, by = ZAXIS ? o : j;
				if (bx < f.aw && by < f.ah && bz < f.ad) y[j] = motion_filter_at(f, bz, by, bx, y[j], coded);
			}
		}
		tiny_dct<N, KIND_REDFT01>(ti, y, x);
#pragma unroll
		for (int j = 0; j < N; j++) p[j * stride] = x[j];
	}
}
// the filter alone over the tile (the top-N sequence, whose selection needs a block's coefficients before any of them is filtered)
template <int NX, int NY, int NZ, int C>
DSP_HD void packed_filter_sweep(const BlockPackedArgs &a, float *lds, int cnt, int tid, unsigned long long &coded)
{
	const int cols = cnt * C * NX;
	for (int l = tid; l < NZ * NY * cols; l += BLOCK_THREADS) {
		const int row = l / cols, c = l - row * cols;
		const int bz = row / NY, by = row - bz * NY, bx = c % NX;
		if (bx < a.filt.aw && by < a.filt.ah && bz < a.filt.ad) {
			const MotionFilter f = packed_filter_of<C>(a, packed_comp_of<C>(c / NX, cnt));
			float *p = lds + row * a.pitch + c;
			*p = motion_filter_at(f, bz, by, bx, *p, coded);
		}
	}
}

// ---- motion -d on packed small blocks (dspfft_execute_roundtrip_u8_packed_dither, block_packed_dither.hip): the store of the sequences above in
// three phases, a barrier after each of the first two.  When the y phase of the inverse ends, every z plane of every tile block is an NY x NX plane
// of the Floyd-Steinberg store (motion.c:778-787 walks each plane of each component block on its own) and lies in LDS whole.
//   inverse x   thread = one x line of a pixel block, as in packed_store_x, but the transformed line goes back to its slot of the tile: the
//               floats the planar kernel would store to the dithered call's work buffer
//   dither      thread = one plane, raster order (dither_plane_tile); the byte takes the float's slot.  The previous row's errors lie in LDS
//               lane-major (no dynamically indexed registers); the planes are dealt to the four waves in equal shares, because a plane is a
//               dependent chain of NY NX steps in double and a wave takes as long over one lane as over 64
//   store       packed_store_x's addresses and dwords, the bytes taken from the tile
struct BlockPackedDitherArgs : BlockPackedArgs {   // out8: the dithered bytes; mul8 is not read
	double sf, norm;                               // motion's scalefactor and normalization (dither_core.h)
	int slots;                                     // dither lanes of a full tile (packed_dither_slots): each has NX doubles of LDS behind the error table
};
// lanes per wave that take a plane when the tile holds `nplanes`
DSP_HD int packed_dither_lanes(int nplanes)
{
	const int q = (nplanes + BLOCK_THREADS / 64 - 1) / (BLOCK_THREADS / 64);
	return q > 64 ? 64 : q;
}
DSP_HD int packed_dither_slots(int nz, int comps, int G) { return (BLOCK_THREADS / 64) * packed_dither_lanes(nz * comps * G); }
// LDS of the dither phase behind the tile and the transfer tables: the 256 doubles of dither_table, then the lanes' error rows
DSP_HD size_t packed_dither_bytes(int nx, int slots) { return (256 + (size_t)slots * nx) * sizeof(double); }

template <int NX, int NY, int NZ, int C>
DSP_HD void packed_inverse_x(const BlockGeom &a, const TinyArgs &tx, float *lds, int cnt, int tid)
{
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
#pragma unroll
		for (int c = 0; c < C; c++) {
			float x[NX], o[NX];
			float4 *q = reinterpret_cast<float4 *>(lds + row * a.pitch + (c * cnt + g) * NX);
#pragma unroll
			for (int j = 0; j < NX / 4; j++) { const float4 v = q[j]; x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w; }
			tiny_dct<NX, KIND_REDFT01>(tx, x, o);
#pragma unroll
			for (int j = 0; j < NX / 4; j++) { float4 v; v.x = o[4 * j]; v.y = o[4 * j + 1]; v.z = o[4 * j + 2]; v.w = o[4 * j + 3]; q[j] = v; }
		}
	}
}
// tab: dither_table(sf, norm); dprow: a.slots * NX doubles; thr NULL: the plain byte, else the threshold table of the inverse plan's characteristic
template <int NX, int NY, int NZ, int C>
DSP_HD void packed_dither_tile(const BlockPackedDitherArgs &a, float *lds, int cnt, int tid, const double *tab, double *dprow, const double *thr, const TrcParams &tp)
{
	const int nb = cnt * C, nplanes = NZ * nb, q = packed_dither_lanes(nplanes), wave = tid >> 6, lane = tid & 63;
	if (lane >= q) return;
	const int slot = wave * q + lane, nslots = (BLOCK_THREADS / 64) * q;
	for (int pl = slot; pl < nplanes; pl += nslots) {
		const int z = pl / nb, gb = pl - z * nb;
		float *plane = lds + z * NY * a.pitch + gb * NX;
		if (thr) dither_plane_tile<true>(plane, a.pitch, NY, NX, a.sf, a.norm, tab, dprow + slot, nslots, thr, &tp);
		else dither_plane_tile<false>(plane, a.pitch, NY, NX, a.sf, a.norm, tab, dprow + slot, nslots);
	}
}
template <int NX, int NY, int NZ, int C>
DSP_HD void packed_store_bytes(const BlockGeom &a, uint8_t *out8, const float *lds, long long bout, int cnt, int tid)
{
	constexpr int W = NX * C / 4;
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
		const int z = row / NY, y = row - z * NY;
		const long long off = bout + (long long)g * a.sxb_out + (long long)z * a.sz_out + (long long)y * a.sy_out;
		uint32_t w[W];
#pragma unroll
		for (int j = 0; j < W; j++) w[j] = 0;
#pragma unroll
		for (int c = 0; c < C; c++) {
			const float *q = lds + row * a.pitch + (c * cnt + g) * NX;
#pragma unroll
			for (int p = 0; p < NX; p++) {
				const int i = C * p + c;
				w[i >> 2] |= dither_tile_byte(q + p) << (8 * (i & 3));
			}
		}
#pragma unroll
		for (int j = 0; j < W; j++) __builtin_memcpy(out8 + off + 4 * j, &w[j], 4);
	}
}

}  // namespace dspfft
