// block_rs_packed_core.h -- motion -b with -s over a block grid (block_rs_core.h) on PACKED 8-bit pixels (block_packed_core.h): rgb24, rgba and
// their like, C = 2, 3 or 4 bytes per pixel, every component of every pixel block a block of its own (motion -c pixel_format=rgb24 --blocksize
// 8x8x8 --size 4x4x4; motion/motion.c:155-156,488-499,535-552,613-776).  The phases of block_rescale_packed.hip's kernel: what is new are the
// two ENDS of a line and a mid phase that knows a line's component; the pruned y lines are block_rs_core.h's as they stand, over cnt * C tile
// blocks, and the line functions (rs_line_mid, tiny_dct, packed_line_pick / _put) are the two parents'.
//   tile      [MZ][MY][C * cnt * AX] floats, M = max(block, scaled) and A = min(block, scaled) per axis: a workgroup takes cnt <= G pixel
//             blocks.  Component-major in the row, as block_packed_core.h's tile and for its reason: tile block c * cnt + g is component c
//             of pixel block g.  pitch = C G tw with tw = AX, where the planar grid's tile has tw = MX: no phase keeps more than AX values
//             of an x line in the tile (the load stores the first AX results, the store reads AX values and puts zeros behind them), so
//             the planar tile's other columns are never touched -- and with C components they cost the pixel blocks per workgroup that
//             the ends need (see rs_packed_group_of for the measurement)
//   load      thread = one x line of one PIXEL block: NX * C contiguous bytes as NX * C / 4 whole dwords; per component the bytes picked out of
//             them (through the decode table when one is set), REDFT10 in registers, the first min(NX, ox) results into the component's slot
//   y, mid    rs_phase_fwd_y / rs_phase_inv_y over cnt * C blocks; the mid phase with the filter of the line's component: damp, boost and
//             grey_add by byte position, quant_only with them (packed_filter_of), every other field shared
//   store     thread = one x line of one pixel block of the OUTPUT: per component min(nx, SX) values out of the tile, zeros behind them,
//             REDFT01 over SX, the quantised (or encoded) bytes OR-ed into SX * C / 4 dwords; the dwords are stored once
// RsTile's strides and the block offsets are in BYTES here (the planar plans' pixel strides times C), G counts pixel blocks, in / out are NULL.
// Plain C++17 for device (hipcc) and host (g++: tests/test_motion_packed_rescale_cpu.py runs the phases thread by thread).
#pragma once
#include "block_rs_core.h"
#include "block_packed_core.h"

namespace dspfft {

struct BlockRsPackedArgs : BlockRsArgs {       // in / out are NULL; filt.damp / boost / grey_add are not read
	int comps;                                   // C
	float damp[PACKED_MAX_COMPS], boost[PACKED_MAX_COMPS], grey_add[PACKED_MAX_COMPS];   // by byte position inside the pixel
};
// The phases read RsTile's scalars (rs_tile_of: block_rs_core.h's reason); the three arrays they read from the kernel's arguments themselves,
// through packed_pick.  (Copied into a local structure beside the tile's scalars they kept the whole copy in scratch memory at C = 3 and 4.)

// Pixel blocks per workgroup, from a component block's tile (mx = AX columns, my = MY rows, mz = MZ planes) and the lines of the two ends (ny nz
// lines of a pixel block at the load, oy oz at the store).  The grid's rule times C -- tiles of about 8192 samples, rows of at most 1 KB --
// leaves the ends short of lines, as packed_group_of found for equal extents: they run one thread per line of a PIXEL block, and a 1x8x8 ->
// 1x16x16 rgb24 tile of five pixel blocks has 40 lines to load for 256 threads.  So the row limit gives way: up to 8192 samples whatever the
// row's length, and pixel blocks until the leaner end has a line for every thread of the workgroup while the tile stays within 12288
// samples (48 KB: the tables and the counter still fit behind it).  Measured on 1920x1080x64 (tools/bench_motion_packed_rescale.py, the
// sweeps over DSPFFT_PACKED_G in profiles/r20_motion_packed_rescale.txt), rgb24: 8x8x8 -> 4x4x4 0.49 ms at five pixel blocks, 0.39 ms at
// eight, 0.36 ms at ten (8192 samples) and 0.30 ms at the rule's sixteen (0.44 ms at twenty, a tile of 60 KB); 4x4x4 -> 8x8x8
// 4.51, 3.58, 3.39 and 2.81 ms; 1x8x8 -> 1x16x16 4.78 ms at five (the row limit), 2.54 ms at ten, 2.13 ms at sixteen and 1.73 ms at the
// rule's thirty-two; rgba 8x8x8 -> 4x4x4 0.61 ms at eight and 0.55 ms at the rule's twelve.  The tile's AX columns are what lets the rule
// reach these counts: with the planar tile's MX columns eight rgb24 pixel blocks of 8x8x8 -> 4x4x4 are the 12288 samples (0.39 ms) and rgba
// stops at seven in 64 KB (0.70 ms).  At least one pixel block.
DSP_HD int rs_packed_group_of(int mx, int my, int mz, int lines_in, int lines_out, int comps, int nxb)
{
	const int e = mx * my * mz * comps, lines = lines_in < lines_out ? lines_in : lines_out;
	int G = 8192 / e;
	int want = (BLOCK_THREADS + lines - 1) / lines;
	if (want > 12288 / e) want = 12288 / e;
	if (G < want) G = want;
	if (G > nxb) G = nxb;
	return G < 1 ? 1 : G;
}

// ---- the two ends ----
// the packed line of a pixel block; per component conversion + REDFT10 along x; the first min(NX, ox) results go into the component's slot
// (rs_load_x's rule and its pruned float4 stores)
template <int NX, int C, bool TRC>
DSP_HD void rs_packed_load_x(const RsTile &a, const TinyArgs &tx, float *lds, long long bin, int cnt, int tid, const float *lut)
{
	constexpr int W = NX * C / 4;
	const int ly = rs_log2(a.ny), lrows = ly + rs_log2(a.nz), my = rs_max(a.ny, a.oy), kx = rs_min(NX, a.ox);
	const int lines = cnt << lrows;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		rs_line_of(a.rows_fast, l, lrows, cnt, row, g);
		const int z = row >> ly, y = row & (a.ny - 1);
		const long long off = bin + (long long)g * a.sxb_in + (long long)z * a.sz_in + (long long)y * a.sy_in;
		uint32_t w[W];
#pragma unroll
		for (int j = 0; j < W; j++) __builtin_memcpy(&w[j], a.in8 + off + 4 * j, 4);
		float *const base = lds + (z * my + y) * a.pitch + g * a.tw;
#pragma unroll
		for (int c = 0; c < C; c++) {
			float x[NX], o[NX];
			packed_line_pick<NX, C, TRC>(w, c, lut, x);
			tiny_dct<NX, KIND_REDFT10>(tx, x, o);
			float4 *q = reinterpret_cast<float4 *>(base + c * cnt * a.tw);
#pragma unroll
			for (int j = 0; j < NX / 4; j++)
				if (4 * j < kx) { float4 v; v.x = o[4 * j]; v.y = o[4 * j + 1]; v.z = o[4 * j + 2]; v.w = o[4 * j + 3]; q[j] = v; }
		}
	}
}
// per component min(nx, SX) values out of the tile, zeros behind them, REDFT01 along x and the bytes into the packed line, stored once
template <int SX, int C, bool TRC>
DSP_HD void rs_packed_store_x(const RsTile &a, const TinyArgs &tx, const float *lds, long long bout, int cnt, int tid, const double *thr, const TrcParams &tp)
{
	constexpr int W = SX * C / 4;
	const int ly = rs_log2(a.oy), lrows = ly + rs_log2(a.oz), my = rs_max(a.ny, a.oy), kx = rs_min(a.nx, SX);
	const int lines = cnt << lrows;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		rs_line_of(a.rows_fast, l, lrows, cnt, row, g);
		const int z = row >> ly, y = row & (a.oy - 1);
		const long long off = bout + (long long)g * a.sxb_out + (long long)z * a.sz_out + (long long)y * a.sy_out;
		uint32_t w[W];
#pragma unroll
		for (int j = 0; j < W; j++) w[j] = 0;
		const float *const base = lds + (z * my + y) * a.pitch + g * a.tw;
#pragma unroll
		for (int c = 0; c < C; c++) {
			float x[SX], o[SX];
			const float4 *q = reinterpret_cast<const float4 *>(base + c * cnt * a.tw);
#pragma unroll
			for (int j = 0; j < SX / 4; j++) {
				float4 v; v.x = v.y = v.z = v.w = 0.f;
				if (4 * j < kx) v = q[j];
				x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
			}
			tiny_dct<SX, KIND_REDFT01>(tx, x, o);
			packed_line_put<SX, C, TRC>(o, c, a.mul8, thr, tp, w);
		}
#pragma unroll
		for (int j = 0; j < W; j++) __builtin_memcpy(a.out8 + off + 4 * j, &w[j], 4);
	}
}

// ---- the phases, in the kernel's order; rs_phase_fwd_y and rs_phase_inv_y run between them over cnt * C blocks ----
// lut: the decode table of motion --linear, or NULL
template <int C>
DSP_HD void rs_packed_phase_load(const RsTile &a, float *lds, long long bin, int cnt, int tid, const float *lut)
{
	const TinyArgs tx = block_axis_args(a.f, 0, false);
	switch (a.nx) {
#define DSP_RS_CASE(N_) \
	case N_: \
		if (lut) rs_packed_load_x<N_, C, true>(a, tx, lds, bin, cnt, tid, lut); \
		else rs_packed_load_x<N_, C, false>(a, tx, lds, bin, cnt, tid, lut); \
		break;
	DSP_RS_CASE(4) DSP_RS_CASE(8) DSP_RS_CASE(16) DSP_RS_CASE(32)
#undef DSP_RS_CASE
	}
}
// rs_phase_mid over the cnt * C blocks of the tile, each line with the filter of its block's component
template <int C>
DSP_HD void rs_packed_phase_mid(const RsTile &a, const BlockRsPackedArgs &pc, float *lds, int cnt, int tid, unsigned long long &coded)
{
	const int kx = rs_min(a.nx, a.ox), lkx = rs_log2(kx), my = rs_max(a.ny, a.oy), nb = cnt * C;
	// column l -> its offset in the tile, the outer index o, x inside the block and the block's filter (rs_col with the component)
#define DSP_RS_COL(OSTRIDE_) \
	const int bx = l & (kx - 1), t = l >> lkx, o = t / nb, gb = t - o * nb; \
	float *p = lds + o * (OSTRIDE_) + gb * a.tw + bx; \
	const MotionFilter f = packed_filter_of<C>(pc, packed_comp_of<C>(gb, cnt), a.filt);
	if (a.nz > 1) {
		const TinyArgs tf = block_axis_args(a.f, 2, true), ti = block_axis_args(a.i, 2, false);
		const int total = rs_min(a.ny, a.oy) * nb * kx;
		switch (a.nz * 64 + a.oz) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { DSP_RS_COL(a.pitch) rs_line_mid<N_, S_, true>(tf, ti, f, p, my * a.pitch, o, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS16(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	} else {
		const TinyArgs tf = block_axis_args(a.f, 1, true), ti = block_axis_args(a.i, 1, false);
		const int total = nb * kx;
		switch (a.ny * 64 + a.oy) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { DSP_RS_COL(0) rs_line_mid<N_, S_, false>(tf, ti, f, p, a.pitch, 0, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS32(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	}
#undef DSP_RS_COL
}
// thr: the threshold table of the transfer characteristic behind tp, or NULL
template <int C>
DSP_HD void rs_packed_phase_store(const RsTile &a, const float *lds, long long bout, int cnt, int tid, const double *thr, const TrcParams &tp)
{
	// the inverse's global scale rides on its x pass, the last one here
	const TinyArgs tx = block_axis_args(a.i, 0, true);
	switch (a.ox) {
#define DSP_RS_CASE(N_) \
	case N_: \
		if (thr) rs_packed_store_x<N_, C, true>(a, tx, lds, bout, cnt, tid, thr, tp); \
		else rs_packed_store_x<N_, C, false>(a, tx, lds, bout, cnt, tid, thr, tp); \
		break;
	DSP_RS_CASE(4) DSP_RS_CASE(8) DSP_RS_CASE(16) DSP_RS_CASE(32)
#undef DSP_RS_CASE
	}
}

}  // namespace dspfft
