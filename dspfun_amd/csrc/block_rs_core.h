// block_rs_core.h -- motion's per-block pipeline with `scaled != block` over a whole grid of blocks (motion --blocksize 8x8x8 --size 4x4x4
// and the like, motion/motion.c:488-499,535-552,613-776): the phases of block_rescale.hip's kernel.  A block is transformed over N =
// `block`, filtered over A = min(block, scaled) and transformed back over S = `scaled` per axis; its output volume has other extents than
// its input volume, so the call is out of place by nature.
//
// One workgroup of BLOCK_THREADS takes G blocks.  Its LDS tile is [MZ][MY][G * MX] floats with M = max(N, S) per axis: the reference's
// minbuf embedding (motion.c:617).  What the reference zeroes there is never stored here: a line lives in one thread's registers, the
// inputs that the embedding would hold as zeros are literal zeros of the inverse line (the compiler drops their products), and the outputs
// that nothing reads are never computed or written:
//   load    thread = one x line of a block: NX samples from the INPUT layout, REDFT10 in registers, the first AX results into the tile
//   y       (3-D blocks) REDFT10 over NY for the columns x < AX, the first AY results back
//   mid     the last forward axis (z; y for 2-D blocks) for the columns x < AX, y < AY; the filter over the first AZ results at the block's
//           own coordinates; zero-padded or truncated to SZ; REDFT01 -- one line in registers, as block_core.h's block_lines_mid
//   y       (3-D blocks) REDFT01: AY values in, SY out, for the planes z < SZ
//   store   thread = one x line: AX values from the tile, REDFT01 over SX, SX samples into the OUTPUT layout
// Every extent is 4, 8, 16 or 32 (a power of two: the index arithmetic shifts).  The tile geometry is run-time; only the line functions
// are templates, on <N, S>, and the two ends on <N, 8-bit, table>, each chosen by a switch that is uniform over the workgroup.
// Plain C++17 for device (hipcc) and host (g++: tests/test_motion_block_rescale_cpu.py runs the phases thread by thread).
// At the end of the file: the further phases of the same grid with motion --coeff-limit (block_rescale_topn.hip).
#pragma once
#include "block_core.h"

namespace dspfft {

// BlockGeom's nx, ny, nz are the FORWARD extents; its *_in strides are the forward plan's input layout, its *_out strides the inverse
// plan's output layout; G, ngroups and pitch are derived for the pair
struct BlockRsArgs : BlockRtArgs {
	int ox, oy, oz;               // the inverse extents (`scaled`)
	int tw;                       // floats of one block in a tile row: max(nx, ox); pitch = G * tw
	const TrcU8Tab *tab_in, *tab_out;     // motion --linear at the 8-bit ends (a plan's device tables; NULL: that end converts plainly)
	int trc_out;                  // the id behind tab_out
};
// What the phases read of the arguments: scalars only, so that a kernel holds them in registers (BlockGeom's batch arrays are indexed at
// run time by block_base alone; a kernel that reads its arguments at hundreds of places through them keeps a copy in scratch memory)
struct RsTile {
	int nx, ny, nz, ox, oy, oz, tw, pitch, rows_fast;
	long long sy_in, sz_in, sxb_in, sy_out, sz_out, sxb_out;
	const float *in;
	float *out;
	const uint8_t *in8;
	uint8_t *out8;
	double mul8;
	BlockScales f, i;
	MotionFilter filt;
};
DSP_HD RsTile rs_tile_of(const BlockRsArgs &a)
{
	RsTile t;
	t.nx = a.nx; t.ny = a.ny; t.nz = a.nz; t.ox = a.ox; t.oy = a.oy; t.oz = a.oz; t.tw = a.tw; t.pitch = a.pitch; t.rows_fast = a.rows_fast;
	t.sy_in = a.sy_in; t.sz_in = a.sz_in; t.sxb_in = a.sxb_in; t.sy_out = a.sy_out; t.sz_out = a.sz_out; t.sxb_out = a.sxb_out;
	t.in = a.in; t.out = a.out; t.in8 = a.in8; t.out8 = a.out8; t.mul8 = a.mul8;
	t.f = a.f; t.i = a.i; t.filt = a.filt;
	return t;
}

DSP_HD int rs_min(int a, int b) { return a < b ? a : b; }
DSP_HD int rs_max(int a, int b) { return a > b ? a : b; }
DSP_HD int rs_log2(int v) { return __builtin_ctz((unsigned)v); }
// bytes of the tile
DSP_HD size_t rs_tile_bytes(const RsTile &a) { return (size_t)rs_max(a.nz, a.oz) * rs_max(a.ny, a.oy) * a.pitch * sizeof(float); }

// x line l of the workgroup -> (row of the block's own 2^lrows rows, block); block_line_of with the shift
DSP_HD void rs_line_of(int rows_fast, int l, int lrows, int cnt, int &row, int &g)
{
	if (rows_fast) { g = l >> lrows; row = l & ((1 << lrows) - 1); } else { row = l / cnt; g = l - row * cnt; }
}

// ---- the two ends ----
// load (float, 8-bit, 8-bit through the decode table) + REDFT10 along x; the first min(NX, ox) results go into the tile
template <int NX, bool U8, bool TRC>
DSP_HD void rs_load_x(const RsTile &a, const TinyArgs &tx, float *lds, long long bin, int cnt, int tid, const float *lut)
{
	const int ly = rs_log2(a.ny), lrows = ly + rs_log2(a.nz), my = rs_max(a.ny, a.oy), kx = rs_min(NX, a.ox);
	const int lines = cnt << lrows;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		rs_line_of(a.rows_fast, l, lrows, cnt, row, g);
		const int z = row >> ly, y = row & (a.ny - 1);
		const long long off = bin + (long long)g * a.sxb_in + (long long)z * a.sz_in + (long long)y * a.sy_in;
		float x[NX], o[NX];
		block_line_read<NX, U8, TRC>(a.in, a.in8, off, lut, x);
		tiny_dct<NX, KIND_REDFT10>(tx, x, o);
		float4 *q = reinterpret_cast<float4 *>(lds + (z * my + y) * a.pitch + g * a.tw);
#pragma unroll
		for (int j = 0; j < NX / 4; j++)
			if (4 * j < kx) { float4 v; v.x = o[4 * j]; v.y = o[4 * j + 1]; v.z = o[4 * j + 2]; v.w = o[4 * j + 3]; q[j] = v; }
	}
}
// min(nx, SX) values out of the tile, zeros behind them, REDFT01 along x + store (float, the quantised byte, the encoded byte)
template <int SX, bool U8, bool TRC>
DSP_HD void rs_store_x(const RsTile &a, const TinyArgs &tx, const float *lds, long long bout, int cnt, int tid, const double *thr, int trc)
{
	const int ly = rs_log2(a.oy), lrows = ly + rs_log2(a.oz), my = rs_max(a.ny, a.oy), kx = rs_min(a.nx, SX);
	const int lines = cnt << lrows;
	const TrcParams tp = trc_params(TRC ? trc : 0);        // (seeds the threshold search)
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		rs_line_of(a.rows_fast, l, lrows, cnt, row, g);
		const int z = row >> ly, y = row & (a.oy - 1);
		const long long off = bout + (long long)g * a.sxb_out + (long long)z * a.sz_out + (long long)y * a.sy_out;
		float x[SX], o[SX];
		const float4 *q = reinterpret_cast<const float4 *>(lds + (z * my + y) * a.pitch + g * a.tw);
#pragma unroll
		for (int j = 0; j < SX / 4; j++) {
			float4 v; v.x = v.y = v.z = v.w = 0.f;
			if (4 * j < kx) v = q[j];
			x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
		}
		tiny_dct<SX, KIND_REDFT01>(tx, x, o);
		block_line_write<SX, U8, TRC>(o, a.out, a.out8, off, a.mul8, thr, tp);
	}
}

// ---- lines along y / z: N samples `stride` floats apart in the tile ----
// REDFT10 over N; only the first min(N, S) results are stored (the others are dead code)
template <int N, int S>
DSP_HD void rs_line_fwd(const TinyArgs &t, float *p, int stride)
{
	constexpr int A = N < S ? N : S;
	float x[N], o[N];
#pragma unroll
	for (int j = 0; j < N; j++) x[j] = p[j * stride];
	tiny_dct<N, KIND_REDFT10>(t, x, o);
#pragma unroll
	for (int j = 0; j < A; j++) p[j * stride] = o[j];
}
// REDFT01 over S of min(N, S) values and zeros
template <int N, int S>
DSP_HD void rs_line_inv(const TinyArgs &t, float *p, int stride)
{
	constexpr int A = N < S ? N : S;
	float x[S], o[S];
#pragma unroll
	for (int j = 0; j < S; j++) x[j] = j < A ? p[j * stride] : 0.f;
	tiny_dct<S, KIND_REDFT01>(t, x, o);
#pragma unroll
	for (int j = 0; j < S; j++) p[j * stride] = o[j];
}
// the last forward axis, the filter (motion.c:683-744) and the same axis of the inverse.  ZAXIS: the line runs along z and `o` is its y,
// else it runs along y and `o` is its z.
template <int N, int S, bool ZAXIS>
DSP_HD void rs_line_mid(const TinyArgs &tf, const TinyArgs &ti, const MotionFilter &f, float *p, int stride, int o, int bx, unsigned long long &coded)
{
	constexpr int A = N < S ? N : S;
	float x[N], y[N];
#pragma unroll
	for (int j = 0; j < N; j++) x[j] = p[j * stride];
	tiny_dct<N, KIND_REDFT10>(tf, x, y);
	if (f.enabled) {
#pragma unroll
		for (int j = 0; j < A; j++) {
			const int bz = ZAXIS ? j : o, by = ZAXIS ? o : j;
			if (bx < f.aw && by < f.ah && bz < f.ad) y[j] = motion_filter_at(f, bz, by, bx, y[j], coded);
		}
	}
	float w[S], r[S];
#pragma unroll
	for (int j = 0; j < S; j++) w[j] = j < A ? y[j] : 0.f;
	tiny_dct<S, KIND_REDFT01>(ti, w, r);
#pragma unroll
	for (int j = 0; j < S; j++) p[j * stride] = r[j];
}

// the <N, S> pairs: 3-D blocks have extents up to 16, 2-D blocks up to 32
#define DSPFFT_RS_PAIRS16(X) X(4, 4) X(4, 8) X(4, 16) X(8, 4) X(8, 8) X(8, 16) X(16, 4) X(16, 8) X(16, 16)
#define DSPFFT_RS_PAIRS32(X) DSPFFT_RS_PAIRS16(X) X(4, 32) X(8, 32) X(16, 32) X(32, 4) X(32, 8) X(32, 16) X(32, 32)
DSP_HD bool rs_extent_ok(int n, bool two_d) { return n == 4 || n == 8 || n == 16 || (two_d && n == 32); }

// column l of a lines phase: x < 2^lkx of each of cnt blocks, times `o` rows or planes `ostride` floats apart -> its offset in the tile
DSP_HD int rs_col(const RsTile &a, int l, int lkx, int cnt, int ostride, int &o, int &bx)
{
	bx = l & ((1 << lkx) - 1);
	const int t = l >> lkx;
	o = t / cnt;
	return o * ostride + (t - o * cnt) * a.tw + bx;
}

// ---- the phases, in the kernel's order; between two of them the workgroup meets at a barrier ----
// lut: the decode table of motion --linear (8-bit input only), or NULL
DSP_HD void rs_phase_load(const RsTile &a, float *lds, long long bin, int cnt, int tid, const float *lut)
{
	// (the forward plan's global scale rides on its last axis: the mid phase)
	const TinyArgs tx = block_axis_args(a.f, 0, false);
	switch (a.nx) {
#define DSP_RS_CASE(N_) \
	case N_: \
		if (!a.in8) rs_load_x<N_, false, false>(a, tx, lds, bin, cnt, tid, lut); \
		else if (lut) rs_load_x<N_, true, true>(a, tx, lds, bin, cnt, tid, lut); \
		else rs_load_x<N_, true, false>(a, tx, lds, bin, cnt, tid, lut); \
		break;
	DSP_RS_CASE(4) DSP_RS_CASE(8) DSP_RS_CASE(16) DSP_RS_CASE(32)
#undef DSP_RS_CASE
	}
}
// 3-D blocks only: forward y for the planes z < nz
DSP_HD void rs_phase_fwd_y(const RsTile &a, float *lds, int cnt, int tid)
{
	if (a.nz == 1) return;
	const TinyArgs ty = block_axis_args(a.f, 1, false);
	const int kx = rs_min(a.nx, a.ox), lkx = rs_log2(kx), my = rs_max(a.ny, a.oy), total = a.nz * cnt * kx;
	switch (a.ny * 64 + a.oy) {
#define DSP_RS_CASE(N_, S_) \
	case N_ * 64 + S_: \
		for (int l = tid; l < total; l += BLOCK_THREADS) { int o, bx; float *p = lds + rs_col(a, l, lkx, cnt, my * a.pitch, o, bx); rs_line_fwd<N_, S_>(ty, p, a.pitch); } \
		break;
	DSPFFT_RS_PAIRS16(DSP_RS_CASE)
#undef DSP_RS_CASE
	}
}
DSP_HD void rs_phase_mid(const RsTile &a, float *lds, int cnt, int tid, unsigned long long &coded)
{
	const int kx = rs_min(a.nx, a.ox), lkx = rs_log2(kx), my = rs_max(a.ny, a.oy);
	if (a.nz > 1) {
		const TinyArgs tf = block_axis_args(a.f, 2, true), ti = block_axis_args(a.i, 2, false);
		const int total = rs_min(a.ny, a.oy) * cnt * kx;
		switch (a.nz * 64 + a.oz) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { int o, bx; float *p = lds + rs_col(a, l, lkx, cnt, a.pitch, o, bx); rs_line_mid<N_, S_, true>(tf, ti, a.filt, p, my * a.pitch, o, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS16(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	} else {
		const TinyArgs tf = block_axis_args(a.f, 1, true), ti = block_axis_args(a.i, 1, false);
		const int total = cnt * kx;
		switch (a.ny * 64 + a.oy) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { int o, bx; float *p = lds + rs_col(a, l, lkx, cnt, 0, o, bx); rs_line_mid<N_, S_, false>(tf, ti, a.filt, p, a.pitch, 0, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS32(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	}
}
// 3-D blocks only: inverse y for the planes z < oz
DSP_HD void rs_phase_inv_y(const RsTile &a, float *lds, int cnt, int tid)
{
	if (a.nz == 1) return;
	const TinyArgs ty = block_axis_args(a.i, 1, false);
	const int kx = rs_min(a.nx, a.ox), lkx = rs_log2(kx), my = rs_max(a.ny, a.oy), total = a.oz * cnt * kx;
	switch (a.ny * 64 + a.oy) {
#define DSP_RS_CASE(N_, S_) \
	case N_ * 64 + S_: \
		for (int l = tid; l < total; l += BLOCK_THREADS) { int o, bx; float *p = lds + rs_col(a, l, lkx, cnt, my * a.pitch, o, bx); rs_line_inv<N_, S_>(ty, p, a.pitch); } \
		break;
	DSPFFT_RS_PAIRS16(DSP_RS_CASE)
#undef DSP_RS_CASE
	}
}
// thr: the threshold table of the transfer characteristic `trc` (8-bit output only), or NULL
DSP_HD void rs_phase_store(const RsTile &a, const float *lds, long long bout, int cnt, int tid, const double *thr, int trc)
{
	// the inverse's global scale rides on its x pass, the last one here
	const TinyArgs tx = block_axis_args(a.i, 0, true);
	switch (a.ox) {
#define DSP_RS_CASE(N_) \
	case N_: \
		if (!a.out8) rs_store_x<N_, false, false>(a, tx, lds, bout, cnt, tid, thr, trc); \
		else if (thr) rs_store_x<N_, true, true>(a, tx, lds, bout, cnt, tid, thr, trc); \
		else rs_store_x<N_, true, false>(a, tx, lds, bout, cnt, tid, thr, trc); \
		break;
	DSP_RS_CASE(4) DSP_RS_CASE(8) DSP_RS_CASE(16) DSP_RS_CASE(32)
#undef DSP_RS_CASE
	}
}

// ---- motion --coeff-limit on a rescaled grid (block_rescale_topn.hip; motion.c:652-668 ranks the whole M embedding) ----
// The reference multiplies only the A corner by the uniform-range factors (:644-647) and then ranks every element of the embedding, so an
// element inside N but outside A competes with its RAW coefficient.  The forward passes here are the pruned kernel's, with the plan's scales
// in the butterflies, over ALL of N; the last of them rewrites what it stores outside A as the value the reference ranks: the scales divided
// out again, times `outside_mul`.  Nothing reads those elements after the selection, so they are keys only.  The selection itself is
// topn_core.h's on the tile; behind it the filter and the inverse passes read A alone, as the pruned kernel's do.
struct BlockRsTopnArgs : BlockRsArgs {
	unsigned int keep;            // 0 < keep < MX MY MZ
	float key_mul;                // outside_mul / f.scale ...
	float key_mul0[3];            // ... and per axis (x, y, z) 1 / f.out0[axis], for index 0 of that axis
};
// what the phases below read of them
struct RsKeys { float mul, mul0[3]; };
DSP_HD RsKeys rs_keys_of(const BlockRsTopnArgs &a)
{
	RsKeys k;
	k.mul = a.key_mul;
	for (int i = 0; i < 3; i++) k.mul0[i] = a.key_mul0[i];
	return k;
}
// The tile as the unpruned forward phases see it: with `scaled` = the embedding, rs_phase_load stores all NX results of a line and
// rs_phase_fwd_y runs over all columns x < NX and stores all NY results (min(N, M) = N).
DSP_HD RsTile rs_tile_unpruned(const RsTile &a)
{
	RsTile t = a;
	t.ox = rs_max(a.nx, a.ox); t.oy = rs_max(a.ny, a.oy); t.oz = rs_max(a.nz, a.oz);
	return t;
}
// zeros where the embedding lies outside N (upscaled axes): the selection reads every element of the embedding.  Runs beside the load,
// which writes inside N only.
DSP_HD void rs_phase_zero_outside(const RsTile &a, float *lds, int cnt, int tid)
{
	const int my = rs_max(a.ny, a.oy), mz = rs_max(a.nz, a.oz);
	if (a.tw == a.nx && my == a.ny && mz == a.nz) return;
	const int lqx = rs_log2(a.tw) - 2, lmy = rs_log2(my), total = (mz * my * cnt) << lqx;
	for (int l = tid; l < total; l += BLOCK_THREADS) {
		const int q = l & ((1 << lqx) - 1), t = l >> lqx, row = t / cnt, g = t - row * cnt;
		if (4 * q >= a.nx || (row & (my - 1)) >= a.ny || (row >> lmy) >= a.nz) {
			float4 v; v.x = v.y = v.z = v.w = 0.f;
			*reinterpret_cast<float4 *>(lds + row * a.pitch + g * a.tw + 4 * q) = v;
		}
	}
}
// REDFT10 over N, all N results stored; in_a: the column lies inside A on the other axes, and then the first min(N, S) results are the
// coefficients; every other result becomes its key value (mul; mul0 at index 0)
template <int N, int S>
DSP_HD void rs_line_fwd_keys(const TinyArgs &t, float *p, int stride, bool in_a, float mul, float mul0)
{
	constexpr int A = N < S ? N : S;
	float x[N], o[N];
#pragma unroll
	for (int j = 0; j < N; j++) x[j] = p[j * stride];
	tiny_dct<N, KIND_REDFT10>(t, x, o);
#pragma unroll
	for (int j = 0; j < N; j++) p[j * stride] = (in_a && j < A) ? o[j] : o[j] * (j == 0 ? mul0 : mul);
}
// the filter over the first min(N, S) values of a line and REDFT01 over S: rs_line_mid without its forward half
template <int N, int S, bool ZAXIS>
DSP_HD void rs_line_filt_inv(const TinyArgs &ti, const MotionFilter &f, float *p, int stride, int o, int bx, unsigned long long &coded)
{
	constexpr int A = N < S ? N : S;
	float w[S], r[S];
#pragma unroll
	for (int j = 0; j < S; j++) w[j] = j < A ? p[j * stride] : 0.f;
	if (f.enabled) {
#pragma unroll
		for (int j = 0; j < A; j++) {
			const int bz = ZAXIS ? j : o, by = ZAXIS ? o : j;
			if (bx < f.aw && by < f.ah && bz < f.ad) w[j] = motion_filter_at(f, bz, by, bx, w[j], coded);
		}
	}
	tiny_dct<S, KIND_REDFT01>(ti, w, r);
#pragma unroll
	for (int j = 0; j < S; j++) p[j * stride] = r[j];
}
// the last forward axis (z; y for 2-D blocks) over all columns x < NX (, y < NY), with the forward plan's global scale as in rs_phase_mid
DSP_HD void rs_phase_fwd_last_keys(const RsTile &a, const RsKeys &k, float *lds, int cnt, int tid)
{
	const int lnx = rs_log2(a.nx), ax = rs_min(a.nx, a.ox), my = rs_max(a.ny, a.oy);
	if (a.nz > 1) {
		const TinyArgs tf = block_axis_args(a.f, 2, true);
		const int total = a.ny * cnt * a.nx, ay = rs_min(a.ny, a.oy);
		switch (a.nz * 64 + a.oz) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { \
				int o, bx; float *p = lds + rs_col(a, l, lnx, cnt, a.pitch, o, bx); \
				const float m = k.mul * (bx ? 1.f : k.mul0[0]) * (o ? 1.f : k.mul0[1]); \
				rs_line_fwd_keys<N_, S_>(tf, p, my * a.pitch, bx < ax && o < ay, m, m * k.mul0[2]); } \
			break;
		DSPFFT_RS_PAIRS16(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	} else {
		const TinyArgs tf = block_axis_args(a.f, 1, true);
		const int total = cnt * a.nx;
		switch (a.ny * 64 + a.oy) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { \
				int o, bx; float *p = lds + rs_col(a, l, lnx, cnt, 0, o, bx); \
				const float m = k.mul * (bx ? 1.f : k.mul0[0]) * k.mul0[2]; \
				rs_line_fwd_keys<N_, S_>(tf, p, a.pitch, bx < ax, m, m * k.mul0[1]); } \
			break;
		DSPFFT_RS_PAIRS32(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	}
}
// behind the selection: the filter and the inverse's first axis over A, rs_phase_mid's columns
DSP_HD void rs_phase_filt_inv_last(const RsTile &a, float *lds, int cnt, int tid, unsigned long long &coded)
{
	const int kx = rs_min(a.nx, a.ox), lkx = rs_log2(kx), my = rs_max(a.ny, a.oy);
	if (a.nz > 1) {
		const TinyArgs ti = block_axis_args(a.i, 2, false);
		const int total = rs_min(a.ny, a.oy) * cnt * kx;
		switch (a.nz * 64 + a.oz) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { int o, bx; float *p = lds + rs_col(a, l, lkx, cnt, a.pitch, o, bx); rs_line_filt_inv<N_, S_, true>(ti, a.filt, p, my * a.pitch, o, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS16(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	} else {
		const TinyArgs ti = block_axis_args(a.i, 1, false);
		const int total = cnt * kx;
		switch (a.ny * 64 + a.oy) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { int o, bx; float *p = lds + rs_col(a, l, lkx, cnt, 0, o, bx); rs_line_filt_inv<N_, S_, false>(ti, a.filt, p, a.pitch, 0, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS32(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	}
}
// the selection's geometry: a block's embedding has E = MX MY MZ elements (16 ... 4096, a power of two), L = min(E, 64) lanes hold K = E / L
// keys each; the <K, MX> with a selection: X(K, MX)
#define DSPFFT_RS_TOPN_SHAPES(X) \
	X(1, 4) X(2, 4) X(4, 4) X(8, 4) X(16, 4) \
	X(1, 8) X(2, 8) X(4, 8) X(8, 8) X(16, 8) X(32, 8) \
	X(1, 16) X(2, 16) X(4, 16) X(8, 16) X(16, 16) X(32, 16) X(64, 16) \
	X(2, 32) X(4, 32) X(8, 32) X(16, 32)
DSP_HD int rs_topn_elems(const RsTile &a) { return a.tw * rs_max(a.ny, a.oy) * rs_max(a.nz, a.oz); }
DSP_HD int rs_topn_keys(int E) { return E >= 64 ? E / 64 : 1; }

}  // namespace dspfft
