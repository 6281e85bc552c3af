// block_rs_packed_wide_core.h -- motion -b with -s on packed 8-bit pixels (block_rs_packed_core.h) with --coeff-limit, with -d, or with both
// (dspfft_execute_roundtrip_u8_packed_rescale_limit / _dither; block_rescale_packed_limit.hip, block_rescale_packed_dither.hip).  The plain kernel's
// tile keeps A = min(block, scaled) columns per component block; both features need more of an x line in the tile:
//   --coeff-limit   the reference ranks the whole M = max(block, scaled) embedding (motion.c:652-668), so the tile is [MZ][MY][C * cnt * MX] and the
//                   forward passes run unpruned, exactly as in block_rescale_topn.hip: the packed load with the unpruned tile (all NX results
//                   of a line), zeros outside `block`, forward y, the last forward pass with the keys (block_rs_core.h, over cnt * C tile
//                   blocks), the selection per COMPONENT block (topn_core.h), then the filter and the inverse's first pass with the filter of
//                   the line's component, inverse y and the packed store
//   -d              the inverse's x pass writes its SX floats back to the tile, so a component block is SX columns wide (MX with a limit): the
//                   oz planes of oy x SX floats of every tile block are the planes of the Floyd-Steinberg store (motion.c:778-787), oy lanes
//                   walk one plane, row y two pixels behind row y - 1 (rs_packed_dither_wave; the host states the same walk one thread per plane,
//                   dither_core.h: dither_plane_tile), and the bytes leave through the packed store's dwords
//                   Tiles of many small planes keep one lane per plane (rs_packed_phase_dither): rs_packed_dither_by_rows chooses.
// LDS: the tile | TrcU8Tab | the workgroup's coded count (16 bytes) | with -d: the 256 doubles of dither_table, then, with one lane per plane, the
// dither lanes' error rows (block_packed_core.h: packed_dither_slots / packed_dither_bytes with SX and oz).
// Plain C++17 for device (hipcc) and host (g++: tests/test_motion_packed_rescale_limit_cpu.py and _dither_cpu.py run the phases thread by thread).
#pragma once
#include "block_rs_packed_core.h"
#include "block_rt.h"

namespace dspfft {

struct BlockRsPackedWideArgs : BlockRsPackedArgs {       // tw = the wide tile's columns per component block (rs_packed_wide_tw)
	unsigned int keep;            // 0: no coefficient limit; else 0 < keep < MX MY MZ
	float key_mul;                // BlockRsTopnArgs's: outside_mul / f.scale ...
	float key_mul0[3];            // ... and per axis (x, y, z) 1 / f.out0[axis]
	int dither;                   // motion -d: out8 takes the dithered bytes, mul8 is not read
	double sf, norm;              // motion's scalefactor and normalization (dither_core.h)
	int slots;                    // dither lanes of a full tile (packed_dither_slots of oz): each has SX doubles of LDS behind the error table
	int by_rows;                  // the dither walks a plane on oy lanes (rs_packed_dither_wave; no error rows in LDS) instead of one
};
DSP_HD RsKeys rs_keys_of(const BlockRsPackedWideArgs &a)
{
	RsKeys k;
	k.mul = a.key_mul;
	for (int i = 0; i < 3; i++) k.mul0[i] = a.key_mul0[i];
	return k;
}

// columns of a component block in the wide tile
DSP_HD int rs_packed_wide_tw(int nx, int ox, bool limit) { return limit ? rs_max(nx, ox) : ox; }
// the dither's LDS behind tile, tables and counter (0 without -d)
// Which walk: one lane per plane takes oy ox dependent steps per round of BLOCK_THREADS planes; oy lanes per plane take ox + 2 (oy - 1) steps per
// round of BLOCK_THREADS / oy planes, each step dearer by its shuffles.  Rows pay when they cut the steps by a quarter or more: tiles of few, large
// planes (1x8x8 -> 1x16x16: 30 planes of 256 pixels), not the many small planes of 3-D blocks.  nplanes: those of a full tile.
DSP_HD bool rs_packed_dither_by_rows(int oy, int ox, int nplanes)
{
	const int one = ((nplanes + BLOCK_THREADS - 1) / BLOCK_THREADS) * oy * ox, rows = ((nplanes * oy + BLOCK_THREADS - 1) / BLOCK_THREADS) * (ox + 2 * (oy - 1));
	return 4 * rows <= 3 * one;
}
DSP_HD size_t rs_packed_wide_dither_bytes(int ox, int oz, int comps, int G, bool dither, bool by_rows)
{
	if (!dither) return 0;
	return by_rows ? 256 * sizeof(double) : packed_dither_bytes(ox, packed_dither_slots(oz, comps, G));
}

// ---- --coeff-limit: behind the selection, rs_phase_filt_inv_last over the cnt * C blocks of the tile, each line with the filter of its component ----
template <int C>
DSP_HD void rs_packed_phase_filt_inv_last(const RsTile &a, const BlockRsPackedArgs &pc, float *lds, int cnt, int tid, unsigned long long &coded)
{
	const int kx = rs_min(a.nx, a.ox), lkx = rs_log2(kx), my = rs_max(a.ny, a.oy), nb = cnt * C;
#define DSP_RS_COL(OSTRIDE_) \
	const int bx = l & (kx - 1), t = l >> lkx, o = t / nb, gb = t - o * nb; \
	float *p = lds + o * (OSTRIDE_) + gb * a.tw + bx; \
	const MotionFilter f = packed_filter_of<C>(pc, packed_comp_of<C>(gb, cnt), a.filt);
	if (a.nz > 1) {
		const TinyArgs ti = block_axis_args(a.i, 2, false);
		const int total = rs_min(a.ny, a.oy) * nb * kx;
		switch (a.nz * 64 + a.oz) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { DSP_RS_COL(a.pitch) rs_line_filt_inv<N_, S_, true>(ti, f, p, my * a.pitch, o, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS16(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	} else {
		const TinyArgs ti = block_axis_args(a.i, 1, false);
		const int total = nb * kx;
		switch (a.ny * 64 + a.oy) {
#define DSP_RS_CASE(N_, S_) \
		case N_ * 64 + S_: \
			for (int l = tid; l < total; l += BLOCK_THREADS) { DSP_RS_COL(0) rs_line_filt_inv<N_, S_, false>(ti, f, p, a.pitch, 0, bx, coded); } \
			break;
		DSPFFT_RS_PAIRS32(DSP_RS_CASE)
#undef DSP_RS_CASE
		}
	}
#undef DSP_RS_COL
}

// ---- -d: the store in three phases, a barrier after each of the first two (block_packed_core.h's, with the grid's run-time geometry) ----
// inverse x: rs_packed_store_x's lines and values, but the transformed line goes back to its slot of the tile (SX <= tw floats): the floats the
// planar call stores to the dithered call's work buffer
template <int SX, int C>
DSP_HD void rs_packed_inverse_x(const RsTile &a, const TinyArgs &tx, float *lds, int cnt, int tid)
{
	const int ly = rs_log2(a.oy), lrows = ly + rs_log2(a.oz), my = rs_max(a.ny, a.oy), kx = rs_min(a.nx, SX);
	const int lines = cnt << lrows;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		rs_line_of(a.rows_fast, l, lrows, cnt, row, g);
		const int z = row >> ly, y = row & (a.oy - 1);
		float *const base = lds + (z * my + y) * a.pitch + g * a.tw;
#pragma unroll
		for (int c = 0; c < C; c++) {
			float x[SX], o[SX];
			float4 *q = reinterpret_cast<float4 *>(base + c * cnt * a.tw);
#pragma unroll
			for (int j = 0; j < SX / 4; j++) {
				float4 v; v.x = v.y = v.z = v.w = 0.f;
				if (4 * j < kx) v = q[j];
				x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
			}
			tiny_dct<SX, KIND_REDFT01>(tx, x, o);
#pragma unroll
			for (int j = 0; j < SX / 4; j++) { float4 v; v.x = o[4 * j]; v.y = o[4 * j + 1]; v.z = o[4 * j + 2]; v.w = o[4 * j + 3]; q[j] = v; }
		}
	}
}
template <int C>
DSP_HD void rs_packed_phase_inverse_x(const RsTile &a, float *lds, int cnt, int tid)
{
	// the inverse's global scale rides on its x pass, the last one
	const TinyArgs tx = block_axis_args(a.i, 0, true);
	switch (a.ox) {
#define DSP_RS_CASE(N_) case N_: rs_packed_inverse_x<N_, C>(a, tx, lds, cnt, tid); break;
	DSP_RS_CASE(4) DSP_RS_CASE(8) DSP_RS_CASE(16) DSP_RS_CASE(32)
#undef DSP_RS_CASE
	}
}
// dither, one lane per plane (the device's walk for tiles of many small planes, and the host's for every tile: the CPU tests): thread = one
// oy x ox plane of one tile block, raster order; the byte takes the float's slot.  packed_dither_tile's dealing of the planes to the waves.  tab: dither_table(sf, norm); dprow: slots * ox doubles; thr NULL: the plain byte
template <int C>
DSP_HD void rs_packed_phase_dither(const RsTile &a, double sf, double norm, float *lds, int cnt, int tid, const double *tab, double *dprow, const double *thr,
                                   const TrcParams &tp)
{
	const int nb = cnt * C, nplanes = a.oz * nb, q = packed_dither_lanes(nplanes), wave = tid >> 6, lane = tid & 63;
	if (lane >= q) return;
	const int slot = wave * q + lane, nslots = (BLOCK_THREADS / 64) * q, my = rs_max(a.ny, a.oy);
	for (int pl = slot; pl < nplanes; pl += nslots) {
		const int z = pl / nb, gb = pl - z * nb;
		float *plane = lds + z * my * a.pitch + gb * a.tw;
		if (thr) dither_plane_tile<true>(plane, a.pitch, a.oy, a.ox, sf, norm, tab, dprow + slot, nslots, thr, &tp);
		else dither_plane_tile<false>(plane, a.pitch, a.oy, a.ox, sf, norm, tab, dprow + slot, nslots);
	}
}
// store: rs_packed_store_x's addresses and dwords, the bytes taken from the tile
template <int SX, int C>
DSP_HD void rs_packed_store_bytes(const RsTile &a, const float *lds, long long bout, int cnt, int tid)
{
	constexpr int W = SX * C / 4;
	const int ly = rs_log2(a.oy), lrows = ly + rs_log2(a.oz), my = rs_max(a.ny, a.oy);
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
			const float *q = base + c * cnt * a.tw;
#pragma unroll
			for (int p = 0; p < SX; p++) {
				const int i = C * p + c;
				w[i >> 2] |= dither_tile_byte(q + p) << (8 * (i & 3));
			}
		}
#pragma unroll
		for (int j = 0; j < W; j++) __builtin_memcpy(a.out8 + off + 4 * j, &w[j], 4);
	}
}
template <int C>
DSP_HD void rs_packed_phase_store_bytes(const RsTile &a, const float *lds, long long bout, int cnt, int tid)
{
	switch (a.ox) {
#define DSP_RS_CASE(N_) case N_: rs_packed_store_bytes<N_, C>(a, lds, bout, cnt, tid); break;
	DSP_RS_CASE(4) DSP_RS_CASE(8) DSP_RS_CASE(16) DSP_RS_CASE(32)
#undef DSP_RS_CASE
	}
}

// store behind rs_packed_inverse_x without -d: the floats of the tile quantised (or encoded) into the packed dwords -- rs_packed_store_x's second half.
// With a limit the store runs in these two phases: fused, a lane held the line, its transform and C lines' dwords at once (187 VGPRs at C = 4, two
// waves per SIMD); apart, neither half holds more than one of them.  The bytes are the same: the floats cross LDS unchanged.
template <int SX, int C, bool TRC>
DSP_HD void rs_packed_store_quant(const RsTile &a, const float *lds, long long bout, int cnt, int tid, const double *thr, const TrcParams &tp)
{
	constexpr int W = SX * C / 4;
	const int ly = rs_log2(a.oy), lrows = ly + rs_log2(a.oz), my = rs_max(a.ny, a.oy);
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
			float o[SX];
			const float4 *q = reinterpret_cast<const float4 *>(base + c * cnt * a.tw);
#pragma unroll
			for (int j = 0; j < SX / 4; j++) { const float4 v = q[j]; o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w; }
			packed_line_put<SX, C, TRC>(o, c, a.mul8, thr, tp, w);
		}
#pragma unroll
		for (int j = 0; j < W; j++) __builtin_memcpy(a.out8 + off + 4 * j, &w[j], 4);
	}
}
template <int C>
DSP_HD void rs_packed_phase_store_quant(const RsTile &a, const float *lds, long long bout, int cnt, int tid, const double *thr, const TrcParams &tp)
{
	switch (a.ox) {
#define DSP_RS_CASE(N_) \
	case N_: \
		if (thr) rs_packed_store_quant<N_, C, true>(a, lds, bout, cnt, tid, thr, tp); \
		else rs_packed_store_quant<N_, C, false>(a, lds, bout, cnt, tid, thr, tp); \
		break;
	DSP_RS_CASE(4) DSP_RS_CASE(8) DSP_RS_CASE(16) DSP_RS_CASE(32)
#undef DSP_RS_CASE
	}
}

#if defined(__HIP__)
// The device's dither phase: rs_packed_phase_dither's planes and bytes on oy lanes per plane instead of one.  Pixel (y, x) needs the errors of
// (y, x - 1) and (y - 1, x - 1 .. x + 1), so row y runs two pixels behind row y - 1: lane y of a plane's group takes x = t - 2 y at step t, and a
// plane is ox + 2 (oy - 1) steps, not oy ox.  A lane keeps its last three errors in registers; the row below reads them with shuffles inside the
// group (oy is 4 .. 32 and divides the wave), so no error row lies in LDS.  dither_pel applies the four terms at the receiving pixel in the
// reference's order, whatever the schedule (dither_core.h: dither_plane_wavefront states the same order on the host).
template <int C>
__device__ __forceinline__ void rs_packed_dither_wave(const RsTile &a, double sf, double norm, float *lds, int cnt, int tid, const double *tab, const double *thr,
                                                      const TrcParams &tp)
{
	const int nb = cnt * C, nplanes = a.oz * nb, h = a.oy, w = a.ox, my = rs_max(a.ny, a.oy);
	const int per = BLOCK_THREADS / h, y = tid & (h - 1), sub = tid / h, steps = w + 2 * (h - 1);
	for (int p0 = 0; p0 < nplanes; p0 += per) {
		const int pl = p0 + sub;
		const bool have = pl < nplanes;
		const int z = have ? pl / nb : 0, gb = have ? pl - z * nb : 0;
		float *row = lds + (z * my + y) * a.pitch + gb * a.tw;
		double h1 = 0.0, h2 = 0.0, h3 = 0.0;          // this lane's errors of the steps t - 1, t - 2, t - 3
		for (int t = 0; t < steps; t++) {
			// the row above: (y - 1, x + 1) was step t - 1 there, (y - 1, x) step t - 2, (y - 1, x - 1) step t - 3
			const double u1 = __shfl_up(h1, 1, h), u2 = __shfl_up(h2, 1, h), u3 = __shfl_up(h3, 1, h);
			const int x = t - 2 * y;
			double dp = h1;
			if (have && x >= 0 && x < w) {
				const bool up = y > 0, xp = x + 1 < w;
				const double dq = (up && xp) ? u1 : 0.0;
				const uint32_t b = thr ? dither_pel<true>(row[x], up, x > 0, xp, u3, u2, dq, h1, sf, norm, tab, dp, thr, &tp)
				                       : dither_pel<false>(row[x], up, x > 0, xp, u3, u2, dq, h1, sf, norm, tab, dp);
				__builtin_memcpy(row + x, &b, 4);
			}
			h3 = h2; h2 = h1; h1 = dp;
		}
	}
}

// the waves take the tile's cnt * C component blocks in turn; all 64 lanes enter the selection together (its ballots need them), a lane group
// without a block -- a short last group, or an odd cnt * C at two blocks per wave -- with active = false (block_rescale_topn.hip's rs_select).
// The lane that holds element 0 keeps the block's DC as it was before the selection (motion.c:650) for the components whose filter restores it (:734).
template <int K, int MX, int C>
__device__ __forceinline__ void rs_packed_select(float *lds, const RsTile &a, const BlockRsPackedArgs &pc, int E, unsigned int keep, int cnt, int tid)
{
	const int L = K > 1 ? 64 : E, per_wave = 64 / L, nb = cnt * C;
	const int sub = (tid & 63) / L, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	for (int g0 = wave * per_wave; g0 < nb; g0 += (BLOCK_THREADS / 64) * per_wave) {
		const int g = g0 + sub;
		const bool active = g < nb, lead = active && (tid & (L - 1)) == 0;
		const bool restore = motion_filter_restores_dc(packed_filter_of<C>(pc, packed_comp_of<C>(active ? g : g0, cnt), a.filt));
		float *blk = lds + (active ? g : g0) * a.tw;
		float dc = 0.f;
		if (restore && lead) dc = blk[0];
		topn_select_lds<K, MX>(blk, a.pitch, E, keep, L, active);
		if (restore && lead) blk[0] = dc;
	}
}

// One sequence for the three calls.  LIMIT: the unfused middle with the selection; DITHER: the store in the tile.
template <int C, bool LIMIT, bool DITHER>
__global__ void __launch_bounds__(BLOCK_THREADS) block_rescale_packed_wide_kernel(const BlockRsPackedWideArgs args)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	float *lds = reinterpret_cast<float *>(lds_raw);
	const RsTile a = rs_tile_of(args);
	unsigned char *behind = lds_raw + rs_tile_bytes(a);
	unsigned int *wg_coded = reinterpret_cast<unsigned int *>(behind + sizeof(TrcU8Tab));
	double *dtab = reinterpret_cast<double *>(behind + sizeof(TrcU8Tab) + 16);
	const int tid = threadIdx.x;
	if (tid == 0) *wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(args, blockIdx.x, bin, bout, cnt);
	if constexpr (DITHER) { for (int i = tid; i < 256; i += BLOCK_THREADS) dtab[i] = dither_table_entry(i, args.sf, args.norm); }
	const BlockTrc t = block_trc_stage(args.tab_in, args.tab_out, args.trc_out, behind, tid);
	const int nb = cnt * C;           // the tile's blocks
	unsigned long long mine = 0;
	if constexpr (LIMIT) {
		const RsTile all = rs_tile_unpruned(a);
		const RsKeys keys = rs_keys_of(args);
		rs_packed_phase_load<C>(all, lds, bin, cnt, tid, t.lut);
		rs_phase_zero_outside(a, lds, nb, tid);
		__syncthreads();
		if (a.nz > 1) { rs_phase_fwd_y(all, lds, nb, tid); __syncthreads(); }
		rs_phase_fwd_last_keys(a, keys, lds, nb, tid);
		__syncthreads();
		{
			const int E = rs_topn_elems(a);
			switch (a.tw * 128 + rs_topn_keys(E)) {
#define DSP_RS_SEL(K_, MX_) case MX_ * 128 + K_: rs_packed_select<K_, MX_, C>(lds, a, args, E, args.keep, cnt, tid); break;
			DSPFFT_RS_TOPN_SHAPES(DSP_RS_SEL)
#undef DSP_RS_SEL
			}
		}
		__syncthreads();
		rs_packed_phase_filt_inv_last<C>(a, args, lds, cnt, tid, mine);
	} else {
		rs_packed_phase_load<C>(a, lds, bin, cnt, tid, t.lut);
		__syncthreads();
		if (a.nz > 1) { rs_phase_fwd_y(a, lds, nb, tid); __syncthreads(); }
		rs_packed_phase_mid<C>(a, args, lds, cnt, tid, mine);
	}
	__syncthreads();
	if (a.nz > 1) { rs_phase_inv_y(a, lds, nb, tid); __syncthreads(); }
	if (a.filt.enabled && args.coded) block_coded_add(mine, wg_coded, args.coded);
	if constexpr (DITHER) {
		rs_packed_phase_inverse_x<C>(a, lds, cnt, tid);
		__syncthreads();
		if (args.by_rows) rs_packed_dither_wave<C>(a, args.sf, args.norm, lds, cnt, tid, dtab, t.thr, t.tp);
		else rs_packed_phase_dither<C>(a, args.sf, args.norm, lds, cnt, tid, dtab, dtab + 256, t.thr, t.tp);
		__syncthreads();
		rs_packed_phase_store_bytes<C>(a, lds, bout, cnt, tid);
	} else if constexpr (LIMIT) {
		rs_packed_phase_inverse_x<C>(a, lds, cnt, tid);
		__syncthreads();
		rs_packed_phase_store_quant<C>(a, lds, bout, cnt, tid, t.thr, t.tp);
	} else rs_packed_phase_store<C>(a, lds, bout, cnt, tid, t.thr, t.tp);
}

template <int C, bool LIMIT, bool DITHER>
static int launch_block_rescale_packed_wide(const BlockRsPackedWideArgs &a, int nwg, size_t lds, void *stream)
{
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_rescale_packed_wide_kernel<C, LIMIT, DITHER>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL((block_rescale_packed_wide_kernel<C, LIMIT, DITHER>), dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}
#endif

// what both launchers check of their arguments ahead of a launch; `lds`: the tile's bytes.  Returns the dynamic LDS of the launch, 0: refuse
inline size_t rs_packed_wide_lds(const BlockRsPackedWideArgs &a, int nwg, size_t lds)
{
	const bool two_d = a.nz == 1 && a.oz == 1;
	if (!rs_extent_ok(a.nx, two_d) || !rs_extent_ok(a.ox, two_d) || !rs_extent_ok(a.ny, two_d) || !rs_extent_ok(a.oy, two_d) ||
	    !(two_d || (rs_extent_ok(a.nz, false) && rs_extent_ok(a.oz, false)))) return 0;
	if (!a.in8 || !a.out8 || a.comps < 2 || a.comps > PACKED_MAX_COMPS) return 0;
	const RsTile t = rs_tile_of(a);
	if (lds != rs_tile_bytes(t) || (lds & 15) || a.G < 1 || a.pitch != a.comps * a.G * a.tw || a.tw != rs_packed_wide_tw(a.nx, a.ox, a.keep != 0) || nwg < 1) return 0;
	if (a.keep) {
		const int E = rs_topn_elems(t);
		bool listed = false;
#define DSP_RS_SEL(K_, MX_) listed = listed || (a.tw == MX_ && rs_topn_keys(E) == K_);
		DSPFFT_RS_TOPN_SHAPES(DSP_RS_SEL)
#undef DSP_RS_SEL
		if (!listed || a.keep >= (unsigned int)E) return 0;
	}
	if (a.dither && a.slots != packed_dither_slots(a.oz, a.comps, a.G)) return 0;
	lds += sizeof(TrcU8Tab) + 16 + rs_packed_wide_dither_bytes(a.ox, a.oz, a.comps, a.G, a.dither != 0, a.by_rows != 0);
	return lds > 64 * 1024 ? 0 : lds;
}

}  // namespace dspfft
