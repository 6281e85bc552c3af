// block_spec_packed_core.h -- motion --spectrogram and --ispectrogram over small blocks of PACKED 8-bit pixels (rgb24, rgba ...: the formats
// the reference switches to for these modes, motion/motion.c:313-318): block_packed_core.h's tile and linear ends with block_spec_core.h's
// encode and decode at the cut.  What is new here are the two encoded ends of a line.
//   spectrogram   packed_load_x, block_lines_y / _z forward over cnt * C tile blocks | packed_spec_store: tile -> the component's filter ->
//                 encode -> the line's packed dwords
//   ispectrogram  packed_ispec_load: the line's packed dwords -> decode -> the component's filter -> tile | block_lines_z / _y inverse,
//                 packed_store_x
// One thread per x line of a PIXEL block in both, as in the phases they stand in for.  A line is walked four pixels at a time: 4 C bytes = C
// whole dwords at a constant place inside the step, so a byte's dword and shift are constants after unrolling and the dwords stay in
// registers, while the tile is read and written as one float4 per component (NX is a multiple of 4).  Every component of a pixel block is a
// block of its own (:613-615): --spectrogram=abs takes c from that component block's DC (:650,755), tile element 0 of tile block c * cnt + g,
// which nothing has written since the last forward axis.
// Plain C++17 for device (hipcc) and the CPU emulation of the phases (g++, tests/test_motion_spec_packed_cpu.py).
#pragma once
#include "block_packed_core.h"
#include "block_spec_core.h"

namespace dspfft {

// keep = 0 and the tables NULL: neither a coefficient limit nor motion --linear goes with a spectrogram.  spectrogram: f holds the plan's
// scales; ispectrogram: i does, and mul8 is the 8-bit store's factor.
struct BlockSpecPackedArgs : BlockPackedArgs {
	MotionSpec sp;
};

// spectrogram's last phase (motion.c:650,683-744,755-776) on the component-major tile
template <int NX, int NY, int NZ, int C>
DSP_HD void packed_spec_store(const BlockSpecPackedArgs &a, const float *lds, long long bout, int cnt, int tid, unsigned long long &coded)
{
	const MotionSpec &sp = a.sp;
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
		const int z = row / NY, y = row - z * NY;
		const long long off = bout + (long long)g * a.sxb_out + (long long)z * a.sz_out + (long long)y * a.sy_out;
		double cc[C];
		float fm[C], fcc[C];
		int fon[C];
#pragma unroll
		for (int c = 0; c < C; c++) {
			cc[c] = sp.mode == MOTION_MODE_ABS ? motion_abs_c(lds[(c * cnt + g) * NX], sp.scalefactor, sp.norm) : sp.c;     // :755
			const MotionFast t = motion_fast_of(sp.mode, sp.scalefactor, sp.norm, cc[c]);
			fm[c] = t.m; fcc[c] = t.cc; fon[c] = t.on;
		}
		const bool filt = a.filt.enabled && y < a.filt.ah && z < a.filt.ad;
#pragma unroll 1
		for (int j = 0; j < NX / 4; j++) {
			uint32_t w[C];
#pragma unroll
			for (int k = 0; k < C; k++) w[k] = 0;
#pragma unroll
			for (int c = 0; c < C; c++) {
				const float4 t = *reinterpret_cast<const float4 *>(lds + row * a.pitch + (c * cnt + g) * NX + 4 * j);
				float v[4] = {t.x, t.y, t.z, t.w};
				if (filt) {
					const MotionFilter f = packed_filter_of<C>(a, c);
#pragma unroll
					for (int k = 0; k < 4; k++) if (4 * j + k < f.aw) v[k] = motion_filter_at(f, z, y, 4 * j + k, v[k], coded);
				}
				MotionFast fast;
				fast.m = fm[c]; fast.cc = fcc[c]; fast.on = fon[c];
#pragma unroll
				for (int k = 0; k < 4; k++) {                                                                             // :759-776
					const int i = C * k + c;
					w[i >> 2] |= motion_spec_byte(v[k], sp.mode, sp.scalefactor, sp.norm, cc[c], fast) << (8 * (i & 3));
				}
			}
#pragma unroll
			for (int k = 0; k < C; k++) __builtin_memcpy(a.out8 + off + 4 * (C * j + k), &w[k], 4);
		}
	}
}

// ispectrogram's first phase (motion.c:621-637,650,683-744) into the component-major tile
template <int NX, int NY, int NZ, int C>
DSP_HD void packed_ispec_load(const BlockSpecPackedArgs &a, float *lds, long long bin, int cnt, int tid, unsigned long long &coded)
{
	const MotionSpec &sp = a.sp;
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
		const int z = row / NY, y = row - z * NY;
		const long long off = bin + (long long)g * a.sxb_in + (long long)z * a.sz_in + (long long)y * a.sy_in;
		const bool filt = a.filt.enabled && y < a.filt.ah && z < a.filt.ad;
#pragma unroll 1
		for (int j = 0; j < NX / 4; j++) {
			uint32_t w[C];
#pragma unroll
			for (int k = 0; k < C; k++) __builtin_memcpy(&w[k], a.in8 + off + 4 * (C * j + k), 4);
#pragma unroll
			for (int c = 0; c < C; c++) {
				float v[4];
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const int i = C * k + c;
					const double pel = (double)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);                                     // :625
					v[k] = (float)motion_load_pel(pel, sp.mode, sp.c, sp.norm);                                            // :627-637
				}
				if (filt) {
					const MotionFilter f = packed_filter_of<C>(a, c);
#pragma unroll
					for (int k = 0; k < 4; k++) if (4 * j + k < f.aw) v[k] = motion_filter_at(f, z, y, 4 * j + k, v[k], coded);
				}
				float4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
				*reinterpret_cast<float4 *>(lds + row * a.pitch + (c * cnt + g) * NX + 4 * j) = o;
			}
		}
	}
}

}  // namespace dspfft
