// block_spec_core.h -- motion --spectrogram and --ispectrogram over small blocks: the two phases that turn the fused block roundtrip
// (block_core.h, block_rt.h) into its halves.
//   spectrogram   block_load_x, block_lines_y / _z forward | block_spec_store: tile -> filter -> encode -> packed bytes or float4
//   ispectrogram  block_ispec_load: packed bytes or float4 -> decode -> filter -> tile | block_lines_z / _y inverse, block_store_x
// (motion/motion.c:617-776 with spec / ispec set: the forward transform is skipped with --ispec, :640, the inverse with --spec, :746).
// One thread per x line of a block in both, as in the phases they stand in for.  --spectrogram=abs needs the block's DC from before the
// filter (:650,755): the store phase reads it from the tile, which nothing has written since the last forward axis.
// Float pixels (motion's float_pixels: sample * 255 on load, pel / 255 on store, :623,774): the end next to the encode or decode does it
// here; at the other end it is a factor of a linear transform, which the engine folds into the plan's global scale (engine.cpp: spec_block).
// Plain C++17 for device (hipcc) and the CPU test (g++).
#pragma once
#include "block_core.h"

namespace dspfft {

struct BlockSpecArgs : BlockGeom {
	const float *in;
	float *out;
	const uint8_t *in8;           // in8 / out8 replace in / out when set (8-bit pixels in the same element layout)
	uint8_t *out8;
	BlockScales s;                // the plan's scales (a float-pixel call: times 255, or times out_mul / 255)
	MotionFilter filt;            // filt.enabled = 0: no filter; positions are the block's own (z, y, x)
	unsigned long long *coded;
	MotionSpec sp;
	double mul8;                  // ispectrogram's 8-bit store: quantise(value * mul8)
};

// spectrogram's last phase (motion.c:650,683-744,755-776): every coefficient of the tile filtered, encoded and stored
template <int NX, int NY, int NZ, bool U8>
DSP_HD void block_spec_store(const BlockSpecArgs &a, const float *lds, long long bout, int cnt, int tid, unsigned long long &coded)
{
	const MotionSpec &sp = a.sp;
	const MotionFilter &f = a.filt;
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
		const int z = row / NY, y = row - z * NY;
		const long long off = bout + (long long)g * a.sxb_out + (long long)z * a.sz_out + (long long)y * a.sy_out;
		const double cc = sp.mode == MOTION_MODE_ABS ? motion_abs_c(lds[g * NX], sp.scalefactor, sp.norm) : sp.c;      // :755
		const MotionFast fast = motion_fast_of(sp.mode, sp.scalefactor, sp.norm, cc);
		const bool filt = f.enabled && y < f.ah && z < f.ad;
		const float4 *q = reinterpret_cast<const float4 *>(lds + row * a.pitch + g * NX);
#pragma unroll 1
		for (int j = 0; j < NX / 4; j++) {
			const float4 t = q[j];
			float v[4] = {t.x, t.y, t.z, t.w};
			if (filt) {
#pragma unroll
				for (int k = 0; k < 4; k++) if (4 * j + k < f.aw) v[k] = motion_filter_at(f, z, y, 4 * j + k, v[k], coded);
			}
			if constexpr (U8) {
				uint32_t w4 = 0;                                                                                         // :759-776
#pragma unroll
				for (int k = 0; k < 4; k++) w4 |= motion_spec_byte(v[k], sp.mode, sp.scalefactor, sp.norm, cc, fast) << (8 * k);
				__builtin_memcpy(a.out8 + off + 4 * j, &w4, 4);
			} else {
				double pel[4];
#pragma unroll
				for (int k = 0; k < 4; k++) pel[k] = motion_store_pel((double)v[k], sp.mode, sp.scalefactor, sp.norm, cc);   // :759-771
				float4 o;                                                                                                 // :774
				o.x = (float)(pel[0] / 255); o.y = (float)(pel[1] / 255); o.z = (float)(pel[2] / 255); o.w = (float)(pel[3] / 255);
				reinterpret_cast<float4 *>(a.out + off)[j] = o;
			}
		}
	}
}

// ispectrogram's first phase (motion.c:621-637,650,683-744): every pixel decoded to the coefficient it stands for, filtered, into the tile
template <int NX, int NY, int NZ, bool U8>
DSP_HD void block_ispec_load(const BlockSpecArgs &a, float *lds, long long bin, int cnt, int tid, unsigned long long &coded)
{
	const MotionSpec &sp = a.sp;
	const MotionFilter &f = a.filt;
	const int lines = NZ * NY * cnt;
	for (int l = tid; l < lines; l += BLOCK_THREADS) {
		int row, g;
		block_line_of(a, l, NZ * NY, cnt, row, g);
		const int z = row / NY, y = row - z * NY;
		const long long off = bin + (long long)g * a.sxb_in + (long long)z * a.sz_in + (long long)y * a.sy_in;
		const bool filt = f.enabled && y < f.ah && z < f.ad;
		float4 *q = reinterpret_cast<float4 *>(lds + row * a.pitch + g * NX);
#pragma unroll 1
		for (int j = 0; j < NX / 4; j++) {
			double pel[4];
			if constexpr (U8) {
				uint32_t w4;
				__builtin_memcpy(&w4, a.in8 + off + 4 * j, 4);
#pragma unroll
				for (int k = 0; k < 4; k++) pel[k] = (double)((w4 >> (8 * k)) & 0xffu);                                  // :625
			} else {
				const float4 t = reinterpret_cast<const float4 *>(a.in + off)[j];
				const float p[4] = {t.x * 255.0f, t.y * 255.0f, t.z * 255.0f, t.w * 255.0f};                           // :623 float * int: a float product
#pragma unroll
				for (int k = 0; k < 4; k++) pel[k] = (double)p[k];
			}
			float v[4];
#pragma unroll
			for (int k = 0; k < 4; k++) v[k] = (float)motion_load_pel(pel[k], sp.mode, sp.c, sp.norm);                 // :627-637
			if (filt) {
#pragma unroll
				for (int k = 0; k < 4; k++) if (4 * j + k < f.aw) v[k] = motion_filter_at(f, z, y, 4 * j + k, v[k], coded);
			}
			float4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
			q[j] = o;
		}
	}
}

}  // namespace dspfft
