// motion_filter_packed.h -- motion_filter.h's filter over full frames of PACKED pixels: a dense [frames][h][w][C] buffer of coefficients in
// which every component of a frame is a block of its own (motion/motion.c:613-615).  Element e of a frame lies in row y = e / (w C), at pixel
// x = (e % (w C)) / C, in component c = e % C, and goes through motion_filter_at at (0, y, x) with component c's damp, boost and grey_add
// (motion -D / -B r:g:b:a, :235-236,683-738; indexed by BYTE POSITION, as dspfft_motion_packed stores them); every other field is shared.
// Used by the stand-alone kernel (motion_filter_packed.hip: dspfft_motion_filter_packed) and by the fused column roundtrip of
// dspfft_execute_roundtrip_u8_packed_frames (spec_fused.h: PackedFilterOp).
#pragma once
#include "motion_filter.h"

namespace dspfft {

struct MotionFilterPacked {
	MotionFilter f;                          // the shared fields: active (1, ah, aw) in PIXELS, band, thresholds, preserve_dc, quantiser; f.damp, f.boost, f.grey_add are not read
	int comps, h, w;                         // C = 2, 3 or 4; the frame's rows and pixels per row
	uint32_t row, per;                       // w C and h w C elements
	FastDiv div_row, div_per;
	float damp[4], boost[4], grey_add[4];
	int quant_only;                          // nothing but the quantiser acts on ANY component: positions and components are not needed
};

// `f` as motion_filter_from leaves it; damp, boost, grey_add: C values by byte position
inline void motion_filter_packed_set(MotionFilterPacked &p, const MotionFilter &f, int h, int w, int comps, const float *damp, const float *boost, const float *grey_add)
{
	p.f = f; p.comps = comps; p.h = h; p.w = w;
	p.row = (uint32_t)w * (uint32_t)comps; p.per = (uint32_t)h * p.row;
	p.div_row = motion_filter_div(p.row); p.div_per = motion_filter_div(p.per);
	p.quant_only = f.ad >= 1 && f.ah >= h && f.aw >= w;      // (a smaller active block leaves the pixels outside it alone)
	for (int c = 0; c < 4; c++) {
		p.damp[c] = c < comps ? damp[c] : 1.f; p.boost[c] = c < comps ? boost[c] : 1.f; p.grey_add[c] = c < comps ? grey_add[c] : 0.f;
		MotionFilter g = f;
		g.damp = p.damp[c]; g.boost = p.boost[c];
		motion_filter_set_divs(g, 1);
		p.quant_only = p.quant_only && g.quant_only;
	}
	p.f.quant_only = p.quant_only;
}

// A select between loads of p.damp[k] becomes ONE load at a selected address, and an argument structure that is indexed at run time is kept
// in scratch memory by every kernel that takes it (204 bytes a lane in the fused column kernels).  Pinned in registers first (DSP_PIN1: a
// constraint, no instruction), the selects are between registers.
DSP_HD float motion_packed_pick(const float (&v)[4], int c)
{
	float v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
	DSP_PIN1(v0); DSP_PIN1(v1); DSP_PIN1(v2); DSP_PIN1(v3);
	return c == 3 ? v3 : c == 2 ? v2 : c == 1 ? v1 : v0;
}

// one coefficient of row y, pixel x, component c: motion_filter_at on the shared filter with the component's three values; pixels outside
// the active block are returned unchanged
DSP_HD float motion_filter_packed_at(const MotionFilterPacked &p, int y, int x, int c, float v, unsigned long long &coded)
{
	if (x >= p.f.aw || y >= p.f.ah || p.f.ad < 1) return v;
	MotionFilter g = p.f;
	g.damp = motion_packed_pick(p.damp, c); g.boost = motion_packed_pick(p.boost, c); g.grey_add = motion_packed_pick(p.grey_add, c);
	return motion_filter_at(g, 0, y, x, v, coded);
}

// element i (< w C) of a row into pixel and component: no division by a run-time C
template <int C> DSP_HD void motion_packed_split(uint32_t i, int &x, int &c) { const uint32_t q = i / (uint32_t)C; x = (int)q; c = (int)(i - q * (uint32_t)C); }
DSP_HD void motion_packed_split(int comps, uint32_t i, int &x, int &c)
{
	switch (comps) {
	case 2: motion_packed_split<2>(i, x, c); break;
	case 3: motion_packed_split<3>(i, x, c); break;
	default: motion_packed_split<4>(i, x, c); break;
	}
}

// one element at row y, element i of the row
DSP_HD float motion_filter_packed_elem(const MotionFilterPacked &p, uint32_t y, uint32_t i, float v, unsigned long long &coded)
{
	int x, c;
	motion_packed_split(p.comps, i, x, c);
	return motion_filter_packed_at(p, (int)y, x, c, v, coded);
}

// one step of a walk over consecutive elements: filters r at (yy, x, c) and moves on -- past a pixel, a row (w C no multiple of 4) and a
// frame (the row after a frame's last is the next frame's first)
DSP_HD void motion_filter_packed_step(const MotionFilterPacked &p, int &yy, int &x, int &c, float &r, unsigned long long &coded)
{
	r = motion_filter_packed_at(p, yy, x, c, r, coded);
	if (++c == p.comps) { c = 0; if (++x == p.w) { x = 0; if (++yy == p.h) yy = 0; } }
	DSP_SCHED_FENCE();
}
DSP_HD void motion_quantise_step(const MotionFilter &f, float &r, unsigned int &nz)
{
	r = motion_quantise(r, f.quantizer, f.rquant);                                                 // motion.c:740-744
	nz += (r != 0.f);
	DSP_SCHED_FENCE();
}

// four consecutive elements of the dense buffer, the first at row y, element i of the row
DSP_HD float4 motion_filter_packed4_at(const MotionFilterPacked &p, uint32_t y, uint32_t i, float4 v, unsigned long long &coded)
{
	if (p.quant_only) {
		unsigned int nz = 0;
		motion_quantise_step(p.f, v.x, nz); motion_quantise_step(p.f, v.y, nz); motion_quantise_step(p.f, v.z, nz); motion_quantise_step(p.f, v.w, nz);
		coded += nz;
		return v;
	}
	int x, c, yy = (int)y;
	motion_packed_split(p.comps, i, x, c);
	motion_filter_packed_step(p, yy, x, c, v.x, coded); motion_filter_packed_step(p, yy, x, c, v.y, coded);
	motion_filter_packed_step(p, yy, x, c, v.z, coded); motion_filter_packed_step(p, yy, x, c, v.w, coded);
	return v;
}

// ... starting at element offset e (< 2^31) of the dense buffer of whole frames
DSP_HD float4 motion_filter_packed4(const MotionFilterPacked &p, uint32_t e, float4 v, unsigned long long &coded)
{
	if (p.quant_only) return motion_filter_packed4_at(p, 0, 0, v, coded);
	const uint32_t el = e - p.div_per.div_exact(e) * p.per;
	const uint32_t y = p.div_row.div_exact(el);
	return motion_filter_packed4_at(p, y, el - y * p.row, v, coded);
}

}  // namespace dspfft
