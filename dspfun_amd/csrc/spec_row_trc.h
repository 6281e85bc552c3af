// spec_row_trc.h -- row_spec_u8_kernel (spec_kernels.h) with motion --linear's tables at its 8-bit end: the kernel of spec_inst_row_trc.hip,
// in a header so that tools/kstamp.hip can stamp it.  Device code only.
#pragma once
#include "spec_kernels.h"

namespace dspfft {


template <int KIND> constexpr size_t trc_lds_bytes() { return KIND == KIND_REDFT10 ? 256 * sizeof(float) : 256 * sizeof(double); }

template <class S, int KIND, bool TLDS>
__global__ void __launch_bounds__(S::T, (u8_waves_per_simd<S, KIND>())) row_spec_u8_trc_kernel(const typename S::PA a_, const U8IOTrc io_)
{
	const typename S::PA a = plain_args(a_);
	U8IOTrc io = io_;
	if constexpr (KIND == KIND_REDFT10) { __builtin_assume(io.in != nullptr); io.out = nullptr; } else { __builtin_assume(io.out != nullptr); io.in = nullptr; }
	extern __shared__ __attribute__((aligned(32))) unsigned char lds[];
	typename S::CX *planes = reinterpret_cast<typename S::CX *>(lds);
	const int tid = threadIdx.x;
	typename S::template State<KIND> st;
	long long bin, bout;
	row_base(a, blockIdx.x, bin, bout);
	DSP_STAMP(0);
	// the table's loads go out first, so that its copy into LDS waits for them alone and not for the line's
	constexpr int TR = (256 + S::T - 1) / S::T;
	float lv[TR];
	double tv[TR];
	if constexpr (TLDS) {
		static_for<0, TR>([&](auto i) {
			const int k = tid + i * S::T;
			if ((i + 1) * S::T <= 256 || k < 256) { if constexpr (KIND == KIND_REDFT10) lv[i] = io.tab_in->lut[k]; else tv[i] = io.tab_out->thr[k]; }
		});
	}
	S::template prefetch_m<KIND, false, false, true>(a, bin, tid, st, &io, nullptr);
	S::fetch_stage_twiddles(a, tid, st);
	if constexpr (TLDS) {
		// (TrcU8Tab's members by offset: thr at 0, lut behind it; the kernel holds only the one it needs, placed so that the member lands on it)
		unsigned char *at = lds + S::LDS;
		static_for<0, TR>([&](auto i) {
			const int k = tid + i * S::T;
			if ((i + 1) * S::T <= 256 || k < 256) {
				if constexpr (KIND == KIND_REDFT10) reinterpret_cast<float *>(at)[k] = lv[i]; else reinterpret_cast<double *>(at)[k] = tv[i];
			}
		});
		if constexpr (KIND == KIND_REDFT10) { io.tab_in = reinterpret_cast<const TrcU8Tab *>(at - offsetof(TrcU8Tab, lut)); __syncthreads(); }
		else io.tab_out = reinterpret_cast<const TrcU8Tab *>(at);
	}
	S::template phase<KIND, 0, decltype(st), false, false, true>(a, planes, bout, tid, st, &io);
	__syncthreads();
	DSP_STAMP(1);
	static_for<1, S::NPH>([&](auto ph) {
		{
			S::template phase<KIND, ph, decltype(st), false, true, true>(a, planes, bout, tid, st, &io);
			if constexpr (ph + 1 < S::NPH) __syncthreads();
			DSP_STAMP(1 + ph);
		}
	});
}

}  // namespace dspfft
