// spec_inst_row_trc.hip -- the planar 8-bit row ends with motion --linear (dspfft_plan_set_u8_trc): row_spec_u8_kernel's phases (dct_spec.h,
// instantiated with TRC) with the transfer characteristic's decode table at the REDFT10 load and its threshold table at the REDFT01 store.
// A translation unit of its own: the plain 8-bit kernels (spec_inst_row.hip) are what they were.
//
// The table the kernel needs (1 KB of floats / 2 KB of doubles) lies in LDS behind the plane: the REDFT10 kernel pays one more barrier for
// the copy, in front of phase 0.  Left in global memory for the vector L1 (spec_row_trc.h TLDS = false) both kernels are slower; only
// tools/kstamp.hip instantiates that form (DESIGN.md has both measured).
#include "spec_row_trc.h"

namespace dspfft {

template <class S, int KIND>
int launch_row_spec_u8_trc(const PassArgs &a, const U8IOTrc &io, int nwork, void *stream)
{
	if constexpr (S::U8_OK) {
		if (!is_plain(a)) return -5;                 // (the kernel is the plain instantiation only)
		if (KIND == KIND_REDFT10 ? !io.tab_in : !io.tab_out) return -5;
		constexpr size_t LDS = S::LDS + trc_lds_bytes<KIND>();
		static DevOnce once;
		if (int lds_rc = allow_lds_dev(once, LDS, row_spec_u8_trc_kernel<S, KIND, true>)) return lds_rc;
		hipLaunchKernelGGL((row_spec_u8_trc_kernel<S, KIND, true>), dim3(nwork), dim3(S::T), LDS, (hipStream_t)stream, a, io);
		HIPCHK(hipGetLastError());
		return 0;
	} else return -5;
}

// spec_registry.inc's row entries in their order: the ids are be_find_spec's
struct TrcRowEntry { int (*launch[2])(const PassArgs &, const U8IOTrc &, int, void *); };
#define DSP_TRC_ROW_ENTRY(N, C, T, ...) {{launch_row_spec_u8_trc<RowSpec<N, C, T, __VA_ARGS__>, 0>, launch_row_spec_u8_trc<RowSpec<N, C, T, __VA_ARGS__>, 1>}},
static const TrcRowEntry g_trc_row_specs[] = {DSPFFT_ROW_SPECS(DSP_TRC_ROW_ENTRY)};

}  // namespace dspfft

/* run_pass_u8's launch when the 8-bit end has a transfer characteristic (engine.cpp reaches this through a weak reference: the CPU
 * emulation links engine.cpp without this unit).  id: a row spec for which be_spec_has_u8 holds. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_row_u8_trc_launch(int id, const dspfft::PassArgs *a, const dspfft::U8IOTrc *io, int nwg, void *stream)
{
	using namespace dspfft;
	if (id < 0 || id >= (int)(sizeof g_trc_row_specs / sizeof g_trc_row_specs[0])) return -5;
	return g_trc_row_specs[id].launch[a->kind](*a, *io, nwg, stream);
}
