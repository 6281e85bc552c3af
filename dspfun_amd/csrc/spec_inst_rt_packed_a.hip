// spec_inst_rt_packed_a.hip -- the fused column roundtrip with the filter of PACKED pixels in the middle (spec_kernels.h
// col_roundtrip_packed_kernel; dspfft_execute_roundtrip_u8_packed_frames), instantiated for the first group of listed column specs, and the
// lookup of both groups.  Translation units of their own: the planar roundtrip kernels (spec_inst_rt_a/b.hip) are what they were.
#include "spec_kernels.h"

namespace dspfft {
#define DSP_RT_PACKED_ENTRY(N, K, T, ...) rt_packed_launcher<N, K, T, ColSpec<N, K, T, __VA_ARGS__>>(),
static const RtPackedLaunch g_rt_packed_a[] = {DSPFFT_COL_SPECS_A(DSP_RT_PACKED_ENTRY)};
constexpr int N_RT_PACKED_A = (int)(sizeof g_rt_packed_a / sizeof g_rt_packed_a[0]);
RtPackedLaunch rt_packed_group_b(int i);      // spec_inst_rt_packed_b.hip; nullptr past its end

// spec_registry.inc's column entries in their order (group A, then group B): the ids are be_find_spec's
static RtPackedLaunch rt_packed_of(int id) { return id < 0 ? nullptr : id < N_RT_PACKED_A ? g_rt_packed_a[id] : rt_packed_group_b(id - N_RT_PACKED_A); }

// whether column spec `id` has the packed twin, and its launch (engine.cpp reaches both through weak references: the CPU emulation links
// engine.cpp without these units)
bool be_roundtrip_packed_has(int id) { return rt_packed_of(id) != nullptr; }
int be_launch_roundtrip_packed(int id, const PassArgs &af, const PassArgs &ai, const MotionFilterPacked &filt, unsigned long long *coded, int nwg, void *stream)
{
	const RtPackedLaunch f = rt_packed_of(id);
	return f ? f(af, ai, filt, coded, nwg, stream) : -5;
}
}  // namespace dspfft
