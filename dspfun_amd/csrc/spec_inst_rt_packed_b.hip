// spec_inst_rt_packed_b.hip -- the fused column roundtrip of packed pixels for the second group of listed column specs (see
// spec_inst_rt_packed_a.hip)
#include "spec_kernels.h"

namespace dspfft {
#define DSP_RT_PACKED_ENTRY(N, K, T, ...) rt_packed_launcher<N, K, T, ColSpec<N, K, T, __VA_ARGS__>>(),
static const RtPackedLaunch g_rt_packed_b[] = {DSPFFT_COL_SPECS_B(DSP_RT_PACKED_ENTRY)};
constexpr int N_RT_PACKED_B = (int)(sizeof g_rt_packed_b / sizeof g_rt_packed_b[0]);
RtPackedLaunch rt_packed_group_b(int i) { return i >= 0 && i < N_RT_PACKED_B ? g_rt_packed_b[i] : nullptr; }
}  // namespace dspfft
