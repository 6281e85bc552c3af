// spec_inst_row_u8c.hip -- the 8-bit row ends of INTERLEAVED RGB lines (dct_spec.h RowU8Rgb): row_spec_u8_kernel instantiated with that trait
// for the lengths spec's images meet first, each from its DSPFFT_ROW_SPECS entry (same radices, same threads).  A translation unit of its
// own: the plain kernels and the planar 8-bit ones (spec_inst_row.hip) are what they were.
#include "spec_kernels.h"

namespace dspfft {

constexpr bool u8c_listed(int n, int c) { return c == 3 && (n == 3840 || n == 1920 || n == 7680 || n == 960 || n == 512 || n == 256); }

typedef int (*U8cLaunch)(const PassArgs &, const U8IO &, int, void *);
template <class S, int KIND> constexpr U8cLaunch u8c_launcher()
{
	if constexpr (u8c_listed(S::N, S::C)) return launch_row_spec_u8<RowU8Rgb<S>, KIND>; else return nullptr;
}

// spec_registry.inc's row entries in their order: the ids are be_find_spec's
struct U8cRowEntry { U8cLaunch launch[2]; };
#define DSP_U8C_ROW_ENTRY(N, C, T, ...) {{u8c_launcher<RowSpec<N, C, T, __VA_ARGS__>, 0>(), u8c_launcher<RowSpec<N, C, T, __VA_ARGS__>, 1>()}},
static const U8cRowEntry g_u8c_row_specs[] = {DSPFFT_ROW_SPECS(DSP_U8C_ROW_ENTRY)};
constexpr int N_U8C = (int)(sizeof g_u8c_row_specs / sizeof g_u8c_row_specs[0]);

}  // namespace dspfft

/* whether row spec `id` has interleaved 8-bit ends, and their launch (engine.cpp reaches both through weak references: the CPU emulation
 * links engine.cpp without this unit).  The caller has checked that every line's byte offset is a multiple of 4. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_row_u8c_has(int id)
{
	return id >= 0 && id < dspfft::N_U8C && dspfft::g_u8c_row_specs[id].launch[0] != nullptr;
}
extern "C" __attribute__((visibility("hidden"))) int dspfft_row_u8c_launch(int id, const dspfft::PassArgs *a, const dspfft::U8IO *io, int nwg, void *stream)
{
	if (!dspfft_row_u8c_has(id)) return -5;
	return dspfft::g_u8c_row_specs[id].launch[a->kind](*a, *io, nwg, stream);
}
