// rotate.hip -- rotate (motion/rotate.c): dspfft_rotate_parse and dspfft_rotate.  The kernels are rotate_core.h's phases, one launch per call:
// rows where input x stays output x (the unsigned identity among them), LDS tiles where it moves.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "../../include/dspfft.h"
#include "rotate_core.h"

extern "C" int dspfft_motion_set_error(const char *m);     // motion_ops.hip: the message dspfft_motion_last_error returns

namespace dspfft {

template <int E, bool FLIP>
__global__ void __launch_bounds__(ROT_THREADS) rotate_rows_kernel(const RotArgs a)
{
	rot_rows_thread<E, FLIP>(a, blockIdx.x, threadIdx.x);
}

__global__ void __launch_bounds__(ROT_THREADS) rotate_tile_b_kernel(const RotArgs a)
{
	__shared__ __attribute__((aligned(16))) uint32_t lds[ROT_TILE_B * ROT_TILE_B / 4];
	const RotTile t = rot_tile_of(a, blockIdx.x);
	rot_tile_load_b(a, t, lds, threadIdx.x);
	__syncthreads();
	rot_tile_store_b(a, t, lds, threadIdx.x);
}

template <int E>
__global__ void __launch_bounds__(ROT_THREADS) rotate_tile_e_kernel(const RotArgs a)
{
	__shared__ uint32_t lds[ROT_TILE_E * ROT_PITCH_E];
	const RotTile t = rot_tile_of(a, blockIdx.x);
	rot_tile_load_e<E>(a, t, lds, threadIdx.x);
	__syncthreads();
	rot_tile_store_e<E>(a, t, lds, threadIdx.x);
}

template <int E>
static void rows_launch(const RotArgs &a, hipStream_t s)
{
	if (a.flip[0]) hipLaunchKernelGGL((rotate_rows_kernel<E, true>), dim3((unsigned)a.nwg), dim3(ROT_THREADS), 0, s, a);
	else hipLaunchKernelGGL((rotate_rows_kernel<1, false>), dim3((unsigned)a.nwg), dim3(ROT_THREADS), 0, s, a);
}

static int rot_bad(const char *what)
{
	char m[200];
	snprintf(m, sizeof m, "rotate: %s", what);
	dspfft_motion_set_error(m);
	return -2;
}

}  // namespace dspfft

extern "C" int dspfft_rotate_parse(const char *spec, int map[3], int invert[3])
{
	if (!spec || !map || !invert) return 1;
	map[0] = map[1] = map[2] = -1;
	invert[0] = invert[1] = invert[2] = 0;
	// rotate.c:76-86: the pointer moves past a sign, the index past a letter
	const char *s = spec;
	for (int i = 0; i < 3; i++) {
		if (s[i] == '-') { invert[i] = 1; s++; }
		else if (s[i] == '+') s++;
		if (!s[i]) break;
		map[i] = s[i] - 'x';
	}
	for (int i = 0; i < 3; i++) if (map[i] < 0 || map[i] > 2) return 1;      // :87-89
	return dspfft::rot_is_permutation(map) ? 0 : 2;
}

extern "C" int dspfft_rotate(void *d_out, const void *d_in, const uint64_t len[3], int elem_bytes, const int map[3], const int invert[3], void *hip_stream)
{
	using namespace dspfft;
	if (!d_out || !d_in || !len || !map || !invert) return rot_bad("null pointer");
	if (elem_bytes < 1 || elem_bytes > 4) return rot_bad("element size outside 1..4 bytes");
	if (!len[0] || !len[1] || !len[2]) return rot_bad("zero extent");
	if (!rot_is_permutation(map)) return rot_bad("the map is no permutation of the three axes");
	const uint64_t lim = UINT64_MAX / 8;
	if (len[0] > lim / (uint64_t)elem_bytes || len[1] > lim / (len[0] * (uint64_t)elem_bytes) || len[2] > lim / (len[0] * len[1] * (uint64_t)elem_bytes))
		return rot_bad("the clip's byte count does not fit 64 bits");
	const uint64_t bytes = len[0] * len[1] * len[2] * (uint64_t)elem_bytes;
	const uint64_t pi = (uint64_t)(uintptr_t)d_in, po = (uint64_t)(uintptr_t)d_out;
	if ((elem_bytes == 2 || elem_bytes == 4) && ((pi | po) & (uint64_t)(elem_bytes - 1))) return rot_bad("pointers must be aligned to the element");
	if (pi > UINT64_MAX - bytes || po > UINT64_MAX - bytes) return rot_bad("the clip's byte count does not fit 64 bits");
	if (pi < po + bytes && po < pi + bytes) return rot_bad("input and output overlap (there is no in-place form)");
	RotArgs a;
	rot_setup(a, len, elem_bytes, map, invert);
	a.in = static_cast<const unsigned char *>(d_in);
	a.out = static_cast<unsigned char *>(d_out);
	if (a.nwg > 0x7fffffffull) return rot_bad("more tiles than a launch grid holds");
	hipStream_t s = (hipStream_t)hip_stream;
	// (the unsigned identity is the row kernel too: it moves a 531 MB clip faster than the runtime's device copy, profiles/r15_rotate.txt)
	if (map[0] == 0) {
		switch (elem_bytes) {
		case 1: rows_launch<1>(a, s); break;
		case 2: rows_launch<2>(a, s); break;
		case 3: rows_launch<3>(a, s); break;
		default: rows_launch<4>(a, s); break;
		}
	} else {
		const dim3 g((unsigned)a.nwg), b(ROT_THREADS);
		switch (elem_bytes) {
		case 1: hipLaunchKernelGGL(rotate_tile_b_kernel, g, b, 0, s, a); break;
		case 2: hipLaunchKernelGGL(rotate_tile_e_kernel<2>, g, b, 0, s, a); break;
		case 3: hipLaunchKernelGGL(rotate_tile_e_kernel<3>, g, b, 0, s, a); break;
		default: hipLaunchKernelGGL(rotate_tile_e_kernel<4>, g, b, 0, s, a); break;
		}
	}
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) { rot_bad(hipGetErrorString(e)); return -4; }
	return 0;
}
