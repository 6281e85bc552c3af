// TEST-ONLY: dspfun_amd/csrc/trc_u8_core.h over arrays, built with g++ -ffp-contract=off by tests/trc_u8_ref.py.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "trc_u8_core.h"

using namespace dspfft;

extern "C" void trcu8_decode_lut(float *lut, int trc) { trc_u8_decode_lut(lut, trc); }
extern "C" void trcu8_thresholds(double *thr, int trc) { trc_u8_thresholds(thr, trc); }
// mode 0: trc_u8_byte (binary search); 1: trc_u8_byte_from a seed of trc_u8_seed; 2: from the worst seeds, 0 and 255 in turn
extern "C" void trcu8_bytes(const double *thr, int trc, int mode, const double *pel, uint8_t *out, size_t n)
{
	const TrcParams p = trc_params(trc);
	for (size_t i = 0; i < n; i++)
		out[i] = (uint8_t)(mode == 0 ? trc_u8_byte(thr, pel[i]) : trc_u8_byte_from(thr, pel[i], mode == 1 ? trc_u8_seed(p, pel[i]) : (i & 1) ? 255u : 0u));
}
extern "C" void trcu8_seeds(int trc, const double *pel, uint8_t *out, size_t n)
{
	const TrcParams p = trc_params(trc);
	for (size_t i = 0; i < n; i++) out[i] = (uint8_t)trc_u8_seed(p, pel[i]);
}
// quantise_u8(trc_exact(encode, pel / 255) * 255): motion.c:769,776 in double
extern "C" void trcu8_exact(int trc, const double *pel, uint8_t *out, size_t n)
{
	const TrcParams p = trc_params(trc);
	for (size_t i = 0; i < n; i++) out[i] = trc_u8_encode_exact(p, pel[i]);
}
// the store's pel in the reference's order, in double (motion.c:759,767)
extern "C" void trcu8_store_pel(const float *c, double scalefactor, double norm, double *pel, size_t n)
{
	for (size_t i = 0; i < n; i++) {
		double v = (double)c[i] * scalefactor * norm;
		v *= norm;
		pel[i] = v;
	}
}
