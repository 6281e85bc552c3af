// TEST-ONLY: dspfun_amd/csrc/trc_core.h over arrays, built with g++ -ffp-contract=off by tests/trc_ref.py.  trcr_pow is libm's pow element
// by element: the numpy statement of the table (tests/trc_ref.py) takes its powers from it, because numpy's own float64 power may come
// from a vector library that differs from libm in the last place.
#include <math.h>
#include <stddef.h>

#include "trc_core.h"

using namespace dspfft;

extern "C" void trcr_exact(int id, int inverse, const double *x, double *y, size_t n)
{
	for (size_t i = 0; i < n; i++) y[i] = trc_exact(id, inverse, x[i]);
}
extern "C" void trcr_eval_f32(int id, int inverse, const float *x, float *y, size_t n)
{
	for (size_t i = 0; i < n; i++) y[i] = trc_eval_f32(id, inverse, x[i]);
}
extern "C" void trcr_pow(const double *x, double e, double *y, size_t n)
{
	for (size_t i = 0; i < n; i++) y[i] = pow(x[i], e);
}
extern "C" void trcr_pow_lean(const double *x, double e, double *y, size_t n)
{
	for (size_t i = 0; i < n; i++) y[i] = trc_pow_lean(x[i], e);
}
extern "C" int trcr_from_name(const char *name) { return trc_from_name(name); }
extern "C" const char *trcr_name(int id) { return trc_name(id); }
