/* TEST-ONLY: the stand-in for scan's inverse transform (scan/scan.c:360,447: an FFTW REDFT01 in both dimensions, unnormalised) that the
 * frame fixtures are generated with and the CPU restatement is fed: a direct DCT-III in float, rows then columns, cosines rounded from
 * double.  Deterministic and the same in the fixture generator's gcc build and the restatement's g++ build (both -ffp-contract=off).
 * out[y][x][z] = sum_{v,u} k(v) k(u) in[v][u][z] cos(pi v (2y+1) / 2h) cos(pi u (2x+1) / 2w), k(0) = 1, k(>0) = 2. */
#ifndef SCAN_FRAMES_STUB_H
#define SCAN_FRAMES_STUB_H
#include <math.h>
#include <stdlib.h>
#include <stddef.h>

static float *sf_stub_table(size_t n)
{
	float *t = (float *)malloc(sizeof(float) * n * n);
	for (size_t k = 0; k < n; k++)
		for (size_t u = 0; u < n; u++)
			t[k * n + u] = (float)((u ? 2.0 : 1.0) * cos(3.14159265358979323846 * (double)u * (double)(2 * k + 1) / (double)(2 * n)));
	return t;
}

static void sf_stub_redft01_2d(const float *in, float *out, size_t w, size_t h, size_t ch)
{
	float *tw = sf_stub_table(w), *th = sf_stub_table(h), *rows = (float *)malloc(sizeof(float) * w * h * ch);
	for (size_t y = 0; y < h; y++)
		for (size_t x = 0; x < w; x++)
			for (size_t z = 0; z < ch; z++) {
				float acc = 0;
				for (size_t u = 0; u < w; u++) acc += in[(y * w + u) * ch + z] * tw[x * w + u];
				rows[(y * w + x) * ch + z] = acc;
			}
	for (size_t y = 0; y < h; y++)
		for (size_t x = 0; x < w; x++)
			for (size_t z = 0; z < ch; z++) {
				float acc = 0;
				for (size_t v = 0; v < h; v++) acc += rows[(v * w + x) * ch + z] * th[y * h + v];
				out[(y * w + x) * ch + z] = acc;
			}
	free(tw); free(th); free(rows);
}
#endif
