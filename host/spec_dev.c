/*
 * spec_dev -- spec and ispec (spec/spec.c, spec/ispec.c) on 8-bit RGB images with the whole path on the device: one
 * dspfft_execute_spec_u8 / dspfft_execute_ispec_u8 call from the pixels of the input to the pixels of the output (include/dspfft.h).
 *
 *   spec_dev spec  [options] in.ppm spectrogram.ppm     also writes spectrogram.ppm.dc: the header's DC values, one double per line
 *   spec_dev ispec [options] spectrogram.ppm out.ppm    reads spectrogram.ppm.dc where it exists
 * options: -t abs|shift|flat|sign|copy (spec.h:71-76; default abs)   -R one|dc|dcs   -T log|linear   -S abs|shift|saturate|retain
 *          -G native|reference|<gain>   -m signmap.ppm  (spec: write the `sign` image beside an abs spectrogram; ispec: read it, ispec.c:87-98)
 *          -p  (ispec: restore the DC values, ispec.c:161-163)
 * Images are P6 PPM with maxval 255.  The reference reads and writes through MagickWand and keeps DC in an image property; the
 * sidecar file stands in for that property.
 */
#include <getopt.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>
#include <dspfft.h>

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define DSP(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, dspfft_last_error()); return 1; } } while (0)

static int read_ppm(const char *path, int *w, int *h, uint8_t **pix)
{
	FILE *f = fopen(path, "rb");
	if (!f) return 1;
	int maxval = 0;
	if (fscanf(f, "P6 %d %d %d", w, h, &maxval) != 3 || maxval != 255 || *w < 1 || *h < 1 || fgetc(f) == EOF) { fclose(f); return 1; }
	const size_t n = (size_t)*w * *h * 3;
	*pix = malloc(n);
	const int ok = *pix && fread(*pix, 1, n, f) == n;
	fclose(f);
	return !ok;
}
static int write_ppm(const char *path, int w, int h, const uint8_t *pix)
{
	FILE *f = fopen(path, "wb");
	if (!f) return 1;
	fprintf(f, "P6\n%d %d\n255\n", w, h);
	const size_t n = (size_t)w * h * 3;
	const int ok = fwrite(pix, 1, n, f) == n;
	return fclose(f) || !ok;
}
static int pick(const char *arg, const char *const *names, int n)
{
	for (int i = 0; i < n; i++) if (!strcmp(arg, names[i])) return i;
	return -1;
}

int main(int argc, char *argv[])
{
	static const char *const RANGES[] = {"one", "dc", "dcs"}, *const SCALES[] = {"log", "linear"}, *const SIGNS[] = {"abs", "shift", "saturate", "retain"};
	static const char *const PRESETS[] = {"abs", "shift", "flat", "sign", "copy"};
	/* spec.h:71-76: scale, sign, gain (0 native, 2 custom), range */
	static const int PRESET[5][4] = {{0, 0, 0, 1}, {0, 1, 0, 0}, {1, 1, 2, 0}, {1, 2, 2, 0}, {1, 3, 2, 0}};
	if (argc < 2 || (strcmp(argv[1], "spec") && strcmp(argv[1], "ispec"))) {
		fprintf(stderr, "usage: %s spec|ispec [-t template] [-R range] [-T scale] [-S sign] [-G gain] [-m signmap.ppm] [-p] <in.ppm> <out.ppm>\n", argv[0]);
		return 2;
	}
	const int inverse = !strcmp(argv[1], "ispec");
	int scale = 0, sign = 0, gaintype = 0, range = 1, restore = 0, o;
	double custom = 1.0;
	const char *mapname = NULL;
	optind = 2;
	while ((o = getopt(argc, argv, "t:R:T:S:G:m:p")) != -1) {
		int v;
		switch (o) {
		case 't': if ((v = pick(optarg, PRESETS, 5)) < 0) { fprintf(stderr, "invalid template '%s'\n", optarg); return 2; }
			scale = PRESET[v][0]; sign = PRESET[v][1]; gaintype = PRESET[v][2]; range = PRESET[v][3]; break;
		case 'R': if ((range = pick(optarg, RANGES, 3)) < 0) { fprintf(stderr, "invalid range '%s'\n", optarg); return 2; } break;
		case 'T': if ((scale = pick(optarg, SCALES, 2)) < 0) { fprintf(stderr, "invalid scale '%s'\n", optarg); return 2; } break;
		case 'S': if ((sign = pick(optarg, SIGNS, 4)) < 0) { fprintf(stderr, "invalid sign '%s'\n", optarg); return 2; } break;
		case 'G':
			if (!strcmp(optarg, "native")) gaintype = 0;
			else if (!strcmp(optarg, "reference")) gaintype = 1;
			else { char *end; custom = strtod(optarg, &end); gaintype = 2; if (end == optarg) { fprintf(stderr, "invalid gain '%s'\n", optarg); return 2; } }
			break;
		case 'm': mapname = optarg; break;
		case 'p': restore = 1; break;
		default: return 2;
		}
	}
	if (argc - optind != 2) { fprintf(stderr, "need an input and an output image\n"); return 2; }
	const char *inname = argv[optind], *outname = argv[optind + 1];

	int w, h, mw, mh;
	uint8_t *pix = NULL, *map = NULL;
	if (read_ppm(inname, &w, &h, &pix)) { fprintf(stderr, "cannot read %s (P6, maxval 255)\n", inname); return 1; }
	const int d = 3;
	const size_t n = (size_t)w * h * d;
	const dspfft_spec_image_params sp = {gaintype == 0 ? 127.5 * sqrt((double)w * h * 4) : gaintype == 1 ? 127.5 * 1024 : custom, range, scale, sign};   /* ispec.c:112-117 */

	uint8_t *d_in, *d_out, *d_map = NULL;
	float *d_work;
	double *d_dc;
	HIP(hipMalloc((void **)&d_in, n)); HIP(hipMalloc((void **)&d_out, n)); HIP(hipMalloc((void **)&d_work, n * sizeof(float))); HIP(hipMalloc((void **)&d_dc, d * sizeof(double)));
	if (mapname) HIP(hipMalloc((void **)&d_map, n));
	HIP(hipMemcpy(d_in, pix, n, hipMemcpyHostToDevice));

	const int hw[2] = {h, w}, kinds[2] = {inverse ? DSPFFT_REDFT01 : DSPFFT_REDFT10, inverse ? DSPFFT_REDFT01 : DSPFFT_REDFT10};
	const float r2 = (float)sqrt(2.0);
	dspfft_plan plan;
	DSP(dspfft_plan_many_r2r_ordered(&plan, 2, hw, d, NULL, d, 1, NULL, d, 1, kinds, inverse));
	/* spec.c:70-78 on (float)byte; ispec.c:153-159 */
	DSP(dspfft_plan_set_scale(plan, inverse ? 0.5f : (float)(1.0 / (255.0 * 2.0 * w * h))));
	for (int a = 0; a < 2; a++) DSP(dspfft_plan_set_axis_scale0(plan, a, inverse ? r2 : 1.f, inverse ? 1.f : 1.f / r2));

	char dcname[4096];
	double dc[3] = {0, 0, 0};
	if (!inverse) {
		DSP(dspfft_execute_spec_u8(plan, d_in, d_out, d_map, d_work, d_dc, &sp, NULL));
		HIP(hipMemcpy(dc, d_dc, sizeof dc, hipMemcpyDeviceToHost));
		snprintf(dcname, sizeof dcname, "%s.dc", outname);
		FILE *f = fopen(dcname, "w");
		if (!f) { fprintf(stderr, "cannot write %s\n", dcname); return 1; }
		for (int z = 0; z < d; z++) fprintf(f, "%.17g\n", dc[z]);
		fclose(f);
	} else {
		int have_dc = 0;
		snprintf(dcname, sizeof dcname, "%s.dc", inname);
		FILE *f = fopen(dcname, "r");
		if (f) { have_dc = fscanf(f, "%lf %lf %lf", &dc[0], &dc[1], &dc[2]) == 3; fclose(f); }
		if (mapname) {
			if (read_ppm(mapname, &mw, &mh, &map) || mw != w || mh != h) { fprintf(stderr, "cannot read %s as a %d x %d sign map\n", mapname, w, h); return 1; }
			for (int z = 0; z < d; z++) dc[z] = map[z] / 255.;                                /* ispec.c:92-93 */
			have_dc = 1;
			HIP(hipMemcpy(d_map, map, n, hipMemcpyHostToDevice));
		}
		if (!have_dc && (restore || range != 0)) { fprintf(stderr, "DC not found (%s)\n", dcname); return 1; }      /* ispec.c:73-77 */
		DSP(dspfft_execute_ispec_u8(plan, d_in, d_map, d_out, d_work, have_dc ? dc : NULL, restore, &sp, NULL));
	}
	HIP(hipDeviceSynchronize());
	HIP(hipMemcpy(pix, d_out, n, hipMemcpyDeviceToHost));
	if (write_ppm(outname, w, h, pix)) { fprintf(stderr, "cannot write %s\n", outname); return 1; }
	if (!inverse && mapname) {
		HIP(hipMemcpy(pix, d_map, n, hipMemcpyDeviceToHost));
		if (write_ppm(mapname, w, h, pix)) { fprintf(stderr, "cannot write %s\n", mapname); return 1; }
	}
	dspfft_destroy_plan(plan);
	HIP(hipFree(d_in)); HIP(hipFree(d_out)); HIP(hipFree(d_work)); HIP(hipFree(d_dc));
	if (d_map) HIP(hipFree(d_map));
	free(pix); free(map);
	return 0;
}
