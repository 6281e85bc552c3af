/*
 * zoom_dev -- zoom's animation loop (zoom/zoom.c:320-410) device-resident over dspfft.h: the image's forward transform, then -n frames,
 * each at its own scale and position, on one dspfft_zoomanim object (no re-planning between frames), with --showsamples and the GBRPF32
 * frame store on the device.  The option arithmetic before the loop (zoom.c:268-303) is zoom_args.c's.
 *
 *   zoom_dev [-s <scale>] [-r WxH] [-p XxY] [-v WxH] [-c] [-P] [-%] [--basis interpolated|centered|native] [--showsamples[=point|grid]]
 *            [-n N] [-q] [--params FILE] [--video PATH] [--trc NAME] <input.ppm|.pf> <output.pf>
 *
 * -s takes a decimal or num/den, or XxY of those, as zoom does.  The per-frame expressions (-x, -y, -S, -X, -Y) need libavutil's evaluator
 * and are refused: --params FILE gives, per line d, the values x y S X Y those expressions would produce at frame d, "-" for one that was
 * not given (a column is all numbers or all "-"; nan and inf are numbers).  They are applied in zoom.c:321-345's order: S sets both scales
 * to (value, 1), X and Y then override one axis each, x and y set the position; the state persists across frames where a column is "-",
 * and a frame with a non-finite position or scale is skipped with the reference's message.  Without --params every frame is the first.
 * -g (linear RGB) asks ImageMagick for the file's colourspace, which a PF / P6 reader cannot answer, and is refused.  --trc NAME
 * (av_color_transfer_name's names: iec61966-2-1, bt709, gamma22, ...; include/dspfft.h lists what is built) does the work -g does once the
 * colourspace is known: the input's pixels are NAME-coded and are decoded on the device before the forward transform; every frame of
 * --video and the final image are encoded with NAME after the overlay (zoom.c:377-399).  Not built for the dense product.
 *
 * output.pf: the last frame, "PF\nVW VH\n-1.0\n" + VH x VW x 3 little-endian f32, top row first (host/rawio.h).
 * --video PATH: every frame as raw gbrpf32le, concatenated (ffmpeg -f rawvideo -pix_fmt gbrpf32le -s VWxVH -r 60 -i PATH; 60 is zoom's
 *   default rate); frames come down asynchronously into two pinned buffers, frame k - 1 written while frame k computes.
 * When the chirp-z plans do not cover the geometry (dspfft_zoomanim_create returns -2: an axis longer than the listed convolutions), every
 * frame is the dense product (dspfft_zoom_basis + dspfft_zoom_product) as in zoom_gpu; --showsamples is not built for that path.
 */
#include <getopt.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>
#include <dspfft.h>
#include "precision.h"
#include "rawio.h"
#include "zoom_args.h"

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int usage(const char *self)
{
	fprintf(stderr, "usage: %s [-s scale] [-r WxH] [-p XxY] [-v WxH] [-c] [-P] [-%%] [--basis interpolated|centered|native] "
	        "[--showsamples[=point|grid]] [-n N] [-q] [--params FILE] [--video PATH] [--trc NAME] <input> <output.pf>\n"
	        "  --trc NAME: the input is NAME-coded (iec61966-2-1, bt709, gamma22, ...): decoded before the transform, every frame encoded\n", self);
	return 2;
}

/* --params: nframes lines of five columns; present[c] = 0 for a column of "-" */
static int read_params(const char *path, size_t nframes, double **table, int present[5])
{
	FILE *f = fopen(path, "r");
	if (!f) { perror(path); return 1; }
	double *t = malloc(sizeof(double) * 5 * (nframes ? nframes : 1));
	char line[1024];
	size_t d = 0;
	while (d < nframes && fgets(line, sizeof line, f)) {
		char *s = line;
		for (int c = 0; c < 5; c++) {
			char tok[256];
			int used = 0;
			if (sscanf(s, "%255s%n", tok, &used) != 1) { fprintf(stderr, "%s:%zu: five columns expected\n", path, d + 1); fclose(f); return 1; }
			s += used;
			int num = strcmp(tok, "-") != 0;
			if (num) {
				char *end;
				t[d * 5 + c] = strtod(tok, &end);
				if (*end) { fprintf(stderr, "%s:%zu: not a number: %s\n", path, d + 1, tok); fclose(f); return 1; }
			} else t[d * 5 + c] = NAN;
			if (d == 0) present[c] = num;
			else if (present[c] != num) { fprintf(stderr, "%s:%zu: column %d mixes numbers and -\n", path, d + 1, c + 1); fclose(f); return 1; }
		}
		char rest[8];
		if (sscanf(s, "%7s", rest) == 1) { fprintf(stderr, "%s:%zu: more than five columns\n", path, d + 1); fclose(f); return 1; }
		d++;
	}
	fclose(f);
	if (d < nframes) { fprintf(stderr, "%s: %zu lines for %zu frames\n", path, d, nframes); return 1; }
	*table = t;
	return 0;
}

int main(int argc, char *argv[])
{
	long double vx = 0, vy = 0, xnum = 1, ynum = 1, lw = 0, lh = 0;
	unsigned long long xden = 1, yden = 1;
	size_t vw = 0, vh = 0, nframes = 1;
	int centered = 0, input_coords = 0, pct = 0, quiet = 0, showsamples = 0, basis = 0, trc = 0;
	const char *params = NULL, *video = NULL;
	const struct option opts[] = {{"showsamples", optional_argument, NULL, 1}, {"basis", required_argument, NULL, 2},
	                              {"params", required_argument, NULL, 3}, {"video", required_argument, NULL, 4}, {"trc", required_argument, NULL, 5}, {0}};
	int c;
	while ((c = getopt_long(argc, argv, "s:r:p:v:cP%n:qgx:y:S:X:Y:", opts, NULL)) != -1) {
		switch (c) {
		case 's': {                         /* num[/den], optionally followed by xnum[/den] for the vertical scale */
			int n = 0;
			if (sscanf(optarg, "%Lf%n/%llu%n", &xnum, &n, &xden, &n) <= 0) return usage(argv[0]);
			const char *rest = optarg + n;
			if (!*rest) { ynum = xnum; yden = xden; }
			else if (sscanf(rest, "x%Lf/%llu", &ynum, &yden) <= 0) return usage(argv[0]);
			break;
		}
		case 'r': sscanf(optarg, "%Lfx%Lf", &lw, &lh); break;
		case 'v': sscanf(optarg, "%zux%zu", &vw, &vh); break;
		case 'p': sscanf(optarg, "%Lfx%Lf", &vx, &vy); break;
		case 'c': centered = 1; break;
		case 'P': input_coords = 1; break;
		case '%': pct = 1; break;
		case 'n': nframes = strtoull(optarg, NULL, 10); break;
		case 'q': quiet = 1; break;
		case 'g':
			fprintf(stderr, "-g (linear RGB) is not supported: it needs ImageMagick's and libavutil's transfer functions"
			        " (when the file is known to be sRGB-coded: --trc iec61966-2-1)\n");
			return 2;
		case 'x': case 'y': case 'S': case 'X': case 'Y':
			fprintf(stderr, "-%c: expressions are not evaluated here; give their per-frame values with --params FILE\n", c); return 2;
		case 1:
			showsamples = 1;
			if (optarg && !strcmp(optarg, "grid")) showsamples = 2;
			else if (optarg && strcmp(optarg, "point")) return usage(argv[0]);
			break;
		case 2:
			if (!strcmp(optarg, "centered")) basis = 1;
			else if (!strcmp(optarg, "native")) basis = 2;
			else if (strcmp(optarg, "interpolated")) return usage(argv[0]);
			break;
		case 3: params = optarg; break;
		case 4: video = optarg; break;
		case 5:
			trc = dspfft_trc_from_name(optarg);
			if (trc < 0) { fprintf(stderr, "--trc %s: unknown transfer characteristic, or not built\n", optarg); return 2; }
			break;
		default: return usage(argv[0]);
		}
	}
	if (argc - optind < 2) return usage(argv[0]);
	quiet |= nframes == 1;
	const char *input = argv[optind], *output = argv[optind + 1];

	size_t width, height;
	float *pix;
	if (read_image(input, &width, &height, &pix)) { fprintf(stderr, "cannot read %s\n", input); return 1; }
	zoom_viewport(width, height, lw, lh, &xnum, &xden, &ynum, &yden, &vw, &vh, &vx, &vy, pct, input_coords, centered);
	if (!vw || !vh) { fprintf(stderr, "empty view %zux%zu\n", vw, vh); return 1; }
	double *table = NULL;
	int present[5] = {0, 0, 0, 0, 0};
	if (params && read_params(params, nframes, &table, present)) return 1;

	/* zoom.c:263-265 on the device: REDFT10 x REDFT10 of the interleaved image, unnormalised */
	const size_t n3 = width * height * 3, npix = vw * vh;
	float *d_coeffs = NULL, *d_frame = NULL, *d_work = NULL;
	HIP(hipMalloc((void **)&d_coeffs, sizeof(float) * n3));
	HIP(hipMalloc((void **)&d_frame, sizeof(float) * npix * 3));
	HIP(hipMemcpy(d_coeffs, pix, sizeof(float) * n3, hipMemcpyHostToDevice));
	if (trc && dspfft_trc_apply_f32(d_coeffs, d_coeffs, n3, trc, 1, NULL)) { fprintf(stderr, "--trc: %s\n", dspfft_last_error()); return 1; }   /* to linear light */
	dspfft_plan fwd;
	if (dspfft_plan_many_r2r(&fwd, 2, (int[]){(int)height, (int)width}, 3, NULL, 3, 1, NULL, 3, 1, (int[]){DSPFFT_REDFT10, DSPFFT_REDFT10}) ||
	    dspfft_execute(fwd, d_coeffs, d_coeffs, NULL)) { fprintf(stderr, "forward transform: %s\n", dspfft_last_error()); return 1; }

	dspfft_zoomanim z = NULL;
	const int rc = dspfft_zoomanim_create(&z, (int)width, (int)height, basis, (int)vw, (int)vh);
	float *xb = NULL, *yb = NULL;
	if (rc == 0) {
		HIP(hipMalloc((void **)&d_work, sizeof(float) * dspfft_zoomanim_work_floats(z)));
		if (dspfft_zoomanim_set_coeffs(z, d_coeffs, NULL) || dspfft_zoomanim_set_trc(z, trc)) { fprintf(stderr, "zoomanim: %s\n", dspfft_zoomanim_last_error()); return 1; }
	} else if (rc == -2) {
		if (trc) { fprintf(stderr, "--trc: not built for the dense product (%s)\n", dspfft_zoomanim_last_error()); return 1; }
		if (showsamples) { fprintf(stderr, "--showsamples: not built for the dense product (%s)\n", dspfft_zoomanim_last_error()); return 1; }
		HIP(hipMalloc((void **)&xb, sizeof(float) * vw * width));
		HIP(hipMalloc((void **)&yb, sizeof(float) * vh * height));
		HIP(hipMalloc((void **)&d_work, sizeof(float) * dspfft_zoom_work_floats((int)width, (int)height, height, (int)vw)));
		fprintf(stderr, "%zux%zu -> %zux%zu: beyond the chirp-z lengths, dense product per frame\n", width, height, vw, vh);
	} else { fprintf(stderr, "zoomanim: %s\n", dspfft_zoomanim_last_error()); return 1; }

	FILE *vf = NULL;
	float *h_frame[2] = {NULL, NULL}, *last = malloc(sizeof(float) * npix * 3);
	hipEvent_t ev[2];
	if (video) {
		if (!(vf = fopen(video, "wb"))) { fprintf(stderr, "cannot write %s\n", video); return 1; }
		for (int k = 0; k < 2; k++) { HIP(hipHostMalloc((void **)&h_frame[k], sizeof(float) * npix * 3, 0)); HIP(hipEventCreate(&ev[k])); }
		fprintf(stderr, "video: up to %zu frames of gbrpf32le %zux%zu (ffmpeg -f rawvideo -pix_fmt gbrpf32le -s %zux%zu -r 60 -i %s)\n",
		        nframes, vw, vh, vw, vh, video);
	}
	size_t kept = 0;
	for (size_t d = 0; d < nframes; d++) {
		if (table) {                                                              /* zoom.c:321-340 */
			const double *v = table + d * 5;
			if (present[2]) { xnum = ynum = v[2]; xden = yden = 1; }
			if (present[3]) { xnum = v[3]; xden = 1; }
			if (present[4]) { ynum = v[4]; yden = 1; }
			if (present[0]) vx = v[0];
			if (present[1]) vy = v[1];
		}
		if (!(isfinite(vx) && isfinite(vy) && isfinite(xnum / xden) && isfinite(ynum / yden))) {          /* zoom.c:342-345 */
			fprintf(stderr, "Skipping non-finite expression result at frame %zu\n", d);
			continue;
		}
		const double xn = (double)xnum, xd = (double)xden, yn = (double)ynum, yd = (double)yden, fx = (double)vx, fy = (double)vy;
		const int planar = vf != NULL;             /* the video's GBRPF32 frame; the interleaved one otherwise (the output file's) */
		if (z) {
			if (dspfft_zoomanim_execute(z, xn, xd, yn, yd, fx, fy, showsamples, planar, d_frame, d_work, NULL)) {
				fprintf(stderr, "frame %zu: %s\n", d, dspfft_zoomanim_last_error()); return 1;
			}
		} else {
			const size_t cw = dspfft_zoom_ncomponents(xn, xd, width), ch = dspfft_zoom_ncomponents(yn, yd, height);
			if (dspfft_zoom_basis(xb, basis, xn, xd, fx, vw, width, NULL) || dspfft_zoom_basis(yb, basis, yn, yd, fy, vh, height, NULL) ||
			    dspfft_zoom_product(d_coeffs, (int)width, (int)height, xb, cw, yb, ch, d_frame, (int)vw, (int)vh, d_work, NULL)) {
				fprintf(stderr, "frame %zu: %s\n", d, dspfft_zoom_last_error()); return 1;
			}
		}
		const size_t k = kept & 1;
		if (vf) {
			HIP(hipMemcpyAsync(h_frame[k], d_frame, sizeof(float) * npix * 3, hipMemcpyDeviceToHost, NULL));
			HIP(hipEventRecord(ev[k], NULL));
			if (kept) {                                       /* the previous frame is written while this one copies */
				HIP(hipEventSynchronize(ev[k ^ 1]));
				if (fwrite(h_frame[k ^ 1], sizeof(float), npix * 3, vf) != npix * 3) { fprintf(stderr, "error writing %s\n", video); return 1; }
			}
		}
		kept++;
		if (!quiet) fprintf(stderr, "\r%zu/%zu         ", d, nframes);
		if (!z && vf) {                                       /* the dense product is interleaved: the planes on the host */
			HIP(hipEventSynchronize(ev[k]));
			memcpy(last, h_frame[k], sizeof(float) * npix * 3);
			for (size_t i = 0; i < npix; i++)
				for (int ch = 0; ch < 3; ch++) h_frame[k][(ch == 0 ? 2 : ch - 1) * npix + i] = last[i * 3 + ch];
		}
	}
	if (!quiet) fprintf(stderr, "\r%zu/%zu         \n", nframes, nframes);
	if (!kept) { fprintf(stderr, "no frame rendered\n"); return 1; }
	/* the last frame, interleaved, for output.pf */
	if (vf) {
		const size_t k = (kept - 1) & 1;
		HIP(hipEventSynchronize(ev[k]));
		if (fwrite(h_frame[k], sizeof(float), npix * 3, vf) != npix * 3 || fclose(vf)) { fprintf(stderr, "error writing %s\n", video); return 1; }
		for (size_t i = 0; i < npix; i++)
			for (int ch = 0; ch < 3; ch++) last[i * 3 + ch] = h_frame[k][(ch == 0 ? 2 : ch - 1) * npix + i];
		for (int j = 0; j < 2; j++) { HIP(hipHostFree(h_frame[j])); HIP(hipEventDestroy(ev[j])); }
	} else HIP(hipMemcpy(last, d_frame, sizeof(float) * npix * 3, hipMemcpyDeviceToHost));
	FILE *f = fopen(output, "wb");
	if (!f) { perror(output); return 1; }
	fprintf(f, "PF\n%zu %zu\n-1.0\n", vw, vh);
	if (fwrite(last, sizeof(float), npix * 3, f) != npix * 3 || fclose(f)) { perror(output); return 1; }
	fprintf(stderr, "%zu of %zu frames, %zux%zu view, last at scale %g x %g, position (%g, %g), %s\n", kept, nframes, vw, vh,
	        (double)(xnum / xden), (double)(ynum / yden), (double)vx, (double)vy, z ? "chirp-z" : "dense product");
	if (z) dspfft_zoomanim_destroy(z);
	dspfft_destroy_plan(fwd);
	HIP(hipFree(d_coeffs)); HIP(hipFree(d_frame)); HIP(hipFree(d_work));
	if (xb) { HIP(hipFree(xb)); HIP(hipFree(yb)); }
	free(pix); free(last); free(table);
	return 0;
}
