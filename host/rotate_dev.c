/*
 * rotate_dev -- rotate (motion/rotate.c) on a raw clip with the arithmetic on the device: upload, ONE dspfft_rotate call, download.
 *
 *   rotate_dev [-s start:nframes] [-c components] <spec> W H FRAMES in.raw out.raw
 *
 * in.raw holds FRAMES frames of H rows of W pixels of `components` bytes (default 1; at most 4).  <spec> is rotate's own argument
 * ("zyx", "-yx+z", ...: rotate.c:74-89); one that begins with '-' goes after "--", as with the reference's getopt.  -s is the reference's seek and frame count (rotate.c:107-120) as a pointer offset into the
 * uploaded clip and a smaller frame count.  The output's dimensions go to stderr as "W H FRAMES".
 */
#include <getopt.h>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>
#include <dspfft.h>

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char *argv[])
{
	uint64_t start = 0, nframes = 0;
	int components = 1, o;
	while ((o = getopt(argc, argv, "s:c:")) != -1) {
		switch (o) {
		case 's': if (sscanf(optarg, "%" SCNu64 ":%" SCNu64, &start, &nframes) < 1) { fprintf(stderr, "invalid -s '%s'\n", optarg); return 2; } break;
		case 'c': components = atoi(optarg); break;
		default: return 2;
		}
	}
	if (argc - optind != 6) {
		fprintf(stderr, "usage: %s [-s start:nframes] [-c components] [--] [-]xyz W H FRAMES in.raw out.raw\n", argv[0]);
		return 2;
	}
	int map[3], invert[3];
	if (dspfft_rotate_parse(argv[optind], map, invert)) { fprintf(stderr, "'%s' is no arrangement of the axes x, y, z\n", argv[optind]); return 2; }
	uint64_t len[3];
	for (int i = 0; i < 3; i++) len[i] = strtoull(argv[optind + 1 + i], NULL, 10);
	if (!len[0] || !len[1] || !len[2] || components < 1 || components > 4) { fprintf(stderr, "W, H, FRAMES >= 1 and 1..4 components\n"); return 2; }
	const char *inname = argv[optind + 4], *outname = argv[optind + 5];
	const uint64_t total = len[2], frame = len[0] * len[1] * (uint64_t)components;
	/* rotate.c:113-120 */
	if (start >= total) { fprintf(stderr, "-s starts beyond the clip\n"); return 2; }
	len[2] = total - start;
	if (nframes && nframes < len[2]) len[2] = nframes;
	const uint64_t nin = total * frame, nout = len[2] * frame;

	uint8_t *pix = malloc(nin);
	FILE *f = fopen(inname, "rb");
	if (!pix || !f || fread(pix, 1, nin, f) != nin) { fprintf(stderr, "cannot read %" PRIu64 " bytes from %s\n", nin, inname); return 1; }
	fclose(f);

	uint8_t *d_in, *d_out;
	HIP(hipMalloc((void **)&d_in, nin));
	HIP(hipMalloc((void **)&d_out, nout));
	HIP(hipMemcpy(d_in, pix, nin, hipMemcpyHostToDevice));
	if (dspfft_rotate(d_out, d_in + start * frame, len, components, map, invert, NULL)) { fprintf(stderr, "dspfft_rotate: %s\n", dspfft_motion_last_error()); return 1; }
	HIP(hipDeviceSynchronize());
	HIP(hipMemcpy(pix, d_out, nout, hipMemcpyDeviceToHost));
	f = fopen(outname, "wb");
	if (!f || fwrite(pix, 1, nout, f) != nout || fclose(f)) { fprintf(stderr, "cannot write %s\n", outname); return 1; }
	fprintf(stderr, "%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", len[map[0]], len[map[1]], len[map[2]]);
	HIP(hipFree(d_in)); HIP(hipFree(d_out));
	free(pix);
	return 0;
}
