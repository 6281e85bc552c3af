/*
 * scan_dev -- scan's main loop (scan/scan.c:289-298 forward + normalisation, :377-383 DC broadcast, :421-459 per-frame
 * scatter / inverse / accumulate) with EVERY buffer resident on the GPU and every scan method generated there
 * (include/dspfft.h "the other scan methods on the device"): one fused masked-accumulate execution per output frame, no
 * PCIe traffic inside the loop.  The host-pointer drop-in of the same loop is host/scan_gpu.c.
 *
 *   scan_dev in.{ppm,pf} out.pf [step] [method] [--offset N] [--skip] [--invert] [--frames N]     (options anywhere)
 *     method: a prefix of horizontal vertical zigzag row column diagonal mirror box ibox radial iradial (scan_methods.c:581-591),
 *             magnitude[:qfactor] (scan_methods.c:240-296), file:<path> (scan_methods.c:393-410, either serialisation), or
 *             random[:seed] (scan_methods.c:210-228: the permutation is drawn on the host with libc rand(), as the tool draws it).
 *             evalxy / evali (scan_methods.c:186-201,333-391) need libavutil's expression evaluator and are not mirrored: write the order
 *             they would give to a file and pass file:<path>.
 *   --offset N / -O N, --skip, --invert / -I, --frames N / -n N: scan.c:55-59,176-205,346-459, arithmetic and quirks included:
 *     nframes = 0 or > limit/step becomes ceil(limit/step) (:347-348; limit/step with a remainder drops the last partial frame);
 *     offset >= limit becomes limit - 1 (:385-386); unless --skip, ONE inverse adds the scan indices [0, offset) first (the fill,
 *     :389-417; inverted: [limit - offset, limit)); the loop then runs FRAMES offset .. offset + nframes - 1 (:421), i.e. from scan index
 *     offset * step, so with step > 1 the indices [offset, offset * step) are never added -- the reference's behaviour, kept; frames past
 *     limit add nothing; --invert walks the scan backwards, index j = limit - 1 - s (:391,424).
 *   The fill and every inverted frame are one dspfft_execute_masked_accumulate_range over the owner index (DC unmarked: the reference
 *   clears it before every inverse, :406,445); box, and files whose indices share pixels, stamp those indices instead (the fill in
 *   chunks of `step` indices under one reserved id, then one step on that id).
 *   -v / --visualize, -s / --spectrogram, --spec-gain G, --spec-opts k=v:..., -i / --intermediates, -M / --max-intermediates,
 *   -P / --measure-parity (scan.c:41-76,176-215, -s implies -v, -M implies -i): the output frames of scan.c:366-536 composed on the device
 *     (include/dspfft.h "scan's output frames"); a frame for EVERY i in [offset, offset + nframes), past the limit included.  -P prints
 *     the reference's message (depth 8 for P6 input, 32 for PF).  -g / --linear is refused (needs a colourspace transform).
 *   --trc NAME (av_color_transfer_name's names: iec61966-2-1, bt709, gamma22, ...; include/dspfft.h lists what is built): the work -g does
 *     once the colourspace is known.  The input's pixels are NAME-coded: they are decoded on the device before the forward transform (and
 *     before -P's copy of the original, scan.c:268-287), every frame's left-hand panels are encoded with NAME (scan.c:412-414,455-457,
 *     486-488), and so is the final image.
 *   --video PATH: every frame as raw gbrpf32le, concatenated (ffmpeg -f rawvideo -pix_fmt gbrpf32le -s W'xH' -r 20 -i PATH); the
 *     geometry goes to stderr.  Frames come down asynchronously into two pinned buffers: frame k - 1 is written while frame k computes
 *     and copies.
 * Output: the final `sum` image; on stderr the number of frames and max|sum - input| (0 up to rounding when the method visits
 * every pixel exactly once and the whole scan is run).  Without the frame options the output is what it was before they existed.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <dspfft.h>
#include <hip/hip_runtime_api.h>
#include "precision.h"
#include "rawio.h"
#include "scan_orders.h"

#define HIP(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 1; } } while (0)
#define DSP(x) do { if (x) { fprintf(stderr, "dspfft: %s (%s:%d)\n", dspfft_last_error(), __FILE__, __LINE__); return 1; } } while (0)

#define FILL_ID 0xFFFFFFFEu

/* speclib.c:42-77 spec_params_parse over k=v pairs separated by ':' (scale=, sign=, preset= or a preset's name as a key); returns the
 * pair that failed to parse, or NULL */
static const char *parse_spec_opts(const char *opts, int *scale, int *sign)
{
	static const char *scales[] = {"linear", "log"}, *signs[] = {"abs", "shift", "saturate"};
	static const struct { const char *name; int scale, sign; } presets[] = {{"abs", 2, 1}, {"shift", 2, 2}, {"flat", 1, 2}, {"signmap", 1, 3}};
	const char *p = opts;
	while (*p) {
		const char *end = strchr(p, ':');
		size_t len = end ? (size_t)(end - p) : strlen(p);
		char kv[64];
		if (len >= sizeof kv) return p;
		memcpy(kv, p, len); kv[len] = 0;
		if (len) {
			char *val = strchr(kv, '=');
			if (val) *val++ = 0; else val = kv + len;
			int ok = 0;
			if (!strcmp(kv, "scale")) { for (int i = 0; i < 2; i++) if (!strcmp(val, scales[i])) { *scale = i + 1; ok = 1; } }
			else if (!strcmp(kv, "sign")) { for (int i = 0; i < 3; i++) if (!strcmp(val, signs[i])) { *sign = i + 1; ok = 1; } }
			else {
				const char *key = strcmp(kv, "preset") ? kv : val;
				for (int i = 0; i < 4; i++) if (!strcmp(key, presets[i].name)) { *scale = presets[i].scale; *sign = presets[i].sign; ok = 1; }
			}
			if (!ok) return p;
		}
		p += len + (end != NULL);
	}
	return NULL;
}           /* the id the fill's pixels are stamped with (frame ids stay below limit + nframes) */

int main(int argc, char *argv[])
{
	/* positional arguments in their order, the options anywhere */
	const char *pos[4] = {NULL, NULL, NULL, NULL};
	int npos = 0, skip = 0, invert = 0;
	size_t offset = 0, nframes = 0;
	dspfft_scan_frame_opts fo;
	memset(&fo, 0, sizeof fo);
	int parity = 0, trc = 0;
	const char *video = NULL;
	for (int a = 1; a < argc; a++) {
		const char *s = argv[a];
		if (!strcmp(s, "-v") || !strcmp(s, "--visualize")) fo.visualize = 1;
		else if (!strcmp(s, "-s") || !strcmp(s, "--spectrogram")) fo.spectrogram = fo.visualize = 1;
		else if (!strcmp(s, "-i") || !strcmp(s, "--intermediates")) fo.intermediates = 1;
		else if (!strcmp(s, "-M") || !strcmp(s, "--max-intermediates")) fo.intermediates = fo.max_intermediates = 1;
		else if (!strcmp(s, "-P") || !strcmp(s, "--measure-parity")) parity = 1;
		else if (!strcmp(s, "-g") || !strcmp(s, "--linear")) {
			fprintf(stderr, "--linear is not supported: it needs ImageMagick's colourspace transform and libavutil's transfer function"
			        " (when the file is known to be sRGB-coded: --trc iec61966-2-1)\n");
			return 2;
		} else if (!strcmp(s, "--trc") && a + 1 < argc) {
			trc = dspfft_trc_from_name(argv[++a]);
			if (trc < 0) { fprintf(stderr, "--trc %s: unknown transfer characteristic, or not built\n", argv[a]); return 2; }
		} else if (!strcmp(s, "--spec-gain") && a + 1 < argc) fo.spec_gain = strtod(argv[++a], NULL);        /* precision_strtoi, INTERMEDIATE=D */
		else if (!strcmp(s, "--spec-opts") && a + 1 < argc) {
			const char *e = parse_spec_opts(argv[++a], &fo.spec_scaletype, &fo.spec_signtype);
			if (e) { fprintf(stderr, "Couldn't parse spec option starting at: %s\n", e); return 2; }
		} else if (!strcmp(s, "--video") && a + 1 < argc) video = argv[++a];
		else if ((!strcmp(s, "--offset") || !strcmp(s, "-O") || !strcmp(s, "--frames") || !strcmp(s, "-n")) && a + 1 < argc) {
			const size_t v = strtoul(argv[++a], NULL, 10);
			if (s[1] == 'O' || s[2] == 'o') offset = v; else nframes = v;
		} else if (!strcmp(s, "--skip")) skip = 1;
		else if (!strcmp(s, "--invert") || !strcmp(s, "-I")) invert = 1;
		else if (s[0] == '-' && s[1]) { fprintf(stderr, "unknown option %s\n", s); return 2; }
		else if (npos < 4) pos[npos++] = s;
		else { fprintf(stderr, "too many arguments\n"); return 2; }
	}
	if (npos < 2) {
		fprintf(stderr, "usage: %s <in> <out.pf> [step] [method] [--offset N] [--skip] [--invert] [--frames N] [-v] [-s] [--spec-gain G] "
		        "[--spec-opts k=v:...] [-i] [-M] [-P] [--video PATH] [--trc NAME]\n"
		        "  --trc NAME: the input is NAME-coded (iec61966-2-1, bt709, gamma22, ...): decoded before the transform, frames and output encoded\n", argv[0]);
		return 2;
	}
	size_t width, height;
	const int channels = 3;
	float *pix;
	if (read_image(pos[0], &width, &height, &pix)) { fprintf(stderr, "cannot read %s\n", pos[0]); return 1; }
	const int frames_on = fo.visualize || fo.intermediates || parity || video != NULL;
	const char *mname = npos > 3 ? pos[3] : "zigzag";
	const uint32_t w = (uint32_t)width, h = (uint32_t)height;
	const size_t npix = width * height, n = npix * channels;

	float *d_coeffs, *d_sum, *d_work;
	uint32_t *d_ids, *d_index = NULL;       /* d_index: the owner index for the fill and inverted frames */
	HIP(hipMalloc((void **)&d_coeffs, n * 4)); HIP(hipMalloc((void **)&d_sum, n * 4)); HIP(hipMalloc((void **)&d_work, n * 4));
	HIP(hipMalloc((void **)&d_ids, npix * 4));
	HIP(hipMemcpy(d_coeffs, pix, n * 4, hipMemcpyHostToDevice));
	float *d_orig = NULL;
	if (trc) DSP(dspfft_trc_apply_f32(d_coeffs, d_coeffs, n, trc, 1, NULL));                              /* to linear light */
	if (parity) {                                                                                         /* scan.c:283-287 */
		HIP(hipMalloc((void **)&d_orig, n * 4));
		HIP(hipMemcpy(d_orig, d_coeffs, n * 4, hipMemcpyDeviceToDevice));
	}

	dspfft_plan fwd, inv;
	const int dims[2] = {(int)height, (int)width}, k10[2] = {DSPFFT_REDFT10, DSPFFT_REDFT10}, k01[2] = {DSPFFT_REDFT01, DSPFFT_REDFT01};
	DSP(dspfft_plan_many_r2r(&fwd, 2, dims, channels, NULL, channels, 1, NULL, channels, 1, k10));      /* scan.c:292 */
	DSP(dspfft_plan_set_scale(fwd, 1.0f / (4.0f * width * height)));                                   /* scan.c:296-298 fused */
	DSP(dspfft_plan_many_r2r(&inv, 2, dims, channels, NULL, channels, 1, NULL, channels, 1, k01));      /* scan.c:359 */
	DSP(dspfft_execute(fwd, d_coeffs, d_coeffs, NULL));

	/* ---- the scan order -> what the frame loop needs ---- */
	uint64_t limit = 0, slots = 0;
	int method = -1, per_frame_lists = 0;
	uint32_t *d_lin = NULL;                 /* per-frame coordinate lists (box, or a file whose indices share pixels) */
	struct scan_order_list fl;
	memset(&fl, 0, sizeof fl);
	if (!strncmp(mname, "magnitude", 9)) {
		const double q = mname[9] == ':' ? strtod(mname + 10, NULL) : 0.0;
		void *d_mw;
		const size_t wb = dspfft_scan_magnitude_work_bytes(w, h);
		uint32_t lim32;
		HIP(hipMalloc(&d_mw, wb));
		DSP(dspfft_scan_magnitude_index(d_ids, d_coeffs, w, h, channels, q, d_mw, wb, &lim32, NULL));
		HIP(hipFree(d_mw));
		limit = lim32;
	} else if (!strncmp(mname, "file:", 5) || !strncmp(mname, "random", 6)) {
		if (mname[0] == 'r') {
			const unsigned int seed = mname[6] == ':' ? (unsigned int)strtoul(mname + 7, NULL, 10) : (unsigned int)time(NULL);   /* scan_methods.c:216 */
			if (scan_order_random(width, height, seed, &fl)) { fprintf(stderr, "cannot draw the random scan order\n"); return 1; }
		} else {
			FILE *f = fopen(mname + 5, "r");
			if (!f || scan_order_read_file(f, width, height, &fl)) { fprintf(stderr, "cannot read the scan order %s\n", mname + 5); return 1; }
			fclose(f);
		}
		limit = fl.limit; slots = fl.max_interval;
		/* a pixel listed under several indices needs per-frame lists; otherwise one owner-index array does */
		uint32_t *owner = malloc(npix * 4);
		memset(owner, 0xff, npix * 4);
		for (size_t i = 0; i < fl.limit && !per_frame_lists; i++)
			for (size_t k = fl.offset[i]; k < fl.offset[i + 1]; k++) {
				const size_t p = fl.yx[k][0] * width + fl.yx[k][1];
				if (owner[p] != 0xffffffffu && owner[p] != i) { per_frame_lists = 1; break; }
				owner[p] = (uint32_t)i;
			}
		if (!per_frame_lists) HIP(hipMemcpy(d_ids, owner, npix * 4, hipMemcpyHostToDevice));    /* unlisted pixels keep 0xFFFFFFFF: never reconstructed */
		free(owner);
	} else {
		method = scan_order_find_prefix(mname);                                               /* scan.c:176 scan_method_find_prefix */
		if (method < 0) { fprintf(stderr, "unknown scan method %s\n", mname); return 2; }
		limit = dspfft_scan_limit(method, w, h);
		slots = dspfft_scan_coord_slots(method, w, h);
		per_frame_lists = method == DSPFFT_SCAN_BOX;
	}
	size_t step = npos > 2 ? strtoul(pos[2], NULL, 10) : (limit + 31) / 32;
	if (!step) step = 1;
	if (!nframes || nframes > limit / step) nframes = (limit + step - 1) / step;                  /* scan.c:347-348 */
	if (offset >= limit) offset = limit - 1;                                                      /* scan.c:385-386 */
	const int fill = !skip && offset > 0;
	/* ---- the output frames (scan.c:366-536) ---- */
	dspfft_scanframes sf = NULL;
	float *d_frame = NULL, *d_image = NULL, *h_frame[2] = {NULL, NULL};
	uint32_t *d_mark = NULL;                /* owner index with DC keeping its index (the marks); NULL: coordinate lists */
	FILE *vf = NULL;
	size_t ffloats = 0;
	hipEvent_t ev[2];
	if (frames_on) {
		FILE *f = fopen(pos[0], "rb");
		char magic[3] = {0, 0, 0};
		if (!f || fread(magic, 1, 2, f) != 2) { fprintf(stderr, "cannot read %s\n", pos[0]); return 1; }
		fclose(f);
		fo.parity_depth = parity ? (!strcmp(magic, "P6") ? 8 : 32) : 0;                           /* host/rawio.h: P6 8-bit, PF float */
		DSP(dspfft_scanframes_create(&sf, w, h, &fo));
		if (trc) DSP(dspfft_scanframes_set_trc(sf, trc));
		ffloats = dspfft_scanframes_frame_floats(sf);
		HIP(hipMalloc((void **)&d_frame, ffloats * 4));
		if (fo.intermediates) {
			HIP(hipMalloc((void **)&d_image, n * 4));
			HIP(hipMemsetD32((hipDeviceptr_t)d_image, 0x80000000u, n));                           /* -0.0f: the step adds into it */
		}
		if (fo.visualize && !per_frame_lists) {
			HIP(hipMalloc((void **)&d_mark, npix * 4));
			if (method >= 0) DSP(dspfft_scan_owner_index(d_mark, method, w, h, NULL));
			else HIP(hipMemcpy(d_mark, d_ids, npix * 4, hipMemcpyDeviceToDevice));
		}
		if (video) {
			if (!(vf = fopen(video, "wb"))) { fprintf(stderr, "cannot write %s\n", video); return 1; }
			for (int k = 0; k < 2; k++) { HIP(hipHostMalloc((void **)&h_frame[k], ffloats * 4, 0)); HIP(hipEventCreate(&ev[k])); }
			fprintf(stderr, "video: %zu frames of gbrpf32le %zux%zu (ffmpeg -f rawvideo -pix_fmt gbrpf32le -s %zux%zu -r 20 -i %s)\n", nframes,
			        width * (1 + fo.visualize), height * (1 + fo.intermediates), width * (1 + fo.visualize), height * (1 + fo.intermediates), video);
		}
		DSP(dspfft_scanframes_begin(sf, d_frame, d_coeffs, NULL));
	}
	if (!per_frame_lists && (fill || invert)) {                                                   /* the owner index, DC unmarked */
		HIP(hipMalloc((void **)&d_index, npix * 4));
		if (method >= 0) DSP(dspfft_scan_owner_index(d_index, method, w, h, NULL));
		else HIP(hipMemcpy(d_index, d_ids, npix * 4, hipMemcpyDeviceToDevice));                    /* magnitude / file: still the index */
		HIP(hipMemset(d_index, 0xff, 4));
	}
	if (per_frame_lists) {
		HIP(hipMalloc((void **)&d_lin, (size_t)step * (slots ? slots : 1) * 4));
		HIP(hipMemset(d_ids, 0xff, npix * 4));
	} else if (method >= 0) DSP(dspfft_scan_frame_ids(d_ids, method, w, h, step, NULL));
	else DSP(dspfft_scan_index_to_frame_ids(d_ids, npix, step, NULL));                            /* magnitude / file: index -> frame */
	/* owner ids that stay put over the frames: let the fused step skip the column tiles a frame does not touch (box restamps its ids) */
	if (!per_frame_lists) DSP(dspfft_plan_scan_prepare(inv, invert ? d_index : d_ids, channels, NULL));

	DSP(dspfft_broadcast_dc(d_sum, d_coeffs, npix, channels, NULL));                              /* scan.c:377-383 */
	uint32_t *h_lin = per_frame_lists && method < 0 ? malloc((size_t)step * (slots ? slots : 1) * 4) : NULL;
	/* stamps d_ids[pixels of scan indices [a, b)] = id, at most `step` indices per list (the size of d_lin) */
	#define STAMP(a, b, id) do { \
		for (size_t c0 = (a); c0 < (b); c0 += step) { \
			const size_t c1 = c0 + step < (b) ? c0 + step : (b); \
			size_t cnt; \
			if (method >= 0) { DSP(dspfft_scan_coords(d_lin, method, w, h, c0, c1 - c0, NULL)); cnt = (c1 - c0) * slots; } \
			else { \
				cnt = fl.offset[c1] - fl.offset[c0]; \
				for (size_t k = 0; k < cnt; k++) h_lin[k] = (uint32_t)(fl.yx[fl.offset[c0] + k][0] * width + fl.yx[fl.offset[c0] + k][1]); \
				HIP(hipMemcpy(d_lin, h_lin, cnt * 4, hipMemcpyHostToDevice)); \
			} \
			DSP(dspfft_scan_stamp(d_ids, d_lin, cnt, (id), NULL)); \
			if (sf) DSP(dspfft_scanframes_mark_coords(sf, d_frame, d_coeffs, d_lin, cnt, (id) != FILL_ID, NULL)); \
		} \
	} while (0)
	if (fill) {                                                                                   /* scan.c:389-417 */
		const size_t a = invert ? limit - offset : 0, b = invert ? limit : offset;
		if (d_mark) DSP(dspfft_scanframes_mark_range(sf, d_frame, d_coeffs, d_mark, (uint32_t)a, (uint32_t)b, 0, NULL));
		if (per_frame_lists) {
			STAMP(a, b, FILL_ID);
			DSP(dspfft_execute_masked_accumulate(inv, d_coeffs, d_work, d_sum, d_ids, FILL_ID, channels, NULL));
		} else DSP(dspfft_execute_masked_accumulate_range(inv, d_coeffs, d_work, d_sum, d_index, (uint32_t)a, (uint32_t)b, channels, NULL));
	}
	for (size_t i = offset; i < offset + nframes; i++) {                                          /* scan.c:421-459 */
		const size_t lo = i * step, hi = lo + step < limit ? lo + step : limit;
		float *acc = d_image ? d_image : d_sum;          /* -i: this frame's inverse alone, added to the sum by compose */
		if (lo < limit) {
			const size_t a = invert ? limit - hi : lo, b = invert ? limit - lo : hi;             /* scan.c:424 j = limit - 1 - s */
			if (d_mark) DSP(dspfft_scanframes_mark_range(sf, d_frame, d_coeffs, d_mark, (uint32_t)a, (uint32_t)b, 1, NULL));
			if (per_frame_lists) STAMP(a, b, (uint32_t)i);
			if (invert && !per_frame_lists)
				DSP(dspfft_execute_masked_accumulate_range(inv, d_coeffs, d_work, acc, d_index, (uint32_t)a, (uint32_t)b, channels, NULL));
			else DSP(dspfft_execute_masked_accumulate(inv, d_coeffs, d_work, acc, d_ids, (uint32_t)i, channels, NULL));
		} else if (!sf) continue;                        /* no scan index left: the frame adds nothing (the sum is emitted unchanged) */
		else if (d_mark) DSP(dspfft_scanframes_mark_range(sf, d_frame, d_coeffs, d_mark, 0, 0, 1, NULL));     /* clears the last marks */
		else if (fo.visualize) DSP(dspfft_scanframes_mark_coords(sf, d_frame, d_coeffs, NULL, 0, 1, NULL));
		if (!sf) continue;
		DSP(dspfft_scanframes_compose(sf, d_frame, d_sum, d_image, d_coeffs, d_orig, i - offset, NULL));
		if (vf) {
			const size_t k = (i - offset) & 1;
			HIP(hipMemcpyAsync(h_frame[k], d_frame, ffloats * 4, hipMemcpyDeviceToHost, NULL));
			HIP(hipEventRecord(ev[k], NULL));
			if (i > offset) {                            /* the previous frame is written while this one copies */
				HIP(hipEventSynchronize(ev[k ^ 1]));
				if (fwrite(h_frame[k ^ 1], 4, ffloats, vf) != ffloats) { fprintf(stderr, "error writing %s\n", video); return 1; }
			}
		}
	}
	if (vf) {
		if (nframes) {
			const size_t k = (nframes - 1) & 1;
			HIP(hipEventSynchronize(ev[k]));
			if (fwrite(h_frame[k], 4, ffloats, vf) != ffloats) { fprintf(stderr, "error writing %s\n", video); return 1; }
		}
		if (fclose(vf)) { fprintf(stderr, "error writing %s\n", video); return 1; }
		for (int k = 0; k < 2; k++) { HIP(hipHostFree(h_frame[k])); HIP(hipEventDestroy(ev[k])); }
	}
	if (parity) {                                                                                 /* scan.c:530-536 */
		uint64_t pf;
		DSP(dspfft_scanframes_parity(sf, &pf, NULL));
		if (pf == UINT64_MAX) fprintf(stderr, "Didn't reach parity with the original image before the end of the scan.\n");
		else fprintf(stderr, "Reached parity with the original image at scan index %llu\n", (unsigned long long)pf);
	}
	#undef STAMP
	float *sum = malloc(n * 4);
	if (trc) DSP(dspfft_trc_apply_f32(d_sum, d_sum, n, trc, 0, NULL));                                    /* the output is coded as the input was */
	HIP(hipMemcpy(sum, d_sum, n * 4, hipMemcpyDeviceToHost));
	double err = 0;
	for (size_t j = 0; j < n; j++) { const double e = fabs((double)sum[j] - pix[j]); if (e > err) err = e; }
	fprintf(stderr, "method %s: %zu scan indices, %zu frames of %zu, device-resident; max|sum-input| = %.3e\n", mname, (size_t)limit, nframes, step, err);
	const int rc = write_pf(pos[1], width, height, sum);
	dspfft_destroy_plan(fwd); dspfft_destroy_plan(inv);
	dspfft_scanframes_destroy(sf);
	hipFree(d_coeffs); hipFree(d_sum); hipFree(d_work); hipFree(d_ids); hipFree(d_index); hipFree(d_lin);
	hipFree(d_frame); hipFree(d_image); hipFree(d_orig); hipFree(d_mark);
	free(sum); free(pix); free(h_lin); scan_order_list_free(&fl);
	return rc;
}
