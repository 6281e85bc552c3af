"""Regenerates tests/golden/ref_scan_frames.npz from the REFERENCE'S OWN frame loop.  Needs the reference tree (DSPFUN_REFERENCE) and gcc;
the tests only read the .npz.

Same method as make_ref_fixtures.py / make_dither_fixtures.py: the text of these line ranges is read from the reference at generation time
into a temporary translation unit, around this script's own declarations of the variables they use, and compiled with plain gcc
(-std=c11 -O2 -ffp-contract=off, no -ffast-math, COEFF_PRECISION=F INTERMEDIATE_PRECISION=D as scan/Makefile:1-2 builds):

  scan/scan.c:366-375             the spectrogram scaler
  scan/scan.c:379-417             clear the frame, DC into the sum, the fill
  scan/scan.c:419-527             the frame loop: panels, intermediates, parity
  scan/scan_methods.c             the parts make_ref_fixtures.py compiles (everything but libavutil's evaluator), so coordinate order
                                  and DC placement are the reference's; radial / iradial / magnitude through their own init functions
  scan/scan_precomputed.c         as it lies (the `file` method's parser)
  include/speclib.c               as it lies

Stand-ins written for this script: scan_context's four accessors over the method's functions; ffapi_setpelf stores into a GBR-planar float
frame (libavutil's comp[] order: R plane 2, G 0, B 1); ffapi_write_frame appends a copy; fftw(execute)(inverse) is the float DCT-III of
tests/scan_frames_stub.h (the CPU restatement compiles the same file); use_fftw is 1 (the pruned IDCT is not this feature).

Inputs are not stored: tests/scan_frames_ref.py regenerates them from the recorded seeds.  Only the frames and the parity frame go in."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DSPFUN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import scan_frames_ref as sfr  # noqa: E402

METHOD = {"horizontal": 0, "vertical": 1, "zigzag": 2, "row": 3, "column": 4, "diagonal": 5, "mirror": 6, "box": 7, "ibox": 8,
          "radial": 9, "iradial": 10, "magnitude": 11, "file": 12}


def lines(path, a, b):
    with open(os.path.join(REF, path)) as f:
        src = f.read().split("\n")
    return "\n".join(src[a - 1:b]) + "\n"


def build(tmp):
    tu = "#include <stdlib.h>\n#include <stdint.h>\n#include <stdbool.h>\n#include <string.h>\n#include <stdio.h>\n#include <math.h>\n"
    tu += lines("scan/scan_methods.c", 5, 7) + lines("scan/scan_methods.c", 11, 14) + lines("scan/scan_methods.c", 16, 184) + lines("scan/scan_methods.c", 203, 331)
    tu += '#include "speclib.h"\n#include "scan_frames_stub.h"\n'
    tu += r"""
/* ---- this script's stand-ins ---- */
struct scan_context { int m; struct scan_precomputed *p; size_t width, height, limit, max_interval; };
typedef void (*scan_fn)(void*, size_t, size_t, size_t, size_t (*)[2]);
static scan_fn fn_of(int m) { scan_fn t[] = {scan_horiz, scan_vert, scan_zigzag, scan_row, scan_col, scan_diag, scan_mirror, scan_box, scan_ibox}; return t[m]; }
void scan(struct scan_context *c, size_t i, size_t (*coords)[2]) { if (c->p) scan_precomputed(c->p, c->width, c->height, i, coords); else fn_of(c->m)(0, c->width, c->height, i, coords); }
size_t scan_interval(struct scan_context *c, size_t i)
{
	size_t w = c->width, h = c->height;
	if (c->p) return interval_precomputed(c->p, w, h, i);
	switch (c->m) { case 3: return w; case 4: return h; case 5: return interval_diag(0, w, h, i); case 6: return interval_mirror(0, w, h, i);
	                case 7: return interval_box(0, w, h, i); case 8: return interval_ibox(0, w, h, i); default: return 1; }
}
size_t scan_limit(struct scan_context *c) { return c->limit; }
size_t scan_max_interval(struct scan_context *c) { return c->max_interval; }
static size_t ctx_limit(int m, size_t w, size_t h)
{
	switch (m) { case 3: return limit_height(0, w, h); case 4: return limit_width(0, w, h); case 5: return limit_sum(0, w, h); case 6: case 7: return limit_max(0, w, h);
	             case 8: return limit_min(0, w, h); default: return w * h; }
}
static size_t ctx_max_interval(int m, size_t w, size_t h)
{
	switch (m) { case 3: return limit_width(0, w, h); case 4: return limit_height(0, w, h); case 5: return limit_min(0, w, h); case 6: return limit_mirror(0, w, h);
	             case 7: case 8: return limit_sum(0, w, h); default: return 1; }
}

static float *g_frame, *g_out, *g_recon, *g_image;
static size_t g_fw, g_fh, g_w, g_h, g_nout;
static void stub_setpelf(size_t x, size_t y, unsigned z, float v) { const size_t pl = z == 0 ? 2 : z - 1; g_frame[(pl * g_fh + y) * g_fw + x] = v; }
static int stub_write_frame(void) { memcpy(g_out + g_nout * 3 * g_fw * g_fh, g_frame, sizeof(float) * 3 * g_fw * g_fh); g_nout++; return 0; }
#define ffapi_setpelf(ctx, frame, x, y, z, v) stub_setpelf((x), (y), (z), (v))
#define ffapi_write_frame(ctx, frame) stub_write_frame()
#define ffapi_clear_frame(frame) memset(g_frame, 0, sizeof(float) * 3 * g_fw * g_fh)
#define av_err2str(e) ""
void fftwf_execute(void *plan) { (void)plan; sf_stub_redft01_2d(g_recon, g_image, g_w, g_h, 3); }
static void pruned_idct(coeff **b, coeff *r, coeff *i, size_t (*c)[2], size_t n, size_t w, size_t h, size_t ch) { abort(); }

/* m: 0..8 closed-form methods, 9 radial, 10 iradial, 11 magnitude, 12 file (path); offset / nframes as scan.c:346-348 leaves them */
int ref_scan_frames(int m, const char *path, size_t width, size_t height, coeff *coeffs, coeff *original, size_t original_depth,
                    size_t step, size_t offset, size_t nframes, int invert_, int skip, int v_, int s_, int i_, int M_, double gain_, int scale_, int sign_,
                    float *out, size_t *parity_out)
{
	const size_t channels = 3;
	bool invert = invert_, fill_offset = !skip, visualize = v_ || s_, spec = s_, intermediates = i_ || M_, max_intermediates = M_;
	bool measure_parity = original_depth != 0, quiet = true;
	int use_fftw = 1, ret = 0;
	intermediate gain = gain_;
	struct spec_params sparams = {scale_, sign_};
	void *ffctx = NULL, *frame = NULL, *inverse = NULL;
	intermediate (*trc_encode)(intermediate) = NULL;
	coeff *basis[2] = {NULL, NULL};
	struct scan_context ctx = {m < 9 ? m : -1, NULL, width, height, 0, 0}, *scanctx = &ctx;
	if (m == 9) ctx.p = init_radial(width, height, channels, coeffs, NULL);
	else if (m == 10) ctx.p = init_iradial(width, height, channels, coeffs, NULL);
	else if (m == 11) ctx.p = init_magnitude(width, height, channels, coeffs, NULL);
	else if (m == 12) { FILE *f = fopen(path, "r"); ctx.p = f ? scan_precomputed_unserialize(f) : NULL; if (f) fclose(f); }
	if (m >= 9 && !ctx.p) return -1;
	ctx.limit = ctx.p ? limit_precomputed(ctx.p, width, height) : ctx_limit(m, width, height);
	ctx.max_interval = ctx.p ? max_interval_precomputed(ctx.p, width, height) : ctx_max_interval(m, width, height);
	size_t max_interval = scan_max_interval(scanctx);
	size_t limit = scan_limit(scanctx);
	size_t (*coords)[2] = malloc(sizeof(*coords) * (max_interval + 1) * step);
	coeff *reconstruction = calloc(width * height * channels, sizeof(coeff)), *image = calloc(width * height * channels, sizeof(coeff));
	g_w = width; g_h = height; g_fw = width * (!!visualize + 1); g_fh = height * (!!intermediates + 1);
	g_frame = malloc(sizeof(float) * 3 * g_fw * g_fh); g_out = out; g_nout = 0; g_recon = reconstruction; g_image = image;
"""
    tu += lines("scan/scan.c", 365, 375) + lines("scan/scan.c", 377, 417) + lines("scan/scan.c", 419, 527)
    tu += r"""
err:
	*parity_out = parity_index == nframes ? (size_t)-1 : parity_index;
	spec_destroy(sp); free(sum); free(coords); free(reconstruction); free(image); free(g_frame);
	(void)ffctx; (void)frame; (void)inverse; (void)use_fftw; (void)basis; (void)quiet; (void)trc_encode; (void)pad;
	return ret ? -2 : (int)g_nout;
}
"""
    src = os.path.join(tmp, "scan_frames.c")
    so = os.path.join(tmp, "scan_frames.so")
    with open(src, "w") as f:
        f.write(tu)
    subprocess.check_call(["gcc", "-std=gnu11", "-D_GNU_SOURCE", "-DCOEFF_PRECISION=F", "-DINTERMEDIATE_PRECISION=D", "-O2", "-ffp-contract=off",
                           "-fPIC", "-shared", "-w", "-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "scan"), "-I" + os.path.dirname(HERE),
                           src, os.path.join(REF, "scan", "scan_precomputed.c"), os.path.join(REF, "include", "speclib.c"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    st, vp = C.c_size_t, C.c_void_p
    lib.ref_scan_frames.argtypes = [C.c_int, C.c_char_p, st, st, vp, vp, st, st, st, st] + [C.c_int] * 6 + [C.c_double, C.c_int, C.c_int, vp, vp]
    return lib


def run(lib, case, tmp):
    name, w, h, seed, method, step, _o, _n, invert, skip = case[:10]
    o = sfr.opts(case)
    orig, co = sfr.case_inputs(case)
    order = sfr.orders(case, co)                   # the restatement's order: only its length and the `file` text are used here
    path = b""
    if method == "file":
        p = os.path.join(tmp, name + ".txt")
        with open(p, "w") as f:
            for cs in order:
                f.write(" ".join("%d,%d" % (x, y) for (y, x) in cs) + "\n")
        path = p.encode()
    limit = len(order)
    offset, nframes = sfr.loop_params(case, limit)
    frames = np.zeros((nframes,) + sfr.frame_shape(case), dtype=np.float32)
    par = np.zeros(1, dtype=np.uint64)
    gain = o["gain"]                               # 0: scan.c:367-368's default
    c = np.ascontiguousarray(co, dtype=np.float32).copy()
    g = np.ascontiguousarray(orig, dtype=np.float32).copy()
    n = lib.ref_scan_frames(METHOD[method], path, w, h, c.ctypes.data, g.ctypes.data, o["P"], step, offset, nframes, int(invert), int(skip),
                            o["v"], o["s"], o["i"], o["M"], float(gain), sfr.SCALES[o["scale"]], sfr.SIGNS[o["sign"]], frames.ctypes.data, par.ctypes.data)
    assert n == nframes, (name, n, nframes)
    p = int(par[0])
    return frames, np.array([-1 if p == 2 ** 64 - 1 else p], dtype=np.int64)


def main(path=os.path.join(HERE, "ref_scan_frames.npz")):
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        for case in sfr.CASES:
            arrays["frames_" + case[0]], arrays["parity_" + case[0]] = run(lib, case, tmp)
            arrays["seed_" + case[0]] = np.array([case[3]], dtype=np.int64)
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
