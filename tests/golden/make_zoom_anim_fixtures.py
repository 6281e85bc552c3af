"""Regenerates tests/golden/ref_zoom_anim.npz from the REFERENCE'S OWN animation loop.  Needs the reference tree (DSPFUN_REFERENCE) and
gcc; the tests only read the .npz.

Same method as make_scan_frames_fixtures.py: the text of these line ranges is read from the reference at generation time into a temporary
translation unit, around this script's own declarations of the variables they use, and compiled with plain gcc (-std=c11 -O2
-ffp-contract=off, no -ffast-math, COEFF_PRECISION=D INTERMEDIATE_PRECISION=L as zoom/Makefile:1-2 builds):

  zoom/zoom.c:22-68     scaling_type, sample_display, min(), generate_scaled_basis
  zoom/zoom.c:320-410   the frame loop: per-frame expressions, the non-finite skip, basis and product, --showsamples, the frame store
  zoom/zoom.c:268-303   the viewport rules (-r, the < 1 clamps, default view, -%, -P, -c), as a function

Stand-ins written for this script: av_expr_eval returns the recorded table value of (expression, vars[0] = frame number); ffapi_setpelf
stores into a GBR-planar float frame (libavutil's comp[] order: R plane 2, G 0, B 1); ffapi_write_frame appends a copy (a skipped frame
appends nothing); trc_encode is NULL.  Only numbers go into the .npz."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DSPFUN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
from oracle_lib import synth_f32  # noqa: E402

NAN, INF = float("nan"), float("inf")


def lines(path, a, b):
    with open(os.path.join(REF, path)) as f:
        src = f.read().split("\n")
    return "\n".join(src[a - 1:b]) + "\n"


def build(tmp):
    tu = "#include <stdlib.h>\n#include <stdio.h>\n#include <stdbool.h>\n#include <string.h>\n#include <math.h>\n#include \"precision.h\"\n"
    tu += lines("zoom/zoom.c", 22, 68)
    tu += r"""
/* ---- this script's stand-ins ---- */
typedef struct { int id; } AVExpr;
static const double *g_table;
static double av_expr_eval(AVExpr *e, const double *vars, void *opaque) { (void)opaque; return g_table[(size_t)vars[0] * 5 + e->id]; }
static float *g_frame, *g_out;
static size_t g_vw, g_vh, g_nout;
static void stub_setpelf(size_t x, size_t y, unsigned z, float v) { const size_t pl = z == 0 ? 2 : z - 1; g_frame[(pl * g_vh + y) * g_vw + x] = v; }
static int stub_write_frame(void) { memcpy(g_out + g_nout * 3 * g_vw * g_vh, g_frame, sizeof(float) * 3 * g_vw * g_vh); g_nout++; return 0; }
#define ffapi_setpelf(ctx, frame, x, y, z, v) stub_setpelf((x), (y), (z), (v))
#define ffapi_write_frame(ctx, frame) stub_write_frame()
#define av_err2str(e) ""

/* the frame loop over a table of nframes x 5 expression values (x y S X Y; present[i] = 0: that expression was not given).
   Returns the number of frames written to out (3 x vh x vw floats each), the frame numbers in kept. */
int ref_zoom_anim(const double *coeffs, size_t width, size_t height, int scaling_type, size_t vw, size_t vh, int showsamples,
                  long double vx, long double vy, long double xscale_num, unsigned long long xscale_den, long double yscale_num,
                  unsigned long long yscale_den, size_t nframes, const double *table, const int *present, float *out, long long *kept)
{
	AVExpr e[5] = {{0}, {1}, {2}, {3}, {4}};
	AVExpr *xexpr = present[0] ? &e[0] : NULL, *yexpr = present[1] ? &e[1] : NULL, *scaleexpr = present[2] ? &e[2] : NULL,
	       *xscaleexpr = present[3] ? &e[3] : NULL, *yscaleexpr = present[4] ? &e[4] : NULL;
	bool quiet = true;
	int ret = 0;
	void *ffctx = NULL, *frame = NULL;
	double (*trc_encode)(double) = NULL;
	size_t maxvectors = vh > vw ? vh : vw;
	g_table = table; g_vw = vw; g_vh = vh; g_out = out; g_nout = 0;
	g_frame = calloc(3 * vw * vh, sizeof(float));
	coeff* icoeffs = malloc(vw*vh*3*sizeof(*icoeffs));
	coeff* xbasis = NULL,* ybuf = NULL;
	intermediate* tmp = NULL;
"""
    # the loop, with one line of this script's after the non-finite skip: record the frame number the next write belongs to
    loop = lines("zoom/zoom.c", 320, 410)
    skip_end = "\t\t\tcontinue;\n\t\t}\n"
    assert loop.count(skip_end) == 1
    loop = loop.replace(skip_end, skip_end + "\t\tkept[g_nout] = (long long)d;\n", 1)
    tu += loop
    tu += r"""
err:
	free(tmp); free(xbasis); free(ybuf); free(icoeffs); free(g_frame);
	(void)ffctx; (void)frame; (void)quiet;
	return ret ? -1 : (int)g_nout;
}

/* zoom.c:268-303 as a function: the scales, view size and position the frame loop starts from */
void ref_viewport(size_t width, size_t height, long double logical_width, long double logical_height, long double *xnum, unsigned long long *xden,
                  long double *ynum, unsigned long long *yden, size_t *vw_, size_t *vh_, long double *vx_, long double *vy_, int pct_coords, int input_coords,
                  int centered)
{
	long double xscale_num = *xnum, yscale_num = *ynum, vx = *vx_, vy = *vy_;
	unsigned long long xscale_den = *xden, yscale_den = *yden;
	size_t vw = *vw_, vh = *vh_;
"""
    tu += lines("zoom/zoom.c", 268, 303)
    tu += r"""
	(void)maxvectors;
	*xnum = xscale_num; *xden = xscale_den; *ynum = yscale_num; *yden = yscale_den; *vw_ = vw; *vh_ = vh; *vx_ = vx; *vy_ = vy;
}
"""
    src = os.path.join(tmp, "zoom_anim.c")
    so = os.path.join(tmp, "zoom_anim.so")
    with open(src, "w") as f:
        f.write(tu)
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-DCOEFF_PRECISION=D", "-DINTERMEDIATE_PRECISION=L", "-O2", "-ffp-contract=off",
                           "-fPIC", "-shared", "-I" + os.path.join(REF, "include"), src, "-o", so, "-lm"])
    return C.CDLL(so)


def coefficients(seed, w, h):
    """make_ref_fixtures.py's draw (zero-mean values times 4 w h), rounded to float32: the device's coefficients are float"""
    return ((synth_f32(seed, h * w * 3).astype(np.float64) * 2 - 1) * (4 * w * h)).astype(np.float32).reshape(h, w, 3)


def ramp(a, b, n):
    return [a + (b - a) * i / (n - 1) for i in range(n)]


# (name, w, h, type, vw, vh, showsamples, (vx, vy, xnum, xden, ynum, yden) initial state, present x y S X Y, table rows)
# type: 0 interpolated, 1 centered, 2 native; showsamples: 0 none, 1 point, 2 grid
def cases():
    c = []
    zin = ramp(0.8, 2.3, 7)                                                 # non-integer scales crossing 1x
    rows = [[0.5 * i, 0.25 * i, s, NAN, NAN] for i, s in enumerate(zin)]
    rows.insert(3, [1.0, 1.0, NAN, NAN, NAN])                               # a NaN scale: skipped, the state keeps the NaN until S is finite again
    rows.insert(5, [INF, 0.0, 1.5, NAN, NAN])                               # a non-finite offset
    for t in (0, 1, 2):
        c.append((f"zoomin_t{t}", 16, 12, t, 24, 18, 0, (0.0, 0.0, 1.0, 1, 1.0, 1), (1, 1, 1, 0, 0), rows))
    c.append(("down_t2", 20, 16, 2, 14, 10, 0, (0.0, 0.0, 1.0, 1, 1.0, 1), (1, 1, 1, 0, 0),
              [[0.0, 0.0, 0.5, NAN, NAN], [1.5, 0.5, 0.65, NAN, NAN], [0.0, 2.0, 0.3, NAN, NAN], [3.0, 1.0, 0.12, NAN, NAN]]))   # (2 components: one would make zoom.c:42 realloc to 0 bytes)
    c.append(("down_t0", 20, 16, 0, 14, 10, 0, (0.0, 0.0, 1.0, 1, 1.0, 1), (0, 0, 1, 0, 0),
              [[NAN, NAN, s, NAN, NAN] for s in (0.5, 0.7, 0.35)]))
    c.append(("xy_t0", 18, 14, 0, 30, 22, 0, (2.0, 1.0, 1.0, 1, 1.0, 1), (0, 0, 0, 1, 1),
              [[NAN, NAN, NAN, x, y] for x, y in zip(ramp(1.3, 2.2, 4), ramp(0.7, 1.6, 4))]))
    c.append(("xy_t1", 18, 14, 1, 30, 22, 0, (0.0, 0.0, 1.0, 1, 1.0, 1), (1, 0, 0, 1, 0),        # X alone: the vertical scale stays at its initial 1
              [[0.5, NAN, NAN, 1.7, NAN], [1.0, NAN, NAN, 2.4, NAN], [1.5, NAN, NAN, 1.1, NAN]]))
    c.append(("pan_t0", 16, 12, 0, 24, 20, 0, (0.0, 0.0, 2.0, 1, 2.0, 1), (1, 1, 0, 0, 0),
              [[1.25 * i, 0.75 * i, NAN, NAN, NAN] for i in range(5)]))
    c.append(("pan_t2", 16, 12, 2, 24, 20, 0, (0.0, 0.0, 2.0, 1, 3.0, 1), (1, 1, 0, 0, 0),
              [[1.5 * i, 2.0 * i, NAN, NAN, NAN] for i in range(4)]))
    for mode in (1, 2):
        c.append((f"show{mode}_wide", 16, 12, 0, 40, 24, mode, (0.0, 0.0, 1.0, 1, 1.0, 1), (1, 1, 0, 1, 1),    # vh < vw
                  [[0.0, 0.0, NAN, 2.5, 3.0], [3.0, 5.0, NAN, 3.0, 2.5], [7.5, 2.25, NAN, 2.75, 2.0], [1.0, 1.0, NAN, 0.9, 3.0]]))
        c.append((f"show{mode}_square", 16, 16, 1, 32, 32, mode, (0.0, 0.0, 1.0, 1, 1.0, 1), (1, 1, 1, 0, 0),  # vh = vw, square input
                  [[0.0, 0.0, 2.0, NAN, NAN], [3.0, 3.0, 2.5, NAN, NAN], [5.0, 2.0, 3.25, NAN, NAN]]))
    return c


def viewport_grid():
    """(width, height, logical_w, logical_h, xnum, xden, ynum, yden, vw, vh, vx, vy, pct, input, centered)"""
    g = []
    for (w, h) in ((16, 12), (1920, 1080)):
        for scale in ((1.0, 1, 1.0, 1), (2.0, 1, 2.0, 1), (3.0, 2, 3.0, 2), (2.5, 1, 1.75, 1), (1.0, 4000, 1.0, 3000), (7.0, 3, 5.0, 1)):
            for logical in ((0.0, 0.0), (2.5 * w, 0.0), (0.0, 3.25 * h)):
                for view in ((0, 0), (37, 23)):
                    for pos in ((0.0, 0.0), (12.5, 7.25)):
                        for flags in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                            g.append((w, h) + logical + scale + view + pos + flags)
    return g


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        vp, ld, sz = C.c_void_p, C.c_longdouble, C.c_size_t
        lib.ref_zoom_anim.restype = C.c_int
        lib.ref_zoom_anim.argtypes = [vp, sz, sz, C.c_int, sz, sz, C.c_int, ld, ld, ld, C.c_ulonglong, ld, C.c_ulonglong, sz, vp, vp, vp, vp]
        cs = cases()
        for i, (_, w, h, typ, vw, vh, show, (vx, vy, xn, xd, yn, yd), present, rows) in enumerate(cs):
            coeffs = coefficients(0xD5F2A00 + i, w, h)
            table = np.ascontiguousarray(rows, dtype=np.float64)
            pres = np.array(present, dtype=np.int32)
            n = len(rows)
            frames = np.zeros((n, 3, vh, vw), dtype=np.float32)
            kept = np.full(n, -1, dtype=np.int64)
            c64 = np.ascontiguousarray(coeffs, dtype=np.float64)
            nk = lib.ref_zoom_anim(c64.ctypes.data, w, h, typ, vw, vh, show, vx, vy, xn, xd, yn, yd, n, table.ctypes.data, pres.ctypes.data,
                                   frames.ctypes.data, kept.ctypes.data)
            name = f"c{i}"
            assert nk >= 0, (name, cs[i][0])
            out[f"{name}_geom"] = np.array([w, h, typ, vw, vh, show, vx, vy, xn, xd, yn, yd], dtype=np.float64)
            out[f"{name}_present"] = pres
            out[f"{name}_table"] = table
            out[f"{name}_coeffs"] = coeffs
            out[f"{name}_frames"] = frames[:nk]
            out[f"{name}_kept"] = kept[:nk]
            print(cs[i][0], (w, h, typ, vw, vh, show), "kept", list(kept[:nk]))
        out["ncases"] = np.array(len(cs))

        lib.ref_viewport.restype = None
        P = C.POINTER
        lib.ref_viewport.argtypes = [sz, sz, ld, ld, P(ld), P(C.c_ulonglong), P(ld), P(C.c_ulonglong), P(sz), P(sz), P(ld), P(ld), C.c_int, C.c_int, C.c_int]
        grid = viewport_grid()
        res = []
        for (w, h, lw, lh, xn, xd, yn, yd, vw, vh, vx, vy, pct, inp, cen) in grid:
            a = [ld(xn), C.c_ulonglong(xd), ld(yn), C.c_ulonglong(yd), sz(vw), sz(vh), ld(vx), ld(vy)]
            lib.ref_viewport(w, h, lw, lh, *[C.byref(x) for x in a], pct, inp, cen)
            res.append([float(x.value) for x in a])
        out["viewport_in"] = np.array(grid, dtype=np.float64)
        out["viewport_out"] = np.array(res, dtype=np.float64)
    path = os.path.join(HERE, "ref_zoom_anim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
