/* zoom_args.h -- zoom's option arithmetic before its frame loop (zoom/zoom.c:268-303), in the tool's default INTERMEDIATE_PRECISION=L
 * (long double), for host harnesses and, as host/libzoomargs.so, the CPU tests. */
#ifndef ZOOM_ARGS_H
#define ZOOM_ARGS_H
#include <stddef.h>

/* In: the image size, -r's logical size (0: not given), -s's scales, -v's view (0: not given), -p's position and the -%, -P, -c flags.
 * Out (in place): the scales and view the loop starts from and the position.  The reference's quirks are kept: -r replaces a scale by
 * logical / size; a scaled length below 1 clamps the scale to 1 / size; the default view truncates the scaled size; -% multiplies vx by
 * vw / 100 in INTEGER division and vy by vy / 100; -P multiplies by the scales; -c centres once, on the initial scale (later per-frame
 * scales do not re-centre); the first of -%, -P, -c given wins. */
void zoom_viewport(size_t width, size_t height, long double logical_width, long double logical_height,
                   long double *xnum, unsigned long long *xden, long double *ynum, unsigned long long *yden,
                   size_t *vw, size_t *vh, long double *vx, long double *vy, int pct_coords, int input_coords, int centered);
#endif
