/* zoom_args.c -- see zoom_args.h */
#include "zoom_args.h"

void zoom_viewport(size_t width, size_t height, long double logical_width, long double logical_height,
                   long double *xnum, unsigned long long *xden, long double *ynum, unsigned long long *yden,
                   size_t *vw, size_t *vh, long double *vx, long double *vy, int pct_coords, int input_coords, int centered)
{
	if (logical_width != 0) { *xnum = logical_width; *xden = width; }
	if (logical_height != 0) { *ynum = logical_height; *yden = height; }
	const long double sw = width * *xnum / *xden, sh = height * *ynum / *yden;
	if (sw < 1) { *xnum = 1; *xden = width; }
	if (sh < 1) { *ynum = 1; *yden = height; }
	const long double scaled_w = width * *xnum / *xden, scaled_h = height * *ynum / *yden;     /* after the clamps */
	if (*vw == 0) *vw = (size_t)scaled_w;
	if (*vh == 0) *vh = (size_t)scaled_h;
	if (pct_coords) {
		*vx *= *vw / 100;                     /* size_t division */
		*vy *= *vy / 100;                     /* vy, not vh */
	} else if (input_coords) {
		*vx *= *xnum / *xden;
		*vy *= *ynum / *yden;
	} else if (centered) {
		*vx = (scaled_w - *vw) / 2;
		*vy = (scaled_h - *vh) / 2;
	}
}
