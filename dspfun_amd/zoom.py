"""Host-side mirror of zoom's frame computation (zoom/zoom.c:263-265 forward transform,
:347-375 basis generation and dense separable product) over device memory."""
import ctypes as C
import math

from . import _lib
from .engine import Plan, DspfftError, REDFT10, trc_apply, trc_id

INTERPOLATED, CENTERED, NATIVE = 0, 1, 2     # zoom/zoom.c:20-26
CACHE_PLANS = 4       # frame plans kept per path: an animated zoom (a new scale every frame) would otherwise keep a plan and a frame-sized work
                      # buffer (about 100 MB at 1080p -> 4K) alive per frame; the least recently used one is destroyed


class _PlanCache:
    """key -> (handle, work) or None ("does not apply"), at most CACHE_PLANS live handles, least recently used destroyed first"""

    def __init__(self, destroy):
        self.destroy, self.d = destroy, {}

    def get(self, key, make):
        if key in self.d:
            self.d[key] = self.d.pop(key)                  # most recently used last
            return self.d[key]
        v = self.d[key] = make()
        live = [k for k, e in self.d.items() if e is not None]
        for k in live[:max(0, len(live) - CACHE_PLANS)]:
            self.destroy(self.d.pop(k)[0])
        for k in [k for k, e in self.d.items() if e is None][:-64]:      # (the "does not apply" marks hold nothing; bounded all the same)
            del self.d[k]
        return v

    def __len__(self):
        return len(self.d)

    def values(self):
        return self.d.values()

    def clear(self):
        for e in self.d.values():
            if e is not None:
                self.destroy(e[0])
        self.d = {}


class Zoom:
    """coeffs = REDFT10^2(image) once (zoom.c:263-265); frame(...) per output frame (zoom.c:320-375)."""

    def __init__(self, torch, image_hwc):
        self.torch = torch
        self.lib = _lib.load()
        self.h, self.w, c = image_hwc.shape
        assert c == 3 and image_hwc.dtype == torch.float32 and image_hwc.is_cuda
        self.coeffs = image_hwc.contiguous().clone()
        Plan.image(self.h, self.w, 3, REDFT10).execute(self.coeffs.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)

    def _frame_fft(self, vw, vh, xscale, yscale, vx, vy, basis_type):
        key = (vw, vh, tuple(xscale), tuple(yscale), basis_type)
        if not hasattr(self, "_fft"):
            self._fft = _PlanCache(self.lib.dspfft_zoomfft_destroy)

        def make():
            z = C.c_void_p()
            rc = self.lib.dspfft_zoomfft_create(C.byref(z), self.w, self.h, basis_type, xscale[0], xscale[1], yscale[0], yscale[1], vw, vh)
            if rc == -2:
                return None                        # this scale / basis / viewport keeps the dense product
            if rc:
                raise DspfftError(self.lib.dspfft_zoomfft_last_error().decode())
            return (z, self.torch.empty(self.lib.dspfft_zoomfft_work_floats(z), dtype=self.torch.float32, device=self.coeffs.device))
        e = self._fft.get(key, make)
        if e is None:
            return None
        z, work = e
        out = self.torch.empty((vh, vw, 3), dtype=self.torch.float32, device=self.coeffs.device)
        if self.lib.dspfft_zoomfft_execute(z, self.coeffs.data_ptr(), float(vx), float(vy), out.data_ptr(), work.data_ptr(),
                                           self.torch.cuda.current_stream().cuda_stream):
            raise DspfftError(self.lib.dspfft_zoomfft_last_error().decode())
        return out

    def _frame_czt(self, vw, vh, xscale, yscale, vx, vy, basis_type):
        """chirp-z transforms along both axes (dspfft_zoomczt_*): any scale, offset and basis; None when an axis is too long for the
        listed convolution lengths"""
        key = (vw, vh, tuple(xscale), tuple(yscale), basis_type)
        if not hasattr(self, "_czt"):
            self._czt = _PlanCache(self.lib.dspfft_zoomczt_destroy)

        def make():
            z = C.c_void_p()
            rc = self.lib.dspfft_zoomczt_create(C.byref(z), self.w, self.h, basis_type, xscale[0], xscale[1], yscale[0], yscale[1], vw, vh)
            if rc == -2:
                return None
            if rc:
                raise DspfftError(self.lib.dspfft_zoomfft_last_error().decode())
            return (z, self.torch.empty(self.lib.dspfft_zoomczt_work_floats(z), dtype=self.torch.float32, device=self.coeffs.device))
        e = self._czt.get(key, make)
        if e is None:
            return None
        z, work = e
        out = self.torch.empty((vh, vw, 3), dtype=self.torch.float32, device=self.coeffs.device)
        if self.lib.dspfft_zoomczt_execute(z, self.coeffs.data_ptr(), float(vx), float(vy), out.data_ptr(), work.data_ptr(),
                                           self.torch.cuda.current_stream().cuda_stream):
            raise DspfftError(self.lib.dspfft_zoomfft_last_error().decode())
        return out

    def __del__(self):
        try:
            for c in (getattr(self, "_fft", None), getattr(self, "_czt", None)):
                if c is not None:
                    c.clear()
        except Exception:
            pass

    def _basis(self, basis_type, num, den, offset, nvectors, length):
        nc = self.lib.dspfft_zoom_ncomponents(num, den, length)
        b = self.torch.empty(nvectors * nc, dtype=self.torch.float32, device=self.coeffs.device)
        if self.lib.dspfft_zoom_basis(b.data_ptr(), basis_type, num, den, offset, nvectors, length, None):
            raise DspfftError(self.lib.dspfft_zoom_last_error().decode())
        return b, nc

    def animation(self, vw, vh, basis_type=INTERPOLATED, trc=0):
        """a ZoomAnimation over these coefficients: per-frame scale and offset without re-planning; trc (a name or an id, zoom -g):
        the transfer characteristic every output sample is encoded with"""
        return ZoomAnimation(self, vw, vh, basis_type, trc)

    def frame(self, vw, vh, xscale=(1.0, 1.0), yscale=(1.0, 1.0), vx=0.0, vy=0.0, basis_type=INTERPOLATED, method="auto"):
        """one output frame: (vh, vw, 3) f32.  method "auto": fast transforms on the DCT-III grid (dspfft_zoomfft_*) when the scaled lengths
        are integers and the basis is interpolated or native; chirp-z transforms (dspfft_zoomczt_*) for every other scale and the centered
        basis; the dense MFMA product only for axes beyond the listed convolution lengths.  "fft" / "czt" / "gemm" force one (fft and czt
        raise if they do not apply)."""
        torch = self.torch
        if method in ("auto", "fft"):
            out = self._frame_fft(vw, vh, xscale, yscale, vx, vy, basis_type)
            if out is not None:
                return out
            if method == "fft":
                raise DspfftError(self.lib.dspfft_zoomfft_last_error().decode())
        if method in ("auto", "czt"):
            out = self._frame_czt(vw, vh, xscale, yscale, vx, vy, basis_type)
            if out is not None:
                return out
            if method == "czt":
                raise DspfftError(self.lib.dspfft_zoomfft_last_error().decode())
        xb, cw = self._basis(basis_type, xscale[0], xscale[1], vx, vw, self.w)
        yb, ch = self._basis(basis_type, yscale[0], yscale[1], vy, vh, self.h)
        out = torch.empty((vh, vw, 3), dtype=torch.float32, device=self.coeffs.device)
        work = torch.empty(self.lib.dspfft_zoom_work_floats(self.w, self.h, ch, vw), dtype=torch.float32, device=self.coeffs.device)
        rc = self.lib.dspfft_zoom_product(self.coeffs.data_ptr(), self.w, self.h, xb.data_ptr(), cw, yb.data_ptr(), ch,
                                          out.data_ptr(), vw, vh, work.data_ptr(), None)
        if rc:
            raise DspfftError(self.lib.dspfft_zoom_last_error().decode())
        return out


LAYOUTS = {"rgb": 0, "gbr": 1}


def resolve_frames(table, present, vx=0.0, vy=0.0, xscale=(1.0, 1.0), yscale=(1.0, 1.0)):
    """zoom.c:320-345 with a table in place of the expressions: row d holds the values x y S X Y would give at frame d, present[i] says
    whether that expression was given.  S sets both scales to (value, 1), X and Y then override one axis each, x and y set the offsets;
    the state persists across frames (and across skipped ones).  Yields (d, xscale, yscale, vx, vy) for every frame the reference renders:
    a frame with a non-finite offset or scale is skipped, as zoom.c:342-345 does.  Finite scales of zero or below are yielded: the device
    clamps them to 1 / len as zoom.c:37-41 does (one component, the DC term alone)."""
    xn, xd = (float(v) for v in xscale)
    yn, yd = (float(v) for v in yscale)
    vx, vy = float(vx), float(vy)
    for d, row in enumerate(table):
        x, y, s, sx, sy = (float(v) for v in row)
        if present[2]:
            xn = yn = s
            xd = yd = 1.0
        if present[3]:
            xn, xd = sx, 1.0
        if present[4]:
            yn, yd = sy, 1.0
        if present[0]:
            vx = x
        if present[1]:
            vy = y
        if not all(math.isfinite(v) for v in (vx, vy, xn / xd, yn / yd)):
            continue
        yield d, (xn, xd), (yn, yd), vx, vy


class ZoomAnimation:
    """zoom's animation loop over one Zoom's coefficients (dspfft_zoomanim_*): one object for the geometry (vw, vh, basis), any scale and
    offset per frame, no allocation or re-planning between frames.  When the chirp-z plans do not cover the geometry (an axis longer than
    the listed convolutions), every frame takes the dense product (Zoom.frame(method="gemm")), which has no --showsamples overlay.
    The coefficients are transposed once, here: call refresh() after changing zoom.coeffs in place."""

    def __init__(self, zoom, vw, vh, basis_type=INTERPOLATED, trc=0):
        self.zoom, self.lib, self.torch = zoom, zoom.lib, zoom.torch
        self.vw, self.vh, self.basis_type, self.trc = vw, vh, basis_type, 0
        z = C.c_void_p()
        rc = self.lib.dspfft_zoomanim_create(C.byref(z), zoom.w, zoom.h, basis_type, vw, vh)
        if rc not in (0, -2):
            raise DspfftError(self.lib.dspfft_zoomanim_last_error().decode())
        self.z = z if rc == 0 else None
        if self.z is not None:
            self.work = self.torch.empty(self.lib.dspfft_zoomanim_work_floats(self.z), dtype=self.torch.float32, device=zoom.coeffs.device)
            self.refresh()
        self.set_trc(trc)

    def set_trc(self, trc):
        """zoom -g: encode every output sample (after the overlay) with this transfer characteristic, a name or an id; 0: none"""
        trc = trc_id(trc, self.lib)
        if self.z is not None and (trc or self.trc) and self.lib.dspfft_zoomanim_set_trc(self.z, trc):      # (0 on an object never told: no call)
            raise DspfftError(self.lib.dspfft_zoomanim_last_error().decode())
        self.trc = trc

    def refresh(self):
        if self.z is not None and self.lib.dspfft_zoomanim_set_coeffs(self.z, self.zoom.coeffs.data_ptr(), self.torch.cuda.current_stream().cuda_stream):
            raise DspfftError(self.lib.dspfft_zoomanim_last_error().decode())

    def frame(self, xscale, yscale, vx, vy, showsamples=0, layout="rgb", out=None):
        """one frame: (vh, vw, 3) for layout "rgb", (3, vh, vw) planes G, B, R for "gbr"; showsamples 0 none, 1 point, 2 grid"""
        torch, lay = self.torch, LAYOUTS[layout]
        shape = (self.vh, self.vw, 3) if lay == 0 else (3, self.vh, self.vw)
        if self.z is None:
            if showsamples:
                raise DspfftError("--showsamples is not built for the dense product (the chirp-z plans do not cover this geometry)")
            f = self.zoom.frame(self.vw, self.vh, xscale, yscale, vx, vy, self.basis_type, method="gemm")
            f = f if lay == 0 else f.permute(2, 0, 1)[[1, 2, 0]].contiguous()
            if self.trc:
                trc_apply(f, self.trc, out=f, lib=self.lib)
            if out is not None:
                out.copy_(f)
                return out
            return f
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.zoom.coeffs.device)
        rc = self.lib.dspfft_zoomanim_execute(self.z, float(xscale[0]), float(xscale[1]), float(yscale[0]), float(yscale[1]), float(vx), float(vy),
                                              showsamples, lay, out.data_ptr(), self.work.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc:
            raise DspfftError(self.lib.dspfft_zoomanim_last_error().decode())
        return out

    def frames(self, table, present, vx=0.0, vy=0.0, xscale=(1.0, 1.0), yscale=(1.0, 1.0), showsamples=0, layout="rgb"):
        """resolve_frames' frames rendered: yields (d, frame); a new tensor per frame"""
        for d, xs, ys, fx, fy in resolve_frames(table, present, vx, vy, xscale, yscale):
            yield d, self.frame(xs, ys, fx, fy, showsamples, layout)

    def __del__(self):
        try:
            if getattr(self, "z", None) is not None:
                self.lib.dspfft_zoomanim_destroy(self.z)
                self.z = None
        except Exception:
            pass
