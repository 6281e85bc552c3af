"""Host-side mirror of the FFTW plan/execute surface the reference uses (reference
include/precision.h:115 `fftw(call)`), over DEVICE memory.

    Plan.many_r2r(...)  <->  fftw(plan_many_r2r)   spec/spec.c:63  ispec.c:165  zoom.c:263  scan.c:292,359  motion.c:535-552
    Plan.r2r_2d(...)    <->  fftw(plan_r2r_2d)     applybasis/draw.c:74
    plan.execute(...)   <->  fftw(execute)
    plan.destroy()      <->  fftw(destroy_plan)

Pointers are raw device addresses (ints, e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t
handle as an int (torch.cuda.current_stream().cuda_stream) or 0 for the default stream.
"""
import ctypes as C

from . import _lib

REDFT01, REDFT10 = _lib.REDFT01, _lib.REDFT10


class DspfftError(RuntimeError):
    pass


def _ia(v):
    return None if v is None else (C.c_int * len(v))(*[int(x) for x in v])


def set_plan_effort(effort, lib=None):
    """dspfft_set_plan_effort: > 0 lets the plans made afterwards compile kernels for frame sizes spec_list.h does not list (FFTW_MEASURE's
    meaning: the plan will run many times); 0 (default) plans at once on the runtime-geometry kernels"""
    (lib or _lib.load()).dspfft_set_plan_effort(int(effort))


class Plan:
    """dtype "f32" (default; the fftwf_ API, COEFF_PRECISION=F) or "f64" (the fftw_ API of spec's, zoom's and
    applybasis's default build, include/precision.h:50-53): buffers, arithmetic and fused scales in that type."""

    def __init__(self, handle, lib, f64=False):
        self._h = handle
        self._lib = lib
        self.f64 = f64

    @classmethod
    def many_r2r(cls, n, kinds, howmany=1, inembed=None, istride=1, idist=0, onembed=None, ostride=1, odist=0, lib=None, dtype="f32",
                 first_axis_first=False):
        """first_axis_first: run axis 0 first and the contiguous axis last (f32 only); the inverse half of
        `roundtrip` is created this way"""
        if dtype not in ("f32", "f64"):
            raise ValueError("dtype must be 'f32' or 'f64'")
        if first_axis_first and dtype != "f32":
            raise ValueError("first_axis_first is an f32 plan option")
        lib = lib or _lib.load()
        n = list(n)
        kinds = list(kinds)
        if len(kinds) != len(n):
            raise ValueError("one kind per transformed dimension")
        h = C.c_void_p()
        if first_axis_first:
            rc = lib.dspfft_plan_many_r2r_ordered(C.byref(h), len(n), _ia(n), howmany, _ia(inembed), istride, idist, _ia(onembed), ostride, odist, _ia(kinds), 1)
        else:
            make = lib.dspfft_plan_many_r2r_f64 if dtype == "f64" else lib.dspfft_plan_many_r2r
            rc = make(C.byref(h), len(n), _ia(n), howmany, _ia(inembed), istride, idist, _ia(onembed), ostride, odist, _ia(kinds))
        if rc:
            raise DspfftError(lib.dspfft_last_error().decode())
        return cls(h, lib, dtype == "f64")

    @classmethod
    def guru(cls, dims, howmany_dims, kinds, lib=None, dtype="f32", first_axis_first=False):
        """The shape of fftw_plan_guru_r2r: dims and howmany_dims are lists of (n, in_stride, out_stride) in elements.  One plan for
        e.g. every 8x8x8 block of a volume (motion --blocksize 8x8x8).  first_axis_first: many_r2r's (f32 only)."""
        if first_axis_first and dtype != "f32":
            raise ValueError("first_axis_first is an f32 plan option")
        lib = lib or _lib.load()
        def arr(d):
            a = (_lib.IoDim * max(1, len(d)))()
            for i, (n, is_, os_) in enumerate(d):
                a[i].n, a[i].is_, a[i].os = int(n), int(is_), int(os_)
            return a
        h = C.c_void_p()
        if first_axis_first:
            rc = lib.dspfft_plan_guru_r2r_ordered(C.byref(h), len(dims), arr(dims), len(howmany_dims), arr(howmany_dims), _ia(list(kinds)), 1)
        else:
            rc = lib.dspfft_plan_guru_r2r(C.byref(h), len(dims), arr(dims), len(howmany_dims), arr(howmany_dims), _ia(list(kinds)), 1 if dtype == "f64" else 0)
        if rc:
            raise DspfftError(lib.dspfft_last_error().decode())
        return cls(h, lib, dtype == "f64")

    @classmethod
    def r2r_2d(cls, n0, n1, kind0, kind1, lib=None):
        lib = lib or _lib.load()
        h = C.c_void_p()
        if lib.dspfft_plan_r2r_2d(C.byref(h), n0, n1, kind0, kind1):
            raise DspfftError(lib.dspfft_last_error().decode())
        return cls(h, lib)

    @classmethod
    def image(cls, h, w, c, kind, lib=None, dtype="f32"):
        """The image tools' plan: rank 2 {h,w}, howmany=c, stride=c, dist=1 (interleaved HWC)."""
        return cls.many_r2r([h, w], [kind, kind], howmany=c, istride=c, idist=1, ostride=c, odist=1, lib=lib, dtype=dtype)

    def set_scale(self, scale):
        if self.f64:
            self._check(self._lib.dspfft_plan_set_scale_f64(self._h, scale))
        else:
            self._check(self._lib.dspfft_plan_set_scale(self._h, scale))
        return self

    def set_axis_scale0(self, axis, in_scale0=1.0, out_scale0=1.0):
        if self.f64:
            self._check(self._lib.dspfft_plan_set_axis_scale0_f64(self._h, axis, in_scale0, out_scale0))
        else:
            self._check(self._lib.dspfft_plan_set_axis_scale0(self._h, axis, in_scale0, out_scale0))
        return self

    def set_u8_trc(self, trc):
        """dspfft_plan_set_u8_trc (motion --linear on 8-bit video): this plan decodes at its 8-bit load as the forward plan of a roundtrip_u8*
        call and encodes at its 8-bit store as the inverse plan.  trc: a name or an id (trc_id); 0 / None / "none" resets."""
        self._check(self._lib.dspfft_plan_set_u8_trc(self._h, trc_id(trc, self._lib)))
        return self

    def set_input_window(self, axis, lo, hi):
        """promise that input samples of `axis` outside [lo, hi) are zero; True when the plan then skips reading (and needing) them"""
        rc = self._lib.dspfft_plan_set_input_window(self._h, axis, lo, hi)
        if rc < 0:
            raise DspfftError(self._lib.dspfft_last_error().decode())
        return bool(rc)

    def set_input_modulation(self, axis, d_mul, reversed_from=0):
        """dspfft_plan_set_input_modulation (on top of an input window): True when honoured"""
        rc = self._lib.dspfft_plan_set_input_modulation(self._h, axis, d_mul or None, int(reversed_from))
        if rc < 0:
            raise DspfftError(self._lib.dspfft_last_error().decode())
        return rc == 1

    def set_output_alternate(self, axis, on=True):
        """output sample j of `axis` times (-1)^j, fused into that axis's pass; True when the plan honours it"""
        rc = self._lib.dspfft_plan_set_output_alternate(self._h, axis, int(on))
        if rc < 0:
            raise DspfftError(self._lib.dspfft_last_error().decode())
        return bool(rc)

    def execute(self, d_in, d_out=None, stream=0):
        d_out = d_in if d_out is None else d_out
        run = self._lib.dspfft_execute_f64 if self.f64 else self._lib.dspfft_execute
        self._check(run(self._h, C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(stream)))

    @property
    def num_passes(self):
        return int(self._lib.dspfft_plan_num_passes(self._h))

    def execute_pass(self, index, d_in, d_out=None, stream=0):
        d_out = d_in if d_out is None else d_out
        self._check(self._lib.dspfft_execute_pass(self._h, index, C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(stream)))

    def execute_masked_accumulate(self, d_in, d_work, d_acc, d_ids=0, frame_id=0, elems_per_id=1, stream=0):
        """scan/scan.c:429-459 fused: d_acc += plan(d_in where ids == frame_id)"""
        run = self._lib.dspfft_execute_masked_accumulate_f64 if self.f64 else self._lib.dspfft_execute_masked_accumulate
        self._check(run(
            self._h, C.c_void_p(d_in), C.c_void_p(d_work), C.c_void_p(d_acc), C.c_void_p(d_ids or None), frame_id, elems_per_id, C.c_void_p(stream)))

    def execute_masked_accumulate_range(self, d_in, d_work, d_acc, d_ids, lo, hi, elems_per_id=1, stream=0):
        """d_acc += plan(d_in where lo <= ids < hi) (dspfft_execute_masked_accumulate_range): the id 0xFFFFFFFF (DC, unowned) is never
        selected; hi <= lo adds nothing"""
        run = self._lib.dspfft_execute_masked_accumulate_range_f64 if self.f64 else self._lib.dspfft_execute_masked_accumulate_range
        self._check(run(self._h, C.c_void_p(d_in), C.c_void_p(d_work), C.c_void_p(d_acc), C.c_void_p(d_ids), int(lo), int(hi), elems_per_id,
                        C.c_void_p(stream)))

    def execute_sum2(self, other, d_in, d_in_other, d_out, stream=0):
        """d_out = self(d_in) + other(d_in_other) (dspfft_execute_sum2: one launch for two one-axis row REDFT01 plans on the same kernel)"""
        self._check(self._lib.dspfft_execute_sum2(self._h, other._h, d_in, d_in_other, d_out, stream or None))

    def scan_prepare(self, d_ids=0, elems_per_id=1, stream=0):
        """owner ids that stay the same over a scan's frames: record each column tile's id range so that the fused step skips a tile
        outside the frame without reading its ids (dspfft_plan_scan_prepare); d_ids = 0 forgets"""
        self._check(self._lib.dspfft_plan_scan_prepare(self._h, C.c_void_p(d_ids or None), elems_per_id, C.c_void_p(stream)))
        return self

    @staticmethod
    def _filter_params(filter):
        if filter is None:
            return None
        fp = _lib.MotionFilterParams()
        fp.active = (C.c_int * 3)(*filter["active"]); fp.minbuf_hw = (C.c_int * 2)(*filter["minbuf_hw"]); fp.block_depth = int(filter["block_depth"])
        fp.band_begin = (C.c_int * 3)(*filter["band_begin"]); fp.band_end = (C.c_int * 3)(*filter["band_end"])
        fp.damp = filter.get("damp", 1.0); fp.boost = filter.get("boost", 1.0)
        fp.threshold_lo = filter.get("threshold_lo", 0.0); fp.threshold_hi = filter.get("threshold_hi", 0.0)
        fp.preserve_dc = filter.get("preserve_dc", 0); fp.grey_add = filter.get("grey_add", 0.0); fp.quantizer = filter.get("quantizer", 0.0)
        return fp

    @classmethod
    def _tail(cls, filter, d_coded, stream, *between):
        """the trailing arguments of a roundtrip or spectrogram entry: (fp, *between, d_coeffs_coded, stream); the by-reference fp keeps its
        structure alive"""
        fp = cls._filter_params(filter)
        return (C.byref(fp) if fp is not None else None,) + between + (C.c_void_p(d_coded or None), C.c_void_p(stream))

    def _topn_work(self, inv, topn_work):
        """(pointer, bytes) of the selection's scratch: the caller's uint8 device tensor, or one allocated here when the plans need any"""
        if topn_work is None:
            need = int(self._lib.dspfft_roundtrip_topn_work_bytes(self._h, inv._h))
            if not need:
                return None, 0, None
            import torch
            topn_work = torch.empty(need, dtype=torch.uint8, device="cuda")
        return C.c_void_p(topn_work.data_ptr()), topn_work.numel() * topn_work.element_size(), topn_work

    def roundtrip(self, inv, d_in, d_out=None, filter=None, d_coded=0, stream=0, coeff_limit=0, topn_work=None):
        """motion/motion.c:641-753: self (REDFT10) -> filter -> inv (REDFT01, created with first_axis_first=True), the middle axis
        fused into one launch when both plans have a specialised column kernel.  filter: dict with the fields of
        dspfft_motion_filter_params, or None.  coeff_limit: motion --coeff-limit, the coefficients kept per block ahead of the filter
        (dspfft_execute_roundtrip_topn; 0: none); topn_work: a uint8 device tensor of dspfft_roundtrip_topn_work_bytes, allocated per
        call when None and the plans need one."""
        d_out = d_in if d_out is None else d_out
        if not coeff_limit:
            self._check(self._lib.dspfft_execute_roundtrip(self._h, inv._h, C.c_void_p(d_in), C.c_void_p(d_out), *self._tail(filter, d_coded, stream)))
            return
        wp, wb, _hold = self._topn_work(inv, topn_work)
        self._check(self._lib.dspfft_execute_roundtrip_topn(self._h, inv._h, C.c_void_p(d_in), C.c_void_p(d_out),
                                                            *self._tail(filter, d_coded, stream, int(coeff_limit), wp, wb)))

    def roundtrip_u8(self, inv, d_in_u8, d_out_u8, d_work, out_mul, filter=None, d_coded=0, stream=0, coeff_limit=0, topn_work=None):
        """the same with motion's 8-bit samples at both ends (motion.c:617-640, :760-776): u8 in, float work buffer, u8 out =
        quantise(value * out_mul); the conversions ride on the first and last row passes when those are planar specialised passes.
        coeff_limit, topn_work: as roundtrip's (dspfft_execute_roundtrip_u8_topn).  d_work may be None / 0 for a rescaled block grid
        (motion_grid_plans: one kernel from the input volume to the output volume, no float intermediate) and for blocks along time
        (motion_temporal_plans, likewise); every other pair needs it."""
        if not coeff_limit:
            self._check(self._lib.dspfft_execute_roundtrip_u8(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), C.c_void_p(d_work), out_mul,
                                                              *self._tail(filter, d_coded, stream)))
            return
        wp, wb, _hold = self._topn_work(inv, topn_work)
        self._check(self._lib.dspfft_execute_roundtrip_u8_topn(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), C.c_void_p(d_work), out_mul,
                                                               *self._tail(filter, d_coded, stream, int(coeff_limit), wp, wb)))

    def _coeff_limit(self, inv, coeff_limit, outside_mul=1.0, topn_work=None, work=True):
        """dspfft_coeff_limit for a call (and what keeps its work buffer alive); work=False: the call needs no work buffer"""
        wp, wb, hold = self._topn_work(inv, topn_work) if work else (None, 0, None)
        cl = _lib.CoeffLimit()
        cl.keep = int(coeff_limit); cl.outside_mul = float(outside_mul); cl.d_work = wp.value if wp is not None else None; cl.work_bytes = wb
        return cl, hold

    def roundtrip_limit(self, inv, d_in, d_out=None, coeff_limit=0, outside_mul=1.0, filter=None, d_coded=0, stream=0, topn_work=None):
        """roundtrip with motion --coeff-limit through dspfft_execute_roundtrip_limit: every pair roundtrip(coeff_limit=...) takes, the same
        bytes, and a rescaled block grid (motion_grid_plans; outside_mul = info["limit_outside_mul"]), whose selection ranks the whole
        max(block, scaled) embedding as the reference does.  coeff_limit must be at least 1."""
        d_out = d_in if d_out is None else d_out
        cl, _hold = self._coeff_limit(inv, coeff_limit, outside_mul, topn_work)
        self._check(self._lib.dspfft_execute_roundtrip_limit(self._h, inv._h, C.c_void_p(d_in), C.c_void_p(d_out), *self._tail(filter, d_coded, stream, C.byref(cl))))

    def roundtrip_u8_limit(self, inv, d_in_u8, d_out_u8, d_work, out_mul, coeff_limit=0, outside_mul=1.0, filter=None, d_coded=0, stream=0, topn_work=None):
        """roundtrip_u8 with motion --coeff-limit through dspfft_execute_roundtrip_u8_limit (see roundtrip_limit); d_work may be None / 0 for
        a rescaled block grid"""
        cl, _hold = self._coeff_limit(inv, coeff_limit, outside_mul, topn_work)
        self._check(self._lib.dspfft_execute_roundtrip_u8_limit(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), C.c_void_p(d_work), out_mul,
                                                                *self._tail(filter, d_coded, stream, C.byref(cl))))

    def roundtrip_u8_packed(self, inv, d_in_u8, d_out_u8, out_mul, packed, filter=None, coeff_limit=0, d_coded=0, stream=0):
        """dspfft_execute_roundtrip_u8_packed: the fused small-block roundtrip on packed 8-bit pixels (rgb24, rgba ...).  self / inv: the planar
        small-block pair (motion_grid_plans(shape, block, block)), planned over the clip in pixels; the buffers hold packed.components bytes per
        pixel.  packed: motion_packed(...) -- its damp, boost and grey_add (by byte position) replace the filter's; filter: as roundtrip_u8's,
        or None.  coeff_limit: motion --coeff-limit per component block (0: none).  Needs no work buffer; may run in place."""
        cl = self._coeff_limit(inv, coeff_limit, work=False)[0] if coeff_limit else None
        between = (C.byref(packed) if packed is not None else None, C.byref(cl) if cl is not None else None)
        self._check(self._lib.dspfft_execute_roundtrip_u8_packed(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), float(out_mul),
                                                                 *self._tail(filter, d_coded, stream, *between)))

    def roundtrip_u8_packed_rescale(self, inv, d_in_u8, d_out_u8, out_mul, packed, filter=None, d_coded=0, stream=0, coeff_limit=0, outside_mul=1.0):
        """dspfft_execute_roundtrip_u8_packed_rescale: motion -b with -s over a block grid on packed 8-bit pixels (rgb24, rgba ...), one launch.
        self / inv: the planar grid pair motion_grid_plans(shape, block, scaled) with scaled != block, planned over the clips in pixels; d_in_u8
        holds info["in_shape"] and d_out_u8 info["out_shape"] pixels of packed.components bytes, and the two must not overlap.  out_mul:
        info["out_mul"].  packed: motion_packed(..., normalization=info["normalization"], scalefactor=info["scalefactor"]) -- its damp, boost
        and grey_add (by byte position) replace the filter's; filter: the planar grid call's (active = info["active"], minbuf_hw and block_depth
        of the embedding), or None.  Needs no work buffer.  coeff_limit: motion --coeff-limit per component block over the whole embedding
        (dspfft_execute_roundtrip_u8_packed_rescale_limit; 0: none) with outside_mul = info["limit_outside_mul"]; the bytes are
        roundtrip_u8_limit's on each component's plane."""
        pk = C.byref(packed) if packed is not None else None
        if coeff_limit:
            cl = self._coeff_limit(inv, coeff_limit, outside_mul, work=False)[0]
            self._check(self._lib.dspfft_execute_roundtrip_u8_packed_rescale_limit(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), float(out_mul),
                                                                                   *self._tail(filter, d_coded, stream, pk, C.byref(cl))))
            return
        self._check(self._lib.dspfft_execute_roundtrip_u8_packed_rescale(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), float(out_mul),
                                                                         *self._tail(filter, d_coded, stream, pk)))

    def roundtrip_u8_packed_rescale_dither(self, inv, d_in_u8, d_out_u8, scalefactor, normalization, packed, filter=None, coeff_limit=0, outside_mul=1.0,
                                           d_coded=0, stream=0):
        """dspfft_execute_roundtrip_u8_packed_rescale_dither: roundtrip_u8_packed_rescale with motion's -d, one launch -- the Floyd-Steinberg store
        runs in the kernel's LDS tile, over the planes of `scaled`.  Arguments as roundtrip_u8_packed_rescale's, with info["scalefactor"] and
        info["normalization"] in place of out_mul.  The bytes are roundtrip_u8_dither's (with coeff_limit and outside_mul: its limit twin's) on
        each component's plane.  Needs no work buffer; out of place."""
        cl = self._coeff_limit(inv, coeff_limit, outside_mul, work=False)[0] if coeff_limit else None
        between = (C.byref(packed) if packed is not None else None, C.byref(cl) if cl is not None else None)
        self._check(self._lib.dspfft_execute_roundtrip_u8_packed_rescale_dither(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), float(scalefactor),
                                                                                float(normalization), *self._tail(filter, d_coded, stream, *between)))

    def roundtrip_u8_packed_frames(self, inv, d_in_u8, d_out_u8, d_work, out_mul, packed, filter=None, d_coded=0, stream=0):
        """dspfft_execute_roundtrip_u8_packed_frames: motion's default block 0x0x1 on packed 8-bit pixels (rgb24, rgba ...) -- every component of
        every frame one block.  self / inv: motion_packed_frame_plans(frames, h, w, components); d_work: frames * h * w * components floats;
        out_mul: info["out_mul"].  packed: motion_packed(...) -- its damp, boost and grey_add (by byte position) replace the filter's; filter:
        as roundtrip_u8's (active, minbuf_hw and block_depth are the call's own: (1, h, w), (h, w), 1), or None.  May run in place."""
        pk = C.byref(packed) if packed is not None else None
        self._check(self._lib.dspfft_execute_roundtrip_u8_packed_frames(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), C.c_void_p(d_work or None),
                                                                        float(out_mul), *self._tail(filter, d_coded, stream, pk)))

    def roundtrip_u8_packed_dither(self, inv, d_in_u8, d_out_u8, scalefactor, normalization, packed, filter=None, coeff_limit=0, d_coded=0, stream=0):
        """dspfft_execute_roundtrip_u8_packed_dither: roundtrip_u8_packed with motion's -d, one launch -- the Floyd-Steinberg store runs in the
        kernel's LDS tile.  Arguments as roundtrip_u8_packed's, with info["scalefactor"] and info["normalization"] in place of out_mul.  The
        bytes are roundtrip_u8_dither's on each component's plane.  Needs no work buffer; may run in place."""
        cl = self._coeff_limit(inv, coeff_limit, work=False)[0] if coeff_limit else None
        between = (C.byref(packed) if packed is not None else None, C.byref(cl) if cl is not None else None)
        self._check(self._lib.dspfft_execute_roundtrip_u8_packed_dither(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), float(scalefactor),
                                                                        float(normalization), *self._tail(filter, d_coded, stream, *between)))

    def roundtrip_u8_packed_frames_dither(self, inv, d_in_u8, d_out_u8, d_work, scalefactor, normalization, packed, filter=None, d_coded=0, stream=0):
        """dspfft_execute_roundtrip_u8_packed_frames_dither: roundtrip_u8_packed_frames with motion's -d -- the inverse ends as floats in
        d_work (which keeps them) and motion_dither_u8_packed's kernels store the bytes.  Arguments as roundtrip_u8_packed_frames's, with
        info["scalefactor"] and info["normalization"] in place of out_mul.  May run in place."""
        pk = C.byref(packed) if packed is not None else None
        self._check(self._lib.dspfft_execute_roundtrip_u8_packed_frames_dither(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), C.c_void_p(d_work or None),
                                                                               float(scalefactor), float(normalization), *self._tail(filter, d_coded, stream, pk)))

    def roundtrip_u8_dither(self, inv, d_in_u8, d_out_u8, d_work, scalefactor, normalization, filter=None, d_coded=0, stream=0,
                            coeff_limit=0, outside_mul=1.0, topn_work=None):
        """roundtrip_u8 with motion's -d (motion.c:756-788): the last inverse pass leaves floats in d_work and the bytes are the
        Floyd-Steinberg dithered store of them (pel = value * scalefactor * normalization * normalization), plane by plane over inv's extents.
        coeff_limit (0: none), outside_mul, topn_work: motion --coeff-limit as roundtrip_limit's (dspfft_execute_roundtrip_u8_dither_limit)"""
        if coeff_limit:
            cl, _hold = self._coeff_limit(inv, coeff_limit, outside_mul, topn_work)
            self._check(self._lib.dspfft_execute_roundtrip_u8_dither_limit(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), C.c_void_p(d_work),
                                                                           float(scalefactor), float(normalization), *self._tail(filter, d_coded, stream, C.byref(cl))))
            return
        self._check(self._lib.dspfft_execute_roundtrip_u8_dither(self._h, inv._h, C.c_void_p(d_in_u8), C.c_void_p(d_out_u8), C.c_void_p(d_work),
                                                                 float(scalefactor), float(normalization), *self._tail(filter, d_coded, stream)))

    def spectrogram(self, d_in, d_out, mode, scalefactor, normalization, c=None, d_work=0, filter=None, d_coded=0, stream=0, pixels="u8"):
        """motion --spectrogram (dspfft_execute_spectrogram_u8 / _f32): load -> self (REDFT10 with motion's index-0 factors) -> filter ->
        encode -> store, one kernel for a small-block plan, the plan's passes and one kernel over all blocks otherwise (d_work needed).
        mode: "abs", "shift", "flat" or "copy" (or DSPFFT_MOTION_*).  c: shift's constant (motion.c:568; motion_spec_constants gives it),
        None for the other modes -- abs derives its own per block on the device.  pixels: "u8", or "f32" for motion's float pixels."""
        sp = _spec_params(mode, scalefactor, normalization, c)
        run = {"u8": self._lib.dspfft_execute_spectrogram_u8, "f32": self._lib.dspfft_execute_spectrogram_f32}[pixels]
        self._check(run(self._h, C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(d_work or None), C.byref(sp), *self._tail(filter, d_coded, stream)))

    def ispectrogram(self, d_in, d_out, mode, scalefactor, normalization, c=None, d_work=0, filter=None, d_coded=0, stream=0, pixels="u8", out_mul=None):
        """motion --ispectrogram (dspfft_execute_ispectrogram_u8 / _f32): load -> decode -> filter -> self (REDFT01 with motion.c:751's
        factors and the global scale) -> store.  mode: "shift", "flat" or "copy"; c: shift's ic (motion.c:569).  out_mul: roundtrip_u8's,
        scalefactor normalization^2 by default."""
        sp = _spec_params(mode, scalefactor, normalization, c)
        mul = float(scalefactor) * float(normalization) ** 2 if out_mul is None else float(out_mul)
        run = {"u8": self._lib.dspfft_execute_ispectrogram_u8, "f32": self._lib.dspfft_execute_ispectrogram_f32}[pixels]
        self._check(run(self._h, C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(d_work or None), C.byref(sp), *self._tail(filter, d_coded, stream, mul)))

    def spectrogram_packed(self, d_in, d_out, mode, scalefactor, normalization, packed, c=None, d_work=0, filter=None, d_coded=0, stream=0):
        """motion --spectrogram on packed 8-bit pixels (dspfft_execute_spectrogram_u8_packed): spectrogram's call with packed.components
        bytes per pixel in d_in and d_out, every component of every block a block of its own.  self: the planar small-block forward plan
        over the clip in pixels (motion_grid_plans(shape, block, block): one kernel, no d_work), or the interleaved full-frame forward plan
        (motion_packed_frame_plans: d_work of frames * h * w * components floats).  packed: motion_packed(...) -- its damp, boost and
        grey_add (by byte position) replace the filter's."""
        sp = _spec_params(mode, scalefactor, normalization, c)
        pk = C.byref(packed) if packed is not None else None
        self._check(self._lib.dspfft_execute_spectrogram_u8_packed(self._h, C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(d_work or None), C.byref(sp),
                                                                   *self._tail(filter, d_coded, stream, pk)))

    def ispectrogram_packed(self, d_in, d_out, mode, scalefactor, normalization, packed, c=None, d_work=0, filter=None, d_coded=0, stream=0, out_mul=None):
        """motion --ispectrogram on packed 8-bit pixels (dspfft_execute_ispectrogram_u8_packed): ispectrogram's call, arguments as
        spectrogram_packed's; self is the inverse plan of the same helpers."""
        sp = _spec_params(mode, scalefactor, normalization, c)
        mul = float(scalefactor) * float(normalization) ** 2 if out_mul is None else float(out_mul)
        pk = C.byref(packed) if packed is not None else None
        self._check(self._lib.dspfft_execute_ispectrogram_u8_packed(self._h, C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(d_work or None), C.byref(sp),
                                                                    *self._tail(filter, d_coded, stream, pk, mul)))

    def spec_u8(self, d_in, d_out, d_work, params, d_signmap=0, d_dc=0, stream=0):
        """spec on an 8-bit image in device memory (dspfft_execute_spec_u8): bytes -> self (the forward plan of spec_image_plans) -> display
        encoding -> bytes, in three sweeps.  params: spec_image_params(...).  d_signmap (abs only): also the `sign` preset's image, what
        ispec -m reads; d_dc: `channels` doubles on the device, the header's DC values."""
        self._check(self._lib.dspfft_execute_spec_u8(self._h, C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(d_signmap or None), C.c_void_p(d_work or None),
                                                     C.c_void_p(d_dc or None), C.byref(params), C.c_void_p(stream)))

    def ispec_u8(self, d_in, d_out, d_work, params, d_signmap=0, dc=None, restore_dc=False, stream=0):
        """ispec on an 8-bit spectrogram in device memory (dspfft_execute_ispec_u8): bytes (+ sign map) -> decoding -> self (the inverse
        plan of spec_image_plans) -> bytes.  dc: the header's DC values (host floats), needed for range dc / dcs and for restore_dc."""
        dcp = None if dc is None else (C.c_double * len(dc))(*[float(v) for v in dc])
        self._check(self._lib.dspfft_execute_ispec_u8(self._h, C.c_void_p(d_in), C.c_void_p(d_signmap or None), C.c_void_p(d_out), C.c_void_p(d_work or None),
                                                      dcp, int(bool(restore_dc)), C.byref(params), C.c_void_p(stream)))

    def describe(self):
        buf = C.create_string_buffer(4096)
        self._check(self._lib.dspfft_plan_describe(self._h, buf, len(buf)))
        return buf.value.decode()

    @property
    def algorithmic_bytes(self):
        return int(self._lib.dspfft_plan_algorithmic_bytes(self._h))

    def destroy(self):
        if self._h:
            self._lib.dspfft_destroy_plan(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise DspfftError(self._lib.dspfft_last_error().decode())


def motion_grid_plans(shape_dhw, block, scaled, lib=None):
    """motion --blocksize `block` --size `scaled` over a [D][H][W] volume (motion/motion.c:488-499,535-552,566-567): the plan pair of
    dspfft_execute_roundtrip* for the volume layout.  block, scaled: (d, h, w), every extent 4, 8 or 16, or d = 1 on both sides for 2-D blocks
    of up to 32 x 32.  fwd cuts the input volume (its pitches are shape_dhw's; W a multiple of 4) into whole blocks -- what is left over at
    the far ends is cropped, as the reference crops -- and inv cuts the dense output volume info["out_shape"] into as many blocks of
    `scaled`.  Both carry motion's scales (2 sqrt 2 and its inverse, the per-axis index-0 factors of the uniform range, :644-647,748-751;
    for 2-D blocks the unit axis of the reference's 3-D plans is folded into them).  info: in_shape (the cropped input extents), out_shape,
    nblocks, active = min(block, scaled) for the filter, scalefactor, normalization, out_mul = scalefactor normalization^2 (roundtrip_u8's),
    limit_outside_mul = roundtrip_limit's outside_mul for these plans (1 for 3-D blocks, 2 for 2-D blocks: the folded unit axis)."""
    import math
    D, H, W = (int(v) for v in shape_dhw)
    (bd, bh, bw), (sd, sh, sw) = (tuple(int(v) for v in t) for t in (block, scaled))
    if (bd == 1) != (sd == 1):
        raise ValueError("block and scaled must both be 2-D (depth 1) or both 3-D")
    if W % 4:
        raise ValueError("the row pitch W must be a multiple of 4")
    nd, nh, nw = D // bd, H // bh, W // bw
    if not (nd and nh and nw):
        raise ValueError("the volume holds no whole block")
    Do, Ho, Wo = nd * sd, nh * sh, nw * sw
    two_d = bd == 1
    r2 = math.sqrt(2.0)

    def plan(ext, vol, kind, scale):
        (ed, eh, ew), (_, vh, vw) = ext, vol
        dims = [(ed, vh * vw, vh * vw), (eh, vw, vw), (ew, 1, 1)][1 if two_d else 0:]
        how = [(nd, ed * vh * vw, ed * vh * vw), (nh, eh * vw, eh * vw), (nw, ew, ew)]
        return Plan.guru(dims, how, [kind] * len(dims), lib=lib).set_scale(scale)
    # (a unit axis of the reference's 3-D plans: REDFT10 doubles and the uniform range divides by sqrt 2; the inverse multiplies by sqrt 2)
    unit = r2 if two_d else 1.0
    fwd = plan((bd, bh, bw), (D, H, W), REDFT10, 2 * r2 * unit)
    inv = plan((sd, sh, sw), (Do, Ho, Wo), REDFT01, unit / (2 * r2))
    for a in range(2 if two_d else 3):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
        inv.set_axis_scale0(a, r2, 1.0)
    ns, nbk = float(sd * sh * sw), float(bd * bh * bw)
    scalefactor, normalization = ns / nbk, 1.0 / math.sqrt(ns * 8)
    info = dict(in_shape=(nd * bd, nh * bh, nw * bw), out_shape=(Do, Ho, Wo), nblocks=(nd, nh, nw),
                active=(min(bd, sd), min(bh, sh), min(bw, sw)), scalefactor=scalefactor, normalization=normalization,
                out_mul=scalefactor * normalization * normalization, limit_outside_mul=2.0 if two_d else 1.0)
    return fwd, inv, info


#: 8-bit packed pixel formats whose every byte is a component: the byte position of each component, in the reference's component order
#: (R, G, B[, A] or Y, A), as libavutil's pixel format descriptors place them
PACKED_FORMATS = {"rgb24": (0, 1, 2), "bgr24": (2, 1, 0), "rgba": (0, 1, 2, 3), "bgra": (2, 1, 0, 3), "argb": (1, 2, 3, 0), "abgr": (3, 2, 1, 0),
                  "ya8": (0, 1)}
_PACKED_PADDED = ("rgb0", "bgr0", "0rgb", "0bgr")


def motion_packed(pix_fmt, boost=None, damp=None, dcstop=False, normalization=1.0, scalefactor=1.0):
    """The dspfft_motion_packed of Plan.roundtrip_u8_packed for an 8-bit packed pixel format (PACKED_FORMATS).  boost / damp: motion's -B / -D,
    up to four values in the reference's component order (r:g:b:a), filled up by its rule (motion/motion.c:235-236: a missing entry repeats the
    one before it; none at all gives 1 for boost and 0 for damp).  grey_add[i] = (1 - (damp[i] if dcstop else boost[i])) 127.5 /
    (normalization^2 scalefactor) (:736; dcstop: the pass band does not begin at the origin).  All three are stored by BYTE POSITION.
    With a rescaled pair (Plan.roundtrip_u8_packed_rescale) normalization and scalefactor are motion_grid_plans' info["normalization"] and
    info["scalefactor"] (the latter is then not 1, :566), and the line gives the pair's grey_add as it stands.
    Formats with a byte that is no component (rgb0, 0rgb ...: the reference never writes it), gray (the planar call) and anything that is not
    8-bit are refused with a ValueError."""
    fmt = str(pix_fmt)
    if fmt in _PACKED_PADDED:
        raise ValueError(f"pixel format {fmt!r} has a padding byte that is no component: not a packed format of roundtrip_u8_packed")
    if fmt in ("gray", "gray8", "y8"):
        raise ValueError(f"pixel format {fmt!r} has one component: that is the planar call (roundtrip_u8)")
    if fmt not in PACKED_FORMATS:
        raise ValueError(f"pixel format {fmt!r} is not an 8-bit packed format with every byte a component (one of {', '.join(PACKED_FORMATS)})")
    pos = PACKED_FORMATS[fmt]

    def fill(v, first):
        v = [] if v is None else ([float(v)] if isinstance(v, (int, float)) else [float(x) for x in v])
        if len(v) > 4:
            raise ValueError("at most four values (r:g:b:a)")
        for i in range(len(v), 4):
            v.append(v[i - 1] if i else first)
        return v
    b, d = fill(boost, 1.0), fill(damp, 0.0)
    p = _lib.MotionPacked()
    p.components = len(pos)
    for i, at in enumerate(pos):
        p.boost[at], p.damp[at] = b[i], d[i]
        p.grey_add[at] = (1.0 - (d[i] if dcstop else b[i])) * 127.5 / (float(normalization) ** 2 * float(scalefactor))
    return p


def motion_packed_frame_plans(frames, h, w, components, lib=None):
    """motion's default block 0x0x1 (one full frame per block) over a clip of packed 8-bit pixels [frames][h][w][components]: the plan pair of
    Plan.spectrogram_packed / Plan.ispectrogram_packed.  Both are in place, dense and interleaved, of rank 2 with the batch levels
    {components: stride 1} and, for frames > 1, {frames: stride h w components}, and carry the scales motion_grid_plans gives 2-D blocks (the
    unit z axis of the reference's 3-D plans folded in, 1 / sqrt 2 out of and sqrt 2 into index 0); inv runs its row pass last.  info:
    scalefactor = 1, normalization, c and ic (motion_spec_constants((1, h, w))), out_mul = normalization^2."""
    import math
    F, h, w, comps = int(frames), int(h), int(w), int(components)
    r2 = math.sqrt(2.0)
    dims = [(h, w * comps, w * comps), (w, comps, comps)]
    how = [(comps, 1, 1)] + ([(F, h * w * comps, h * w * comps)] if F > 1 else [])
    unit = r2          # (motion_grid_plans: the unit axis of the reference's 3-D plans)
    fwd = Plan.guru(dims, how, [REDFT10, REDFT10], lib=lib).set_scale(2 * r2 * unit)
    inv = Plan.guru(dims, how, [REDFT01, REDFT01], lib=lib, first_axis_first=True).set_scale(unit / (2 * r2))
    for a in range(2):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
        inv.set_axis_scale0(a, r2, 1.0)
    k = motion_spec_constants((1, h, w))
    info = dict(scalefactor=1.0, normalization=k["normalization"], c=k["c"], ic=k["ic"], out_mul=k["normalization"] ** 2)
    return fwd, inv, info


def motion_temporal_plans(shape_dhw, block_d, scaled_d=None, lib=None):
    """motion --blocksize 1x1xD (--size 1x1xD') over a [D_total][H][W] plane (motion/README.md:87-89, motion/motion.c:488-499,535-552,
    566-567): every pixel of every run of D = block_d frames is a 1-D block, transformed over D, filtered by z and transformed back over
    D' = scaled_d (default D).  The plan pair of dspfft_execute_roundtrip*: fwd is a rank-1 REDFT10 of length D along the frame axis, at
    stride P = H W, batched over the nd = D_total // D blocks and the P pixels (P a multiple of 4; leftover frames are cropped, as the
    reference crops them); inv the REDFT01 of length D' over the dense output clip [nd D'][H][W].  Both carry motion's scales with the two
    unit axes of the reference's 3-D plans folded in, sqrt 2 each (:644-647,748-751).  info: in_shape (the cropped input), out_shape,
    nblocks, active = (min(D, D'), 1, 1), scalefactor = D' / D, normalization = 1 / sqrt(8 D'), out_mul = scalefactor normalization^2
    (roundtrip_u8's).  Filter dictionaries for these plans: active = info["active"], minbuf_hw = (1, 1), block_depth = max(D, D'), bands
    (z0, 0, 0) to (z1, 1, 1).  The 8-bit call runs in place for D' = D; with D' != D input and output must not overlap."""
    import math
    Dt, H, W = (int(v) for v in shape_dhw)
    D = int(block_d)
    S = D if scaled_d is None else int(scaled_d)
    P = H * W
    if D < 2 or S < 2:
        raise ValueError("block_d and scaled_d must be at least 2")
    if P < 4 or P % 4:
        raise ValueError("the samples per frame H * W must be a multiple of 4")
    nd = Dt // D
    if not nd:
        raise ValueError("the clip holds no whole block")
    r2 = math.sqrt(2.0)
    how = lambda n: [(nd, n * P, n * P), (P, 1, 1)]
    # (a unit axis of the reference's 3-D plans: REDFT10 doubles and the uniform range divides by sqrt 2; the inverse multiplies by sqrt 2)
    unit = r2
    fwd = Plan.guru([(D, P, P)], how(D), [REDFT10], lib=lib).set_scale(2 * r2 * unit * unit).set_axis_scale0(0, 1.0, 1.0 / r2)
    inv = Plan.guru([(S, P, P)], how(S), [REDFT01], lib=lib).set_scale(unit * unit / (2 * r2)).set_axis_scale0(0, r2, 1.0)
    scalefactor, normalization = S / D, 1.0 / math.sqrt(S * 8.0)
    info = dict(in_shape=(nd * D, H, W), out_shape=(nd * S, H, W), nblocks=(nd, H, W), active=(min(D, S), 1, 1), scalefactor=scalefactor,
                normalization=normalization, out_mul=scalefactor * normalization * normalization)
    return fwd, inv, info


def motion_dither_u8(d_pix, d_coeffs, n, row_pitch=None, plane_pitch=None, nblocks=(1, 1, 1), block_step=(0, 0, 0), scalefactor=1.0,
                     normalization=1.0, stream=0, lib=None, trc=0):
    """dspfft_motion_dither_u8: motion.c:756-788 with -d over the {d, h, w} = n planes of every block (element (b, z, y, x) at
    sum(b_i block_step_i) + z plane_pitch + y row_pitch + x in both buffers); d_coeffs is only read.  trc (a name or an id; 0: none):
    motion --linear, the bytes are the encoded ones (dspfft_motion_dither_u8_trc)"""
    lib = lib or _lib.load()
    trc = trc_id(trc, lib)
    n = [int(v) for v in n]
    g = _lib.DitherGeom()
    g.n[:] = n
    g.row_pitch = n[2] if row_pitch is None else int(row_pitch)
    g.plane_pitch = n[1] * g.row_pitch if plane_pitch is None else int(plane_pitch)
    g.nblocks[:] = [int(v) for v in nblocks]
    g.block_step[:] = [int(v) for v in block_step]
    if trc:
        rc = lib.dspfft_motion_dither_u8_trc(C.c_void_p(d_pix), C.c_void_p(d_coeffs), C.byref(g), float(scalefactor), float(normalization), trc, C.c_void_p(stream))
    else:
        rc = lib.dspfft_motion_dither_u8(C.c_void_p(d_pix), C.c_void_p(d_coeffs), C.byref(g), float(scalefactor), float(normalization), C.c_void_p(stream))
    if rc:
        raise DspfftError(lib.dspfft_motion_last_error().decode())


def motion_dither_u8_packed(d_pix, d_coeffs, n, components, row_pitch=None, plane_pitch=None, nblocks=(1, 1, 1), block_step=(0, 0, 0), scalefactor=1.0,
                            normalization=1.0, stream=0, lib=None, trc=0):
    """dspfft_motion_dither_u8_packed: motion_dither_u8 over buffers of `components` values per pixel, every component a plane of its own.
    n, the pitches and the block steps count PIXELS, as motion_dither_u8's; the element of component c is at components * (pixel offset) + c."""
    lib = lib or _lib.load()
    n = [int(v) for v in n]
    g = _lib.DitherGeom()
    g.n[:] = n
    g.row_pitch = n[2] if row_pitch is None else int(row_pitch)
    g.plane_pitch = n[1] * g.row_pitch if plane_pitch is None else int(plane_pitch)
    g.nblocks[:] = [int(v) for v in nblocks]
    g.block_step[:] = [int(v) for v in block_step]
    if lib.dspfft_motion_dither_u8_packed(C.c_void_p(d_pix), C.c_void_p(d_coeffs), C.byref(g), int(components), float(scalefactor), float(normalization),
                                          trc_id(trc, lib), C.c_void_p(stream)):
        raise DspfftError(lib.dspfft_last_error().decode())


def motion_topn_blocks(t, count, keep, stride=None, stream=None, lib=None):
    """dspfft_motion_topn_blocks in place on a contiguous float32 device tensor: motion --coeff-limit in each of its runs of `count` floats,
    `stride` floats apart (default: count, the runs back to back); what lies between the runs stays.  Returns t."""
    lib = lib or _lib.load()
    import torch
    count, keep = int(count), int(keep)
    stride = count if stride is None else int(stride)
    assert t.is_contiguous() and t.element_size() == 4 and count >= 1 and stride >= count
    nblocks = (t.numel() - count) // stride + 1
    assert nblocks >= 1
    need = int(lib.dspfft_motion_topn_blocks_work_bytes(count, nblocks))
    work = torch.empty(need, dtype=torch.uint8, device=t.device) if need else None
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    if lib.dspfft_motion_topn_blocks(C.c_void_p(t.data_ptr()), count, nblocks, stride, keep, _ptr(work), need, C.c_void_p(stream)):
        raise DspfftError(lib.dspfft_motion_last_error().decode())
    return t


def trc_id(trc, lib=None):
    """a transfer characteristic given by av_color_transfer_name's name or by its AVColorTransferCharacteristic id -> the id; 0 / None /
    "none": no function.  Raises for one that is unknown or not built."""
    lib = lib or _lib.load()
    if trc is None or trc == 0 or trc == "none":
        return 0
    v = lib.dspfft_trc_from_name(trc.encode()) if isinstance(trc, str) else (int(trc) if lib.dspfft_trc_name(int(trc)) else -1)
    if v < 0:
        raise DspfftError(f"transfer characteristic {trc!r} is unknown or not built")
    return v


def trc_apply(t, trc, inverse=False, out=None, stream=None, lib=None):
    """dspfft_trc_apply_f32 over a contiguous float32 device tensor: encode (linear light -> coded), or decode with inverse=True (the
    input side of scan -g / zoom -g).  out: a tensor of the same size (t itself for in place); a new one by default."""
    lib = lib or _lib.load()
    trc = trc_id(trc, lib)
    if out is None:
        out = t.new_empty(t.shape)
    assert t.is_contiguous() and out.is_contiguous() and t.numel() == out.numel() and t.element_size() == 4 and out.element_size() == 4
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    if trc == 0:
        if out.data_ptr() != t.data_ptr():
            out.copy_(t)
        return out
    if lib.dspfft_trc_apply_f32(C.c_void_p(out.data_ptr()), C.c_void_p(t.data_ptr()), t.numel(), trc, int(bool(inverse)), C.c_void_p(stream)):
        raise DspfftError(lib.dspfft_last_error().decode())
    return out


_MOTION_MODES = {"none": 0, "abs": 1, "shift": 2, "flat": 3, "copy": 4}


def _spec_params(mode, scalefactor, normalization, c=None):
    m = _MOTION_MODES[mode] if isinstance(mode, str) else int(mode)
    return _lib.MotionSpecParams(m, float(scalefactor), float(normalization), 0.0 if c is None else float(c))


def spec_image_plans(h, w, c, lib=None):
    """The plan pair of Plan.spec_u8 / Plan.ispec_u8 for an h x w image of c interleaved channels: REDFT10 with spec.c:70-78's normalisation
    of (float)byte (scale 1 / (255 * 2wh), 1 / sqrt 2 at index 0 of both axes) and REDFT01, row pass last, with ispec.c:153-159's factors."""
    import math
    r2 = math.sqrt(2.0)
    fwd = Plan.image(h, w, c, REDFT10, lib=lib).set_scale(1.0 / (255.0 * 2.0 * w * h))
    inv = Plan.many_r2r([h, w], [REDFT01, REDFT01], howmany=c, istride=c, idist=1, ostride=c, odist=1, lib=lib, first_axis_first=True).set_scale(0.5)
    for a in range(2):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
        inv.set_axis_scale0(a, r2, 1.0)
    return fwd, inv


SPEC_IMAGE_RANGES = {"one": 0, "dc": 1, "dcs": 2}
SPEC_IMAGE_SCALES = {"log": 0, "linear": 1}
SPEC_IMAGE_SIGNS = {"abs": 0, "shift": 1, "saturate": 2, "retain": 3}
#: spec -t (spec/spec.h:71-79): scale, sign, gain, range
SPEC_IMAGE_PRESETS = {"abs": ("log", "abs", "native", "dc"), "shift": ("log", "shift", "native", "one"), "flat": ("linear", "shift", "custom", "one"),
                      "sign": ("linear", "saturate", "custom", "one"), "copy": ("linear", "retain", "custom", "one")}


def spec_image_params(h, w, preset="abs", range=None, scale=None, sign=None, gain=None):
    """dspfft_spec_image_params from spec's options: preset is -t, and range (-R), scale (-T), sign (-S) and gain (-G: "native" =
    127.5 sqrt(4wh), "reference" = 127.5 * 1024, or a number; a preset's "custom" is 1) replace what it sets."""
    import math
    sc, sg, gn, rg = SPEC_IMAGE_PRESETS[preset]
    rg, sc, sg = range or rg, scale or sc, sign or sg
    gn = gn if gain is None else gain
    if gn == "native":
        g = 127.5 * math.sqrt(w * h * 4)
    elif gn == "reference":
        g = 127.5 * 1024
    elif gn == "custom":
        g = 1.0
    else:
        g = float(gn)
    return _lib.SpecImageParams(g, SPEC_IMAGE_RANGES[rg], SPEC_IMAGE_SCALES[sc], SPEC_IMAGE_SIGNS[sg])


def motion_spec_constants(block, scaled=None):
    """motion.c:566-569 for blocks of `block` = (d, h, w) stored as `scaled` (default: block): scalefactor, normalization, and the shift
    types' constants c (--spectrogram=shift) and ic (--ispectrogram=shift), which are the same number"""
    import math
    scaled = block if scaled is None else scaled
    nb, ns = float(block[0] * block[1] * block[2]), float(scaled[0] * scaled[1] * scaled[2])
    scalefactor, normalization = ns / nb, 1.0 / math.sqrt(ns * 8)
    c = 127.5 / math.log1p(ns * normalization * 255 * 8)
    return dict(scalefactor=scalefactor, normalization=normalization, c=c, ic=c)


def _spec_blocks(fn, d_a, d_b, n, minbuf_hw, nblocks, block_stride, mode, scalefactor, normalization, c, filter, d_coded, stream, lib):
    lib = lib or _lib.load()
    n = [int(v) for v in n]
    hw = (n[1], n[2]) if minbuf_hw is None else minbuf_hw
    stride = hw[0] * hw[1] * n[0] if block_stride is None else int(block_stride)
    sp = _spec_params(mode, scalefactor, normalization, c)
    if getattr(lib, fn)(_ptr(d_a), _ptr(d_b), _ia(n), _ia(hw), int(nblocks), stride, C.byref(sp), *Plan._tail(filter, d_coded, stream)):
        raise DspfftError(lib.dspfft_motion_last_error().decode())


def motion_spec_blocks(d_pix, d_coeffs, n, mode, scalefactor, normalization, c=None, minbuf_hw=None, nblocks=1, block_stride=None, filter=None,
                       d_coded=0, stream=0, pixels="u8", lib=None):
    """dspfft_motion_spec_blocks_u8 / _f32: filter, encode and store the `nblocks` blocks of n = (d, h, w) coefficients in d_coeffs (read
    only; planes of minbuf_hw, blocks block_stride apart: dense by default) as pixels in d_pix, the same layout.  abs takes every block's c
    from its own element 0."""
    _spec_blocks("dspfft_motion_spec_blocks_" + pixels, d_pix, d_coeffs, n, minbuf_hw, nblocks, block_stride, mode, scalefactor, normalization, c,
                 filter, d_coded, stream, lib)


def motion_ispec_blocks(d_coeffs, d_pix, n, mode, scalefactor, normalization, c=None, minbuf_hw=None, nblocks=1, block_stride=None, filter=None,
                        d_coded=0, stream=0, pixels="u8", lib=None):
    """dspfft_motion_ispec_blocks_u8 / _f32: load, decode (c is ic for shift) and filter the pixels of d_pix into coefficients in d_coeffs"""
    _spec_blocks("dspfft_motion_ispec_blocks_" + pixels, d_coeffs, d_pix, n, minbuf_hw, nblocks, block_stride, mode, scalefactor, normalization, c,
                 filter, d_coded, stream, lib)


def motion_filter_packed(d_coeffs, h, w, components, frames, packed, filter, d_coded=0, stream=0, lib=None):
    """dspfft_motion_filter_packed: motion's filter, in place, over `frames` dense frames [h][w][components] of coefficients; every component of
    a frame is a block of its own, filtered with packed's damp, boost and grey_add for its byte position (motion_packed(...)).  filter: the
    dictionary of Plan.roundtrip_u8's, active = (1, h, w) for whole frames."""
    lib = lib or _lib.load()
    pk = C.byref(packed) if packed is not None else None
    if lib.dspfft_motion_filter_packed(_ptr(d_coeffs), int(h), int(w), int(components), int(frames), *Plan._tail(filter, d_coded, stream, pk)):
        raise DspfftError(lib.dspfft_motion_last_error().decode())


def _spec_blocks_packed(fn, d_a, d_b, h, w, components, frames, mode, scalefactor, normalization, c, packed, filter, d_coded, stream, lib):
    lib = lib or _lib.load()
    sp = _spec_params(mode, scalefactor, normalization, c)
    pk = C.byref(packed) if packed is not None else None
    if getattr(lib, fn)(_ptr(d_a), _ptr(d_b), int(h), int(w), int(components), int(frames), C.byref(sp), *Plan._tail(filter, d_coded, stream, pk)):
        raise DspfftError(lib.dspfft_motion_last_error().decode())


def motion_spec_blocks_packed(d_pix, d_coeffs, h, w, components, frames, mode, scalefactor, normalization, packed, c=None, filter=None, d_coded=0,
                              stream=0, lib=None):
    """dspfft_motion_spec_blocks_u8_packed: filter, encode and store the coefficients of `frames` dense frames [h][w][components] in d_coeffs
    (read only) as packed 8-bit pixels in d_pix, the same layout; every component of a frame is a block of its own (abs: its own c)."""
    _spec_blocks_packed("dspfft_motion_spec_blocks_u8_packed", d_pix, d_coeffs, h, w, components, frames, mode, scalefactor, normalization, c, packed,
                        filter, d_coded, stream, lib)


def motion_ispec_blocks_packed(d_coeffs, d_pix, h, w, components, frames, mode, scalefactor, normalization, packed, c=None, filter=None, d_coded=0,
                               stream=0, lib=None):
    """dspfft_motion_ispec_blocks_u8_packed: load, decode (c is ic for shift) and filter the packed pixels of d_pix into d_coeffs"""
    _spec_blocks_packed("dspfft_motion_ispec_blocks_u8_packed", d_coeffs, d_pix, h, w, components, frames, mode, scalefactor, normalization, c, packed,
                        filter, d_coded, stream, lib)


def _motion_linear(fn, mode, allowed, d_dst, d_src, n, minbuf_hw, extra, trc, stream, lib):
    lib = lib or _lib.load()
    mode = _MOTION_MODES[mode] if isinstance(mode, str) else int(mode)
    if mode not in allowed:
        return -1                                             # motion.c:631-633,765-769: --linear acts in these cases of the switch only
    hw = (n[1], n[2]) if minbuf_hw is None else minbuf_hw
    rc = getattr(lib, fn)(_ptr(d_dst), _ptr(d_src), _ia(n), _ia(hw), *extra, trc_id(trc, lib), C.c_void_p(stream))
    if rc not in (0, -1):
        raise DspfftError(lib.dspfft_last_error().decode())
    return rc


def motion_load_f32_linear(d_coeffs, d_pix, n, minbuf_hw=None, trc="iec61966-2-1", ispec_mode="none", stream=0, lib=None):
    """dspfft_motion_load_f32_linear (motion --linear on float pixels, motion.c:623,633).  Returns 0; -1, decided here before the
    library is called and with nothing written, for an ispec_mode other than none (the reference decodes a spectrogram instead); -1 from
    the library for trc 0 (no function).  A trc name or id that is unknown or not built raises DspfftError (trc_id), as does a failed launch."""
    return _motion_linear("dspfft_motion_load_f32_linear", ispec_mode, (0,), d_coeffs, d_pix, n, minbuf_hw, (), trc, stream, lib)


def motion_store_f32_linear(d_pix, d_coeffs, n, minbuf_hw=None, scalefactor=1.0, normalization=1.0, trc="iec61966-2-1", spec_mode="none",
                            stream=0, lib=None):
    """dspfft_motion_store_f32_linear (motion.c:759,767-769,774).  Returns 0; -1, decided here before the library is called and with
    nothing written, for a spec_mode other than none / copy; -1 from the library for trc 0.  A trc that is unknown or not built raises
    DspfftError (trc_id), as does a failed launch."""
    return _motion_linear("dspfft_motion_store_f32_linear", spec_mode, (0, 4), d_pix, d_coeffs, n, minbuf_hw,
                          (float(scalefactor), float(normalization)), trc, stream, lib)


def motion_load_u8_linear(d_coeffs, d_pix, n, minbuf_hw=None, trc="iec61966-2-1", ispec_mode="none", stream=0, lib=None):
    """dspfft_motion_load_u8_linear (motion --linear on 8-bit pixels, motion.c:625,633): coeff = lut[byte].  Returns as
    motion_load_f32_linear does."""
    return _motion_linear("dspfft_motion_load_u8_linear", ispec_mode, (0,), d_coeffs, d_pix, n, minbuf_hw, (), trc, stream, lib)


def motion_store_u8_linear(d_pix, d_coeffs, n, minbuf_hw=None, scalefactor=1.0, normalization=1.0, trc="iec61966-2-1", spec_mode="none",
                           stream=0, lib=None):
    """dspfft_motion_store_u8_linear (motion.c:759,767-769,776): the byte of the encoded pel.  Returns as motion_store_f32_linear does."""
    return _motion_linear("dspfft_motion_store_u8_linear", spec_mode, (0, 4), d_pix, d_coeffs, n, minbuf_hw,
                          (float(scalefactor), float(normalization)), trc, stream, lib)


def u8_to_f32_trc(src, trc, out=None, stream=None, lib=None):
    """dspfft_u8_to_f32_trc over a contiguous uint8 device tensor: out = lut[src], the decode of motion --linear on 8-bit pixels (trc 0:
    the plain conversion, dspfft_u8_to_f32).  out: a float32 tensor of the same size; a new one by default."""
    import torch
    lib = lib or _lib.load()
    trc = trc_id(trc, lib)
    if out is None:
        out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    assert src.is_contiguous() and out.is_contiguous() and src.numel() == out.numel() and src.element_size() == 1 and out.element_size() == 4
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    a = (C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), src.numel())
    rc = lib.dspfft_u8_to_f32_trc(*a, trc, C.c_void_p(stream)) if trc else lib.dspfft_u8_to_f32(*a, C.c_void_p(stream))
    if rc:
        raise DspfftError(lib.dspfft_last_error().decode())
    return out


def f32_to_u8_trc(src, trc, mul=1.0, out=None, stream=None, lib=None):
    """dspfft_f32_to_u8_trc over a contiguous float32 device tensor: the byte of the encoded linear value src * mul (trc 0: the plain
    quantiser, dspfft_f32_to_u8).  out: a uint8 tensor of the same size; a new one by default."""
    import torch
    lib = lib or _lib.load()
    trc = trc_id(trc, lib)
    if out is None:
        out = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    assert src.is_contiguous() and out.is_contiguous() and src.numel() == out.numel() and src.element_size() == 4 and out.element_size() == 1
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    a = (C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), float(mul), src.numel())
    rc = lib.dspfft_f32_to_u8_trc(*a, trc, C.c_void_p(stream)) if trc else lib.dspfft_f32_to_u8(*a, C.c_void_p(stream))
    if rc:
        raise DspfftError(lib.dspfft_last_error().decode())
    return out


SPEC_SCALES = {"none": 0, "linear": 1, "log": 2}
SPEC_SIGNS = {"none": 0, "abs": 1, "shift": 2, "saturate": 3}


class ScanFrames:
    """dspfft_scanframes: scan's output frames composed on the device (scan/scan.c:366-536).  Takes torch device tensors (float32 HWC
    images, uint32 owner / coordinate tables, the float32 frame of frame_floats elements); every failure raises DspfftError.
    Options as scan's: visualize (-v), spectrogram (-s, implies -v), intermediates (-i), max_intermediates (-M, implies -i),
    spec_gain (--spec-gain, 0: the default), spec_scale / spec_sign (--spec-opts scale= / sign=), parity_depth (-P: 8, 16 or 32),
    trc (-g: the transfer characteristic, a name or an id, the left-hand panels are encoded with; 0: none)."""

    def __init__(self, w, h, visualize=False, spectrogram=False, intermediates=False, max_intermediates=False, spec_gain=0.0,
                 spec_scale="none", spec_sign="none", parity_depth=0, lib=None, trc=0):
        self._lib = lib or _lib.load()
        self._h = None
        o = _lib.ScanFrameOpts(int(bool(visualize)), int(bool(spectrogram)), int(bool(intermediates)), int(bool(max_intermediates)), float(spec_gain),
                               SPEC_SCALES[spec_scale] if isinstance(spec_scale, str) else int(spec_scale),
                               SPEC_SIGNS[spec_sign] if isinstance(spec_sign, str) else int(spec_sign), int(parity_depth))
        h_ = C.c_void_p()
        self._check(self._lib.dspfft_scanframes_create(C.byref(h_), int(w), int(h), C.byref(o)))
        self._h = h_
        self.w, self.h = int(w), int(h)
        self.visualize = bool(visualize or spectrogram)
        self.intermediates = bool(intermediates or max_intermediates)
        if trc:
            self.set_trc(trc)

    def set_trc(self, trc):
        self._check(self._lib.dspfft_scanframes_set_trc(self._h, trc_id(trc, self._lib)))

    @property
    def shape(self):
        """(3, H', W'): the frame's G, B, R planes"""
        return 3, self.h * (1 + self.intermediates), self.w * (1 + self.visualize)

    @property
    def frame_floats(self):
        return int(self._lib.dspfft_scanframes_frame_floats(self._h))

    def begin(self, frame, coeffs, stream=0):
        self._check(self._lib.dspfft_scanframes_begin(self._h, _ptr(frame), _ptr(coeffs), C.c_void_p(stream)))

    def mark_range(self, frame, coeffs, owner, lo, hi, current, stream=0):
        self._check(self._lib.dspfft_scanframes_mark_range(self._h, _ptr(frame), _ptr(coeffs), _ptr(owner), int(lo), int(hi), int(bool(current)),
                                                           C.c_void_p(stream)))

    def mark_coords(self, frame, coeffs, lin, nslots=None, current=False, stream=0):
        n = lin.numel() if nslots is None else int(nslots)
        self._check(self._lib.dspfft_scanframes_mark_coords(self._h, _ptr(frame), _ptr(coeffs), _ptr(lin), n, int(bool(current)), C.c_void_p(stream)))

    def compose(self, frame, sum_, image, coeffs, original, frame_no, stream=0):
        self._check(self._lib.dspfft_scanframes_compose(self._h, _ptr(frame), _ptr(sum_), _ptr(image), _ptr(coeffs), _ptr(original), int(frame_no),
                                                        C.c_void_p(stream)))

    def parity(self, stream=0):
        """the first frame at parity, or None (synchronises the stream)"""
        v = C.c_uint64()
        self._check(self._lib.dspfft_scanframes_parity(self._h, C.byref(v), C.c_void_p(stream)))
        return None if v.value == 2 ** 64 - 1 else int(v.value)

    def destroy(self):
        if self._h:
            self._lib.dspfft_scanframes_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise DspfftError(self._lib.dspfft_last_error().decode())


def _ptr(t):
    """a torch tensor, a raw device address or None -> c_void_p"""
    if t is None:
        return None
    return C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def scan_frame_rgb(frame, w, h, visualize=False, intermediates=False):
    """a frame (flat float32 tensor or array, G, B, R planes as dspfft_scanframes writes them) as [3, H', W'] in R, G, B order.  The planes
    are reshaped views; reordering them takes one gather (a copy: no stride maps 0, 1, 2 to planes 2, 0, 1)."""
    fw, fh = w * (1 + bool(visualize)), h * (1 + bool(intermediates))
    return frame.reshape(3, fh, fw)[[2, 0, 1]]


class Stream:
    """A HIP stream of the library's own (dspfft_stream_create: hipStreamNonBlocking).  `handle` is what execute / Batch take."""

    def __init__(self, lib=None):
        self._lib = lib or _lib.load()
        self.handle = self._lib.dspfft_stream_create()
        if not self.handle:
            raise DspfftError("stream creation failed")

    def synchronize(self):
        if self._lib.dspfft_stream_synchronize(self.handle):
            raise DspfftError(self._lib.dspfft_last_error().decode())

    def __del__(self):
        try:
            self._lib.dspfft_stream_destroy(self.handle)
        except Exception:
            pass


class Events:
    """n timing events of the library (dspfft_event_create): recorded by Batch.run on the streams of the bracketed items"""

    def __init__(self, n, lib=None):
        self._lib = lib or _lib.load()
        self.handles = (C.c_void_p * n)(*[self._lib.dspfft_event_create() for _ in range(n)])
        if any(h is None for h in self.handles):
            raise DspfftError("event creation failed")

    def elapsed_ms(self, i, j):
        ms = C.c_float()
        if self._lib.dspfft_event_elapsed_ms(self.handles[i], self.handles[j], C.byref(ms)):
            raise DspfftError(self._lib.dspfft_last_error().decode())
        return float(ms.value)

    def __del__(self):
        try:
            for h in self.handles:
                self._lib.dspfft_event_destroy(h)
        except Exception:
            pass


def many_fused_pairs(lib=None):
    """dspfft_many_fused_pairs: forward/inverse pairs that Batch.run / run_repeat have run as one roundtrip so far in this process"""
    return int((lib or _lib.load()).dspfft_many_fused_pairs())


class Batch:
    """A fixed list of executions -- (plan, d_in, d_out, stream) per item -- enqueued by ONE call of dspfft_execute_many: the
    per-frame loop of motion (motion/motion.c:613-753) or of a clip of spec/ispec frames, without a binding-layer call per frame."""

    def __init__(self, items, lib=None):
        items = list(items)
        self._lib = lib or _lib.load()
        self._keep = [it[0] for it in items]
        n = len(items)
        self.n = n
        self._plans = (C.c_void_p * n)(*[it[0]._h for it in items])
        self._in = (C.c_void_p * n)(*[it[1] for it in items])
        self._out = (C.c_void_p * n)(*[(it[1] if it[2] is None else it[2]) for it in items])
        self._streams = (C.c_void_p * n)(*[(it[3] or None) for it in items])

    def run(self, timed_item=0, timed_count=0, events=None, event_offset=0):
        ev = None
        if events is not None and timed_count:
            ev = C.cast(C.byref(events.handles, event_offset * C.sizeof(C.c_void_p)), C.POINTER(C.c_void_p))
        rc = self._lib.dspfft_execute_many(self.n, self._plans, self._in, self._out, self._streams, timed_item, timed_count if ev is not None else 0, ev)
        if rc:
            raise DspfftError(self._lib.dspfft_last_error().decode())

    def run_repeat(self, repeats, rejoin_every=0, timed_every=0, timed_count=0, events=None):
        """dspfft_execute_many_repeat: the batch `repeats` times in one library call (the frame loop of a clip); the streams of the
        batch are re-joined every `rejoin_every` repeats; every `timed_every`-th repeat brackets the passes of a rotating window of
        `timed_count` items with `events` (2 per pass, in order)."""
        ev = None
        if events is not None and timed_every and timed_count:
            ev = C.cast(events.handles, C.POINTER(C.c_void_p))
        rc = self._lib.dspfft_execute_many_repeat(self.n, self._plans, self._in, self._out, self._streams, int(repeats), int(rejoin_every),
                                                  int(timed_every) if ev is not None else 0, int(timed_count) if ev is not None else 0, ev)
        if rc:
            raise DspfftError(self._lib.dspfft_last_error().decode())

