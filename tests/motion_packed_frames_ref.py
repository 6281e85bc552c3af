"""TEST INFRASTRUCTURE ONLY: motion's default block -b 0x0x1 on packed 8-bit pixels (dspfft_execute_roundtrip_u8_packed_frames,
dspfft_motion_filter_packed): the cases, the filters and the float64 reference that tests/test_motion_packed_frames_cpu.py, _gpu.py and
tools/bench_motion_packed_frames.py --accuracy share.  The reference per component is tests/motion_spec_ref.py's forward -> apply_filter ->
inverse -> lround_u8 with every frame a block (motion/motion.c:613-615,641-776)."""
import functools

import numpy as np

import motion_spec_ref as sr
import oracle_lib as ol

FMT_OF = {2: "ya8", 3: "rgb24", 4: "rgba"}
PERMUTED = {2: "ya8", 3: "bgr24", 4: "abgr"}
#: (F, h, w, C) of the CPU test of the filter functions: rows of 54 (groups of four straddle rows and frames), two and four components
FILTER_SHAPES = [(2, 10, 18, 3), (2, 16, 12, 2), (3, 24, 40, 4)]
FILTERS = ("none", "quant", "full-dc", "full-grey", "full-permuted")
BOOST, DAMP = [2.0, 1.0, 0.5, 1.5], [0.25, 0.5, 0.0, 0.75]


def quantizer_of(h, w):
    return float(np.float32(sr.gr.quantizer_of(sr.QUANT, (1, h, w))))


def settings(h, w, comps, info, name):
    """(filter dict of the packed call, dspfft_motion_packed, the planar filter dict of every BYTE POSITION).  none; quant: the quantiser
    alone; full-dc / full-grey: the band (0, 3, 1) - (1, h - 5, w - 7), which stops the DC, another damp and boost per component, a threshold,
    preserve_dc = 1 / 2 and the quantiser; full-permuted: full-grey through motion_packed("bgr24" / "abgr"), whose byte positions are not the
    component order."""
    from dspfun_amd.engine import motion_packed, PACKED_FORMATS
    fmt = PERMUTED[comps] if name == "full-permuted" else FMT_OF[comps]
    base = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w))
    if name == "none":
        return None, motion_packed(fmt), [None] * comps
    q = quantizer_of(h, w)
    if name == "quant":
        f = dict(base, quantizer=q)
        # (-D's default of 0 never acts: the band is the whole frame; the packed call does not read the dictionary's damp and boost)
        return dict(f, damp=99.0, boost=99.0), motion_packed(fmt, damp=1.0), [dict(f, damp=1.0, boost=1.0) for _ in range(comps)]
    f = dict(base, band_begin=(0, 3, 1), band_end=(1, h - 5, w - 7), threshold_lo=q / 8, threshold_hi=1e30, preserve_dc=1 if name == "full-dc" else 2, quantizer=q)
    p = motion_packed(fmt, boost=BOOST[:comps], damp=DAMP[:comps], dcstop=True, normalization=info["normalization"], scalefactor=info["scalefactor"])
    planes = [dict(f, damp=p.damp[at], boost=p.boost[at], grey_add=p.grey_add[at]) for at in range(comps)]
    for i, at in enumerate(PACKED_FORMATS[fmt]):
        assert planes[at]["boost"] == np.float32(BOOST[i]) and planes[at]["damp"] == np.float32(DAMP[i])
    return dict(f, damp=99.0, boost=99.0, grey_add=99.0), p, planes


@functools.lru_cache(maxsize=None)
def clip_of(F, h, w, comps, seed=0x0F2A):
    a = ol.synth_u8(seed + comps + 16 * F + w, F * h * w * comps).reshape(F, h, w, comps)
    a.setflags(write=False)
    return a


# ---- the float64 reference of the rgb24 clip of 3 x 24 x 40 ----
REF_FRAMES, REF_H, REF_W = 3, 24, 40
REF_BLOCK = (1, REF_H, REF_W)
REF_KINDS = (None, "band", "full", "q")
# another damp and boost per component (motion -D / -B r:g:b), float32 values; the band, preserve_dc = dc and -q are motion_spec_ref.filter_of's
REF_DAMP, REF_BOOST = (0.25, 0.5, 0.75), (1.5, 2.0, 1.25)


def ref_filter(kind, comp):
    f = sr.filter_kind(kind, REF_BLOCK)
    if kind in ("band", "full"):
        f = dict(f, damp=REF_DAMP[comp], boost=REF_BOOST[comp])
    return f


def _roundtrip(plane, filt):
    """one component plane [F][h][w] of bytes through the reference: every frame a block"""
    c = sr.forward(plane.astype(np.float64)[:, None], REF_BLOCK)
    win = []
    coded, tie = sr.apply_filter(c, filt, window=win)
    pel = sr.inverse(c, REF_BLOCK)[:, 0]
    # a coefficient on a tie may round either way in a float pipeline, and the inverse transform spreads it over its frame
    frames = None if tie is None else np.broadcast_to(tie.any(axis=(1, 2, 3))[:, None, None], pel.shape)
    return dict(pel=pel, out8=sr.lround_u8(pel), coded=coded, tie=frames, coeff_tie=tie, window=win[0] if win else 0.0, filt=filt)


@functools.lru_cache(maxsize=None)
def ref_seeds():
    """per component, the first seed from 400 on whose plane keeps every coefficient of the reference, as each quantising filter of that
    component leaves it ahead of the quantiser, farther than EDGE from a rounding boundary of coefficient / quantizer -- how
    motion_grid_ref.case chooses its volumes"""
    seeds = []
    n = REF_FRAMES * REF_H * REF_W
    for comp in range(3):
        for seed in range(400 + 100 * comp, 500 + 100 * comp):
            plane = ol.synth_u8(seed, n).reshape(REF_FRAMES, REF_H, REF_W)
            ok = True
            for kind in ("full", "q"):
                f = ref_filter(kind, comp)
                c = sr.forward(plane.astype(np.float64)[:, None], REF_BLOCK)
                sr.apply_filter(c, dict(f, quantizer=0.0))
                t = c / f["quantizer"]
                ok = ok and float(np.abs(np.abs(t - np.floor(t)) - 0.5).min()) > sr.EDGE
            if ok:
                seeds.append(seed)
                break
        else:
            raise AssertionError("no seed keeps the coefficients off the quantiser's rounding boundaries")
    return tuple(seeds)


@functools.lru_cache(maxsize=None)
def ref_case(kind):
    """(the interleaved rgb24 clip, [the reference of every component])"""
    n = REF_FRAMES * REF_H * REF_W
    planes = [ol.synth_u8(seed, n).reshape(REF_FRAMES, REF_H, REF_W) for seed in ref_seeds()]
    refs = [_roundtrip(p, ref_filter(kind, comp)) for comp, p in enumerate(planes)]
    clip = np.ascontiguousarray(np.stack(planes, axis=-1))
    clip.setflags(write=False)
    return clip, refs


def ref_packed(kind, info):
    """the packed call's (filter dict, dspfft_motion_packed) for ref_case(kind)"""
    from dspfun_amd.engine import motion_packed
    f = sr.filter_kind(kind, REF_BLOCK)
    if kind in ("band", "full"):
        return f, motion_packed("rgb24", boost=REF_BOOST, damp=REF_DAMP, dcstop=True, normalization=info["normalization"], scalefactor=info["scalefactor"])
    return f, motion_packed("rgb24", damp=1.0)


def ref_shares(outs, refs):
    """(max byte difference, differing bytes, bytes compared) of the component planes `outs` against the references, off the ties"""
    mx = n = size = 0
    for out, ref in zip(outs, refs):
        m, d, s = sr.share_of(out, ref["out8"], ref["tie"])
        mx, n, size = max(mx, m), n + d, size + s
    return mx, n, size


# ---- device runs (torch is passed in) ----
PAGE, MARK = 4096, 0xA5


def framed(torch, n, offset=0):
    """n output bytes with a marker page on each side (offset: bytes off the page's alignment)"""
    buf = torch.full((n + 2 * PAGE + offset,), MARK, dtype=torch.uint8, device="cuda:0")
    return buf, buf[PAGE + offset:PAGE + offset + n]


def check_frame(buf, n, offset=0):
    b = buf.cpu().numpy()
    assert (b[:PAGE + offset] == MARK).all() and (b[PAGE + offset + n:] == MARK).all(), "the call wrote outside the clip"


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def run_call(torch, fwd, inv, src, info, packed, filt=None, in_place=False, offset=0):
    """Plan.roundtrip_u8_packed_frames on the interleaved clip src (numpy [F][h][w][C]).  Returns (bytes, coded)."""
    n = src.size
    buf, out = framed(torch, n, offset)
    if offset:          # (the input shares the output's misalignment)
        _, d_in = framed(torch, n, offset)
        d_in.copy_(torch.from_numpy(np.array(src)).reshape(-1))
    else:
        d_in = torch.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    if in_place:
        out.copy_(d_in)
        d_in = out
    wk = torch.empty(n, dtype=torch.float32, device="cuda:0")
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8_packed_frames(inv, d_in.data_ptr(), out.data_ptr(), wk.data_ptr(), info["out_mul"], packed, filter=filt, d_coded=coded.data_ptr(),
                                   stream=stream_of(torch))
    torch.cuda.synchronize()
    check_frame(buf, n, offset)
    return out.cpu().numpy().reshape(src.shape), int(coded.item())


def composition(torch, L, fwd, inv, src, info, packed, filt, trc=0):
    """dspfft_u8_to_f32 -> dspfft_execute(fwd) -> dspfft_motion_filter_packed -> dspfft_execute(inv) -> dspfft_f32_to_u8(out_mul); trc: the
    flat pair with that transfer characteristic at both ends.  Returns (bytes, coded, the coefficients the filter read, those it left)."""
    from dspfun_amd.engine import motion_filter_packed
    F, h, w, comps = src.shape
    n = src.size
    s = stream_of(torch)
    d_in = torch.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    wk = torch.empty(n, dtype=torch.float32, device="cuda:0")
    buf, out = framed(torch, n)
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    if trc:
        assert L.dspfft_u8_to_f32_trc(wk.data_ptr(), d_in.data_ptr(), n, trc, s) == 0
    else:
        assert L.dspfft_u8_to_f32(wk.data_ptr(), d_in.data_ptr(), n, s) == 0
    fwd.execute(wk.data_ptr(), stream=s)
    before = wk.clone()
    if filt is not None:
        motion_filter_packed(wk, h, w, comps, F, packed, dict(filt, active=(1, h, w), minbuf_hw=(h, w), block_depth=1), d_coded=coded.data_ptr(), stream=s)
    after = wk.clone()
    inv.execute(wk.data_ptr(), stream=s)
    if trc:
        assert L.dspfft_f32_to_u8_trc(out.data_ptr(), wk.data_ptr(), info["out_mul"], n, trc, s) == 0
    else:
        assert L.dspfft_f32_to_u8(out.data_ptr(), wk.data_ptr(), info["out_mul"], n, s) == 0
    torch.cuda.synchronize()
    check_frame(buf, n)
    return out.cpu().numpy().reshape(src.shape), int(coded.item()), before.cpu().numpy().reshape(src.shape), after.cpu().numpy().reshape(src.shape)


def planar_roundtrip(torch, plane, filt):
    """Plan.roundtrip_u8 on one component plane [F][h][w] with per-frame plans (motion's scales).  Returns (bytes, coded)."""
    F, h, w = plane.shape
    block = (1, h, w)
    fwd, inv = sr.stack_plan(block, F, ol.REDFT10), sr.stack_plan(block, F, ol.REDFT01)
    sf, nm, _ = sr.constants(block)
    d_in = torch.from_numpy(np.ascontiguousarray(plane)).to("cuda:0")
    d_out = torch.zeros_like(d_in)
    wk = torch.empty(plane.size, dtype=torch.float32, device="cuda:0")
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), wk.data_ptr(), sf * nm * nm, filter=filt, d_coded=coded.data_ptr(), stream=stream_of(torch))
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), int(coded.item())

