"""TEST INFRASTRUCTURE ONLY: motion --spectrogram and --ispectrogram over a grid of blocks in float64 (motion/motion.c:617-776 with `spec` /
`ispec` set), block by block.  The spectrogram without a filter or with -q alone IS tests/motion_ref.py's block_roundtrip(..., spec=);
with the whole filter (-p with a DC stop, --preserve-dc, -q: :683-744) and for float pixels it is the same pieces -- the oracle's REDFT10,
oracle_motion_uniform_f64 -- with :683-744 and :755-771 restated here, and spec_grid asserts that the two agree byte for byte wherever
block_roundtrip can express the case.  The ispectrogram direction: decode per :627-630, the filter, oracle_motion_uniform_f64 backwards, the
oracle's REDFT01, :759-776.  Shared by tests/test_motion_spec_cpu.py and _gpu.py."""
import functools

import numpy as np

import motion_grid_ref as gr
import motion_ref as mr
import oracle_lib as ol

SPEC_MODES = ("abs", "shift", "flat", "copy")
ISPEC_MODES = ("shift", "flat", "copy")
# (block, volume) as (d, h, w): in every one the last workgroup of a row of blocks is partly filled, and the 16-element blocks share a wave
SHAPES = [((4, 4, 4), (8, 12, 68)), ((8, 8, 8), (16, 24, 72)), ((4, 8, 16), (8, 16, 80)), ((16, 16, 16), (16, 32, 48)), ((1, 32, 32), (3, 64, 96)),
          ((1, 4, 4), (2, 8, 52))]
# every other plan: (block, frames or blocks) -- 540 x 960 are the smallest listed row and column kernels with an 8-bit row end (spec_list.h:
# 960 C=1, 540); 24 x 40 is runtime geometry, converted by sweeps; one 3-D block
PASSES = [((1, 540, 960), 3), ((1, 24, 40), 3), ((4, 24, 40), 1)]
BLOCK_MAJOR = (0, 4)             # the shapes also run as block-major stacks
# -q.  Not a short decimal: the coefficients of 8-bit samples lie on a lattice (integers / 8, times powers of sqrt 2), and a quantizer that is a
# ratio of small integers (0.4 with 4x4x4 blocks: 128 / 5) puts some of them exactly on its ties in every volume
QUANT = float(np.float32(np.sqrt(0.17)))
EDGE = gr.EDGE


def shape_id(s):
    return "x".join(map(str, s[0])) + "-in-" + "x".join(map(str, s[1]))


def nblocks_of(block, vol):
    return tuple(v // b for v, b in zip(vol, block))


def constants(block):
    """motion.c:566-569 with scaled = block"""
    sf, nm = mr.consts(block, block)
    c = 127.5 / np.log1p(float(np.prod(block)) * nm * 255 * 8)
    return sf, nm, c


def filter_of(block, quant=QUANT):
    """-p with a DC stop, --preserve-dc=dc, --damp, --boost and -q as dspfft_motion_filter_params' fields (Plan._filter_params' dict); every
    float field is a float32 value, so the float64 restatement and the kernels read the same numbers"""
    d, h, w = block
    return dict(active=block, minbuf_hw=(h, w), block_depth=d, band_begin=(0, 1, 1), band_end=(d, max(2, h - 1), max(2, w - 2)),
                damp=0.25, boost=1.5, preserve_dc=1, quantizer=float(np.float32(gr.quantizer_of(quant, block))))


def band_only(block):
    """filter_of without -q: every sample is compared (no quantiser, no ties)"""
    f = filter_of(block)
    f["quantizer"] = 0.0
    return f


def filter_kind(kind, block):
    """None, "band" (band_only), "full" (filter_of) or "q" (quant_only)"""
    return {None: None, "band": band_only(block), "full": filter_of(block), "q": quant_only(block)}[kind]


def check_tie_share(ref, inverse):
    """the samples a comparison leaves out are few: twice the tie window's half-width of the coefficients (with room for clustering: five times that); in the inverse direction
    a whole block per tie, and a decoded byte is one of 256 values, so one value near a tie recurs in many blocks: fewer than half"""
    if ref["tie"] is None:
        return
    share = float(ref["tie"].mean())
    assert share < 0.5 if inverse else share <= 10 * ref["window"] + 8 / ref["tie"].size, share


def coded_slack(ref, block):
    """by how much a float pipeline's count of coded coefficients may differ from the reference's: the coefficients on a tie"""
    return ref["nties"] * int(np.prod(block)) if "nties" in ref else int(ref["tie"].sum())


def quant_only(block, quant=QUANT):
    d, h, w = block
    return dict(active=block, minbuf_hw=(h, w), block_depth=d, band_begin=(0, 0, 0), band_end=block, quantizer=float(np.float32(gr.quantizer_of(quant, block))))


def lround_u8(pel):
    r = np.where(pel >= 0, np.floor(pel + 0.5), -np.floor(-pel + 0.5))              # lround: halves away from zero (:776)
    return np.clip(r, 0, 255).astype(np.uint8)


def apply_filter(c, filt, transformed=True, window=None):
    """motion.c:683-744 on blocks [nb][d][h][w] of uniform-range coefficients, in place.  Returns (coded count, `tie`: where the quotient
    coefficient / quantizer comes within EDGE of a rounding boundary -- there the float pipeline, the reference's own included, may round the
    other way, and this float64 restatement does not say which way the reference goes)."""
    window = [] if window is None else window          # (out: the mean half-width of the tie window, for check_tie_share)
    if filt is None:
        return 0, None
    _, d, h, w = c.shape
    dc = c[:, 0, 0, 0].copy()                                                        # :650
    b0, b1 = filt["band_begin"], filt["band_end"]
    damp, boost = float(np.float32(filt.get("damp", 1.0))), float(np.float32(filt.get("boost", 1.0)))
    inside = np.zeros((d, h, w), dtype=bool)
    inside[b0[0]:b1[0], b0[1]:b1[1], b0[2]:b1[2]] = True
    c[:, ~inside] *= damp                                                            # :683-714: the six slabs are the complement of the box
    c[:, inside] *= boost                                                            # :715-719
    assert not filt.get("threshold_hi")
    pdc = filt.get("preserve_dc", 0)
    if pdc and (any(b0) or boost != 1.0):                                            # :730-738
        assert pdc == 1
        c[:, 0, 0, 0] = dc
    q = filt.get("quantizer", 0.0)
    if not q:
        return 0, None
    t = c / q                                                                        # :740-744
    # (the reference and the kernels divide in single precision, :744: a quotient moves by up to 2^-24 |t| against this float64 one)
    # and a float transform that made the coefficient (`transformed`: the spectrogram direction) carries about one rounding per butterfly
    # stage, log2(E) of them.  While E x 255 < 2^24 every partial sum of 8-bit samples is exact in float, the block's DC contributes no
    # rounding and the roundings are relative to the AC coefficients (inside EDGE); beyond that (a 540x960 frame) they are relative to the
    # block's largest coefficient, the DC: 2^-24 log2(E) max|t|, about 1e-3 of a quantiser step there
    e = float(d * h * w)
    grow = 2.0 ** -24 * np.log2(e) * np.abs(t).max(axis=(1, 2, 3), keepdims=True) if transformed and e * 255 >= 2 ** 24 else 0.0
    tie = np.abs(np.abs(t - np.floor(t)) - 0.5) <= EDGE + 1.2e-7 * np.abs(t) + grow
    r = np.copysign(np.floor(np.abs(t) + 0.5), t)
    c[...] = r * q
    window.append(float(np.mean(EDGE + 1.2e-7 * np.abs(t) + grow)))
    return int(np.count_nonzero(r)), tie


def encode(c, dc, mode, block):
    """motion.c:755-771: the pel of every coefficient of blocks [nb][d][h][w]; dc [nb]: the blocks' DCs from before the filter"""
    sf, nm, cs = constants(block)
    pel = c * sf * nm
    if mode == "abs":
        cc = 255.0 / np.log1p(np.abs(dc * sf * nm))
        return cc[:, None, None, None] * np.log1p(np.abs(pel))
    if mode == "shift":
        return cs * np.copysign(np.log1p(np.abs(pel)), pel) + 127.5
    if mode == "flat":
        return pel * nm / 2 + 127.5
    return pel * nm


def decode(pel, mode, block):
    """motion.c:627-630"""
    _, nm, ic = constants(block)
    if mode == "shift":
        return np.copysign(np.expm1(np.abs((pel - 127.5) / ic)), pel - 127.5) / nm
    if mode == "flat":
        return (pel - 127.5) * 2 / nm / nm
    return pel / nm / nm


@functools.lru_cache(maxsize=None)
def uniform(block, direction):
    """the factors of :644-647 (direction 1) or :748-751 (-1) for one block: oracle_motion_uniform_f64 applied to ones"""
    f = np.ones(block, dtype=np.float64)
    ol.lib().oracle_motion_uniform_f64(f.ctypes.data, block[0], block[1], block[2], block[1], block[2], direction)
    f.setflags(write=False)
    return f


def forward(pel_blocks, block):
    """[nb][d][h][w] float64 pels -> uniform-range coefficients (:641-647)"""
    nb = len(pel_blocks)
    e = int(np.prod(block))
    c = ol.r2r_many(np.ascontiguousarray(pel_blocks, dtype=np.float64), list(block), [ol.REDFT10] * 3, howmany=nb, idist=e, odist=e, impl="port").reshape((nb,) + tuple(block))
    return c * uniform(block, 1)


def inverse(c, block):
    """uniform-range coefficients -> the pels before :776 rounds them (:748-753,759,767)"""
    nb = len(c)
    e = int(np.prod(block))
    c = np.ascontiguousarray(c * uniform(block, -1), dtype=np.float64)
    o = ol.r2r_many(c, list(block), [ol.REDFT01] * 3, howmany=nb, idist=e, odist=e, impl="port").reshape((nb,) + tuple(block))
    sf, nm, _ = constants(block)
    return o * sf * nm * nm


def spec_grid(vol, block, mode, filt=None, float_pixels=False):
    """the spectrogram of every block of a [D][H][W] uint8 volume.  float_pixels: the samples are float32(vol / 255) and the pel is their
    float product with 255 (:623).  Returns dict(pel, out8, tie: volumes (tie: apply_filter's, None without a quantiser); coded; dc [nb])."""
    nbk = nblocks_of(block, vol.shape)
    if float_pixels:
        pels = (pixels_f32(vol) * np.float32(255)).astype(np.float64)
    else:
        pels = vol.astype(np.float64)
    c = forward(gr.to_blocks(pels, block), block)
    dc = c[:, 0, 0, 0].copy()
    win = []
    coded, tie = apply_filter(c, filt, window=win)
    pel = encode(c, dc, mode, block)
    out8 = lround_u8(pel)
    plain_q = filt is not None and not any(filt["band_begin"]) and tuple(filt["band_end"]) == tuple(block) and filt.get("damp", 1.0) == 1.0 and filt.get("boost", 1.0) == 1.0
    if not float_pixels and (filt is None or plain_q):
        # tests/motion_ref.py block by block: the same bytes (its quantiser is QUANT's own float64 value; the float32 one the kernels and
        # the restatement take differs from it by 3e-8 of itself, far less than EDGE, so off the ties both round alike)
        for b, blk in enumerate(gr.to_blocks(vol, block)):
            o, _, _ = mr.block_roundtrip(blk, block, block, block, quant=QUANT if filt else 0.0, spec=mode)
            same = o == out8[b]
            assert np.all(same if tie is None else same | tie[b]), (b, mode)
    return dict(pel=gr.from_blocks(pel, block, nbk), out8=gr.from_blocks(out8, block, nbk), coded=coded, dc=dc,
                tie=None if tie is None else gr.from_blocks(tie, block, nbk), window=win[0] if win else 0.0)


def ispec_grid(pix, block, mode, filt=None):
    """the inverse spectrogram of every block of a [D][H][W] volume of pixels: uint8, or float32 samples (float_pixels).  Returns dict(pel,
    out8, tie: volumes (tie: every sample of a block one of whose coefficients is on a tie); coded)."""
    nbk = nblocks_of(block, pix.shape)
    pels = pix.astype(np.float64) if pix.dtype == np.uint8 else (pix.astype(np.float32) * np.float32(255)).astype(np.float64)
    c = decode(gr.to_blocks(pels, block), mode, block)
    coded, tie = apply_filter(c, filt, transformed=False)
    pel = inverse(c, block)
    if tie is not None:
        tie = np.broadcast_to(tie.any(axis=(1, 2, 3))[:, None, None, None], tie.shape)
    return dict(pel=gr.from_blocks(pel, block, nbk), out8=gr.from_blocks(lround_u8(pel), block, nbk), coded=coded,
                tie=None if tie is None else gr.from_blocks(tie, block, nbk), nties=0 if tie is None else int(tie[:, 0, 0, 0].sum()))


def pixels_f32(vol_u8):
    return (vol_u8.astype(np.float32) / np.float32(255)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def volume(block, vol_shape, seed=300):
    """a seeded uint8 volume (oracle_lib.synth_u8)"""
    vol = ol.synth_u8(seed + sum(block), int(np.prod(vol_shape))).reshape(vol_shape)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def spec_case(block, vol_shape, mode, filt_kind=None, float_pixels=False):
    """filt_kind: filter_kind's.  Computed once per session; the arrays are read-only."""
    vol = volume(block, vol_shape)
    filt = filter_kind(filt_kind, block)
    r = spec_grid(vol, block, mode, filt, float_pixels)
    assert np.all(r["dc"] != 0)
    r.update(vol=vol, filt=filt)
    for a in (r["pel"], r["out8"]):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def ispec_case(block, vol_shape, mode, filt_kind=None, float_pixels=False):
    """the input is the reference's own spectrogram of volume(...) in `mode` (bytes, or for float pixels float32(pel / 255), :774), so the
    output is an image and not a saturated plane"""
    src = spec_case(block, vol_shape, mode, None, float_pixels)
    pix = (src["pel"] / 255).astype(np.float32) if float_pixels else src["out8"]
    filt = filter_kind(filt_kind, block)
    r = ispec_grid(pix, block, mode, filt)
    r.update(pix=pix, filt=filt)
    for a in (r["pel"], r["out8"], pix):
        a.setflags(write=False)
    return r


# ---- plans with motion's scales (motion.c:644-647 forward; :748-751 and 1 / (2 sqrt 2) inverse), for the tests and the bench tool's twin ----
def _scaled(p, kind, naxes, two_d):
    import math
    r2 = math.sqrt(2.0)
    unit = r2 if two_d else 1.0          # a unit axis of the reference's 3-D plans: REDFT10 doubles and the uniform range divides by sqrt 2
    p.set_scale(2 * r2 * unit if kind == ol.REDFT10 else unit / (2 * r2))
    for a in range(naxes):
        p.set_axis_scale0(a, *((1.0, 1.0 / r2) if kind == ol.REDFT10 else (r2, 1.0)))
    return p


def volume_plan(block, vol, kind, lib=None):
    """every block of a [D][H][W] volume, in place"""
    from dspfun_amd.engine import Plan
    (bd, bh, bw), (D, H, W) = block, vol
    two_d = bd == 1
    dims = [(bd, H * W, H * W), (bh, W, W), (bw, 1, 1)][1 if two_d else 0:]
    how = [(D // bd, bd * H * W, bd * H * W), (H // bh, bh * W, bh * W), (W // bw, bw, bw)]
    return _scaled(Plan.guru(dims, how, [kind] * len(dims), lib=lib), kind, len(dims), two_d)


def stack_plan(block, nblocks, kind, lib=None):
    """a block-major stack of nblocks blocks, in place; also the plan of a clip of frames (block = (1, h, w)) and of one 3-D block"""
    from dspfun_amd.engine import Plan
    two_d = block[0] == 1
    n = list(block[1:] if two_d else block)
    e = int(np.prod(block))
    p = Plan.many_r2r(n, [kind] * len(n), howmany=nblocks, idist=e, odist=e, lib=lib, first_axis_first=kind == ol.REDFT01)
    return _scaled(p, kind, len(n), two_d)


# ---- device runs shared by tests/test_motion_spec_gpu.py and tools/bench_motion_spec.py --accuracy (torch is passed in) ----
def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def fused(torch, plan, inverse, pix, block, mode, filt=None, with_work=False, in_place=False):
    """one fused call on a device copy of `pix` (uint8 or float32, any shape the plan's layout reads); returns (output array, coded)"""
    sf, nm, c = constants(block)
    src = dev(torch, pix)
    out = src if in_place else torch.zeros_like(src)
    work = torch.empty(src.numel(), dtype=torch.float32, device="cuda:0") if with_work else None
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    run = plan.ispectrogram if inverse else plan.spectrogram
    run(src.data_ptr(), out.data_ptr(), mode, sf, nm, c, d_work=work.data_ptr() if with_work else 0, filter=filt, d_coded=coded.data_ptr(),
        stream=torch.cuda.current_stream().cuda_stream, pixels="u8" if pix.dtype == np.uint8 else "f32")
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(coded.item())


def composition(torch, L, inverse, stack, block, mode, filt=None):
    """what a caller composed before the fused calls, on a block-major stack [nb][d][h][w] of pixels (uint8 or float32): returns the stack
    of output pixels.  abs reads every block's DC back to the host for its c (motion.c:755)."""
    from dspfun_amd.engine import Plan
    sf, nm, c = constants(block)
    nb = len(stack)
    d, h, w = block
    e = d * h * w
    import ctypes as C
    I3, I2 = C.c_int * 3, C.c_int * 2
    u8 = stack.dtype == np.uint8
    plan = stack_plan(block, nb, ol.REDFT01 if inverse else ol.REDFT10)
    pix = dev(torch, stack)
    co = torch.zeros(nb * e, dtype=torch.float32, device="cuda:0")
    m = {"none": 0, "abs": 1, "shift": 2, "flat": 3, "copy": 4}
    fp = Plan._filter_params(filt)

    def filter_blocks():
        if fp is None:
            return
        for b in range(nb):
            assert L.dspfft_motion_filter(co.data_ptr() + 4 * b * e, I3(d, h, w), I2(h, w), fp.band_begin, fp.band_end, fp.damp, fp.boost, fp.threshold_lo,
                                          fp.threshold_hi, fp.preserve_dc, fp.grey_add, fp.quantizer, None, None) == 0
    all_n, hw = I3(nb * d, h, w), I2(h, w)
    if not inverse:
        load = L.dspfft_motion_load_u8 if u8 else L.dspfft_motion_load_f32
        assert load(co.data_ptr(), pix.data_ptr(), all_n, hw, 0, 0.0, nm, None) == 0
        plan.execute(co.data_ptr())
        dcs = co[::e].cpu().numpy().astype(np.float64) if mode == "abs" else None                   # the host round trip
        filter_blocks()
        out = torch.zeros_like(pix)
        store = L.dspfft_motion_store_u8 if u8 else L.dspfft_motion_store_f32
        if mode == "abs":
            for b in range(nb):
                cc = 255.0 / np.log1p(abs(dcs[b] * sf * nm))
                assert store(out.data_ptr() + b * e * pix.element_size(), co.data_ptr() + 4 * b * e, I3(d, h, w), hw, 1, sf, nm, cc, None) == 0
        else:
            assert store(out.data_ptr(), co.data_ptr(), all_n, hw, m[mode], sf, nm, c, None) == 0
    else:
        load = L.dspfft_motion_load_u8 if u8 else L.dspfft_motion_load_f32
        assert load(co.data_ptr(), pix.data_ptr(), all_n, hw, m[mode], c, nm, None) == 0
        filter_blocks()
        plan.execute(co.data_ptr())
        out = torch.zeros_like(pix)
        if u8:
            assert L.dspfft_f32_to_u8(out.data_ptr(), co.data_ptr(), sf * nm * nm, nb * e, None) == 0
        else:
            assert L.dspfft_motion_store_f32(out.data_ptr(), co.data_ptr(), all_n, hw, 0, sf, nm, 0.0, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def share_of(got, ref, tie=None):
    """(max byte difference, differing bytes, bytes compared) off the quantiser's ties (motion_spec_ref.apply_filter)"""
    diff = np.abs(got.astype(int) - ref.astype(int))
    if tie is not None:
        diff = diff[~tie]
    return int(diff.max()), int((diff > 0).sum()), diff.size


def float_err(got, ref_pel, tie=None):
    want = ref_pel / 255
    ok = slice(None) if tie is None else ~tie
    return float(np.abs(got - want)[ok].max() / np.abs(want).max())


def cases_of(inverse, block, vol_shape, mode):
    """(filter kind, float pixels?, reference, pixels) for 8-bit pixels without a filter, with the filter without -q, with the whole filter and
    with -q alone, and for float pixels without one"""
    case = ispec_case if inverse else spec_case
    for kind, fl in ((None, False), ("band", False), ("full", False), ("q", False), (None, True)):
        ref = case(block, vol_shape, mode, kind, fl)
        pix = ref["pix"] if inverse else (pixels_f32(ref["vol"]) if fl else ref["vol"])
        yield kind, fl, ref, pix
