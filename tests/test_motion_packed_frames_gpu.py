"""motion's default block -b 0x0x1 on packed 8-bit pixels on the device (dspfft_execute_roundtrip_u8_packed_frames,
dspfft_motion_filter_packed).
  1. the call equals, byte for byte and count for count, the composition dspfft_u8_to_f32 -> dspfft_execute(fwd) ->
     dspfft_motion_filter_packed -> dspfft_execute(inv) -> dspfft_f32_to_u8 on the same plans -- fused passes give the bits of their separate
     passes (tests/test_gpu_parity.py) --, in place and out of place, under DSPFFT_NO_FUSED_ROUNDTRIP=1 and with a transfer characteristic
  2. the stand-alone kernel equals the planar dspfft_motion_filter on every de-interleaved plane with that component's values
  3. the call is held against the float64 reference (tests/motion_packed_frames_ref.py) per component
  4. refusals on the device library write nothing
Every output goes into a buffer with a marker page on each side."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_packed_frames_ref as pf
import motion_spec_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


class unfused:
    """DSPFFT_NO_FUSED_ROUNDTRIP=1 for the calls inside (the library reads it on every call)"""
    def __enter__(self):
        self.prev = os.environ.get("DSPFFT_NO_FUSED_ROUNDTRIP")
        os.environ["DSPFFT_NO_FUSED_ROUNDTRIP"] = "1"

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ["DSPFFT_NO_FUSED_ROUNDTRIP"]
        else:
            os.environ["DSPFFT_NO_FUSED_ROUNDTRIP"] = self.prev


def lines_of(plan, axis):
    return [l for l in plan.describe().splitlines() if l.startswith(f"axis {axis}")]


# (F, h, w, C, byte offset): what describe() must show of the pair -- row: the listed interleaved row kernel (ROW* C=3); col: the listed
# column kernel of that tile width (COL* K=..), None: generic passes
CASES = [
    (2, 256, 256, 3, 0, "ROW*", 32),          # interleaved 8-bit row ends, the 256-point column spec with K = 32, the fused packed column kernel
    (2, 256, 256, 3, 1, "ROW*", 32),          # the byte buffers 1 off a multiple of 4: the sweeps at the ends
    (2, 256, 80, 3, 0, None, 16),             # inner extent 240: K = 16, a tile straddles pixels and components; generic rows
    (2, 256, 64, 4, 0, None, 32),             # four components: fused column, no interleaved row end
    (3, 24, 40, 3, 0, None, None),            # generic passes: the unfused sequence
    (3, 24, 40, 4, 0, None, None),
    (2, 10, 18, 3, 0, None, None),            # rows of 54: the scalar path of the filter kernel
    (2, 16, 12, 2, 0, None, None),            # two components
]


def check_kernels(fwd, inv, comps, row, col):
    for plan in (fwd, inv):
        r, c = lines_of(plan, 1), lines_of(plan, 0)
        assert len(r) == 1 and len(c) == 1, plan.describe()
        assert ("ROW*" in r[0] and f"C={comps}" in r[0]) == (row is not None), plan.describe()
        if col is None:
            assert "COL*" not in c[0], plan.describe()
        else:
            assert "COL*" in c[0] and f"K={col} " in c[0] and "N=256" in c[0], plan.describe()


# ---- 1. the call equals its composition ----
@pytest.mark.parametrize("F,h,w,comps,offset,row,col", CASES, ids=[f"{f}x{h}x{w}x{c}" + ("-off1" if o else "") for f, h, w, c, o, _, _ in CASES])
def test_the_call_equals_its_composition(gpu, F, h, w, comps, offset, row, col):
    from dspfun_amd import _lib
    from dspfun_amd.engine import motion_packed_frame_plans
    L = _lib.load()
    fwd, inv, info = motion_packed_frame_plans(F, h, w, comps)
    check_kernels(fwd, inv, comps, row, col)
    src = pf.clip_of(F, h, w, comps)
    for name in pf.FILTERS:
        filt, packed, planes = pf.settings(h, w, comps, info, name)
        want, wcoded, _, _ = pf.composition(gpu, L, fwd, inv, src, info, packed, filt)
        assert (name == "none") == (wcoded == 0), (name, wcoded)
        assert len(np.unique(want)) > 8, name
        if name == "none":
            assert np.abs(want.astype(int) - src.astype(int)).max() <= 1          # the roundtrip of bytes brings them back
        for in_place in (False, True):
            got, coded = pf.run_call(gpu, fwd, inv, src, info, packed, filt, in_place=in_place, offset=offset)
            assert np.array_equal(got, want), (name, in_place, int((got != want).sum()))
            assert coded == wcoded, (name, in_place, coded, wcoded)
        with unfused():
            got, coded = pf.run_call(gpu, fwd, inv, src, info, packed, filt, offset=offset)
        assert np.array_equal(got, want) and coded == wcoded, (name, "unfused", int((got != want).sum()), coded, wcoded)


@pytest.mark.parametrize("F,h,w,comps", [(2, 256, 256, 3), (3, 24, 40, 4)], ids=["2x256x256x3", "3x24x40x4"])
def test_a_transfer_characteristic_is_honoured_by_the_flat_sweeps(gpu, F, h, w, comps):
    """motion --linear: dspfft_plan_set_u8_trc on both plans; that end then does not ride on the row pass"""
    from dspfun_amd import _lib
    from dspfun_amd.engine import motion_packed_frame_plans, trc_id
    L = _lib.load()
    fwd, inv, info = motion_packed_frame_plans(F, h, w, comps)
    plain = motion_packed_frame_plans(F, h, w, comps)
    src = pf.clip_of(F, h, w, comps)
    trc = trc_id("iec61966-2-1", L)
    fwd.set_u8_trc("iec61966-2-1"); inv.set_u8_trc("iec61966-2-1")
    for name in ("none", "full-grey"):
        filt, packed, _ = pf.settings(h, w, comps, info, name)
        want, wcoded, _, _ = pf.composition(gpu, L, plain[0], plain[1], src, info, packed, filt, trc=trc)
        without = pf.composition(gpu, L, plain[0], plain[1], src, info, packed, filt)[0]
        assert not np.array_equal(want, without) or name == "none"
        for in_place in (False, True):
            got, coded = pf.run_call(gpu, fwd, inv, src, info, packed, filt, in_place=in_place)
            assert np.array_equal(got, want) and coded == wcoded, (name, in_place, int((got != want).sum()), coded, wcoded)
    # one end only: the other keeps its row end or plain sweep
    inv.set_u8_trc(None)
    filt, packed, _ = pf.settings(h, w, comps, info, "quant")
    got, coded = pf.run_call(gpu, fwd, inv, src, info, packed, filt)
    s = pf.stream_of(gpu)
    n = src.size
    d_in = gpu.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    wk = gpu.empty(n, dtype=gpu.float32, device="cuda:0")
    out = gpu.zeros(n, dtype=gpu.uint8, device="cuda:0")
    cnt = gpu.zeros(1, dtype=gpu.int64, device="cuda:0")
    from dspfun_amd.engine import motion_filter_packed
    assert L.dspfft_u8_to_f32_trc(wk.data_ptr(), d_in.data_ptr(), n, trc, s) == 0
    plain[0].execute(wk.data_ptr(), stream=s)
    motion_filter_packed(wk, h, w, comps, F, packed, filt, d_coded=cnt.data_ptr(), stream=s)
    plain[1].execute(wk.data_ptr(), stream=s)
    assert L.dspfft_f32_to_u8(out.data_ptr(), wk.data_ptr(), info["out_mul"], n, s) == 0
    gpu.cuda.synchronize()
    assert np.array_equal(got.reshape(-1), out.cpu().numpy()) and coded == int(cnt.item())


# ---- 2. the stand-alone kernel against the planar one ----
@pytest.mark.parametrize("F,h,w,comps", [(2, 10, 18, 3), (2, 16, 12, 2), (3, 24, 40, 4), (2, 256, 80, 3)], ids=lambda v: str(v))
def test_the_stand_alone_kernel_equals_the_planar_filter_on_every_plane(gpu, F, h, w, comps):
    """the coefficients are those a forward transform of the clip leaves; 10 x 18 x 3 takes the scalar path, and so does every shape on a
    buffer 4 bytes off a multiple of 16"""
    from dspfun_amd import _lib
    from dspfun_amd.engine import Plan, motion_filter_packed, motion_packed_frame_plans
    torch = gpu
    L = _lib.load()
    fwd, inv, info = motion_packed_frame_plans(F, h, w, comps)
    src = pf.clip_of(F, h, w, comps)
    n = src.size
    s = pf.stream_of(torch)
    coeffs = torch.empty(n, dtype=torch.float32, device="cuda:0")
    assert L.dspfft_u8_to_f32(coeffs.data_ptr(), torch.from_numpy(np.array(src)).to("cuda:0").data_ptr(), n, s) == 0
    fwd.execute(coeffs.data_ptr(), stream=s)
    torch.cuda.synchronize()
    host = coeffs.cpu().numpy().reshape(src.shape)
    I3, I2 = C.c_int * 3, C.c_int * 2
    for name in pf.FILTERS[1:]:
        filt, packed, planes = pf.settings(h, w, comps, info, name)
        want, counts = np.empty_like(host), []
        for c, pl in enumerate(planes):
            plane = torch.from_numpy(np.ascontiguousarray(host[..., c])).to("cuda:0")
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            fp = Plan._filter_params(pl)
            for b in range(F):
                assert L.dspfft_motion_filter(plane.data_ptr() + 4 * b * h * w, I3(1, h, w), I2(h, w), fp.band_begin, fp.band_end, fp.damp, fp.boost, fp.threshold_lo,
                                              fp.threshold_hi, fp.preserve_dc, fp.grey_add, fp.quantizer, cnt.data_ptr(), s) == 0
            torch.cuda.synchronize()
            want[..., c] = plane.cpu().numpy()
            counts.append(int(cnt.item()))
        assert sum(counts) > 0 and (name == "quant" or len(set(counts)) > 1), (name, counts)          # the components were filtered differently
        for off in (0, 1):
            raw = torch.full((n + 2 * 1024 + off,), float("nan"), dtype=torch.float32, device="cuda:0")
            buf = raw[1024 + off:1024 + off + n]
            buf.copy_(coeffs)
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            motion_filter_packed(buf, h, w, comps, F, packed, filt, d_coded=cnt.data_ptr(), stream=s)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().reshape(src.shape)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, off, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            assert int(cnt.item()) == sum(counts), (name, off, int(cnt.item()), counts)
            edge = raw.cpu().numpy()
            assert np.isnan(edge[:1024 + off]).all() and np.isnan(edge[1024 + off + n:]).all(), "the kernel wrote outside the clip"


# ---- 3. against the reference's arithmetic ----
# Share of bytes that differ from the float64 reference for the PLANAR Plan.roundtrip_u8 calls with per-frame plans on the three component
# planes of motion_packed_frames_ref.ref_case (3 x 24 x 40, the seeds of ref_seeds()), per filter: tools/bench_motion_packed_frames.py
# --accuracy on the kernels of commit 208e796, the parent of the commit that added this file, which leaves the planar calls as they were
# (profiles/r19_motion_packed_frames.txt).
PLANAR_SHARE = {None: 0.0, "band": 0.0, "full": 0.0, "q": 0.0}
EXTRA_BYTES = 4


def test_the_call_against_the_float64_reference(gpu):
    """no byte differs by more than 1; the share that differs is at most 1.5 times the planar calls' on the same planes, plus 4 bytes (the
    rule of tests/test_motion_spec_packed_gpu.py: the interleaved row and column kernels round in the last place differently from the planar
    ones, and a byte moves only where a value sits at a rounding boundary); the coded count is the reference's to within the coefficients on
    a quantiser tie"""
    from dspfun_amd.engine import motion_packed_frame_plans
    fwd, inv, info = motion_packed_frame_plans(pf.REF_FRAMES, pf.REF_H, pf.REF_W, 3)
    sf, nm, _ = sr.constants(pf.REF_BLOCK)
    assert (sf, nm) == (info["scalefactor"], info["normalization"]) and info["out_mul"] == sf * nm * nm
    for kind in pf.REF_KINDS:
        clip, refs = pf.ref_case(kind)
        filt, packed = pf.ref_packed(kind, info)
        got, coded = pf.run_call(gpu, fwd, inv, clip, info, packed, filt)
        for ref in refs:
            sr.check_tie_share(ref, True)
        mx, diff, size = pf.ref_shares([got[..., k] for k in range(3)], refs)
        cap = 1.5 * PLANAR_SHARE[kind] * size + EXTRA_BYTES
        print(f"filter={kind}: {diff} of {size} bytes differ ({diff / max(size, 1):.5%}), max difference {mx}, cap {cap:.1f} bytes")
        assert mx <= 1, (kind, mx)
        assert diff <= cap, (kind, diff, size, cap)
        if kind in ("full", "q"):
            want = sum(r["coded"] for r in refs)
            slack = sum(sr.coded_slack(dict(tie=r["coeff_tie"]), pf.REF_BLOCK) for r in refs)
            print(f"  coded {coded}, reference {want}, on a quantiser tie: {slack}")
            assert coded > 0 and abs(coded - want) <= slack, (kind, coded, want, slack)
        else:
            assert coded == 0


# ---- 4. refusals on the device library: nothing is written between the marker pages ----
def test_refusals_write_nothing(gpu):
    from dspfun_amd.engine import DspfftError, Plan, REDFT01, REDFT10, motion_grid_plans, motion_packed, motion_packed_frame_plans
    torch = gpu
    h, w = 12, 20
    fwd, inv, info = motion_packed_frame_plans(2, h, w, 3)
    n4 = 16 * 16 * 88 * 4
    src = torch.full((n4,), 77, dtype=torch.uint8, device="cuda:0")
    raw = torch.full((n4 + 2 * 1024,), float("nan"), dtype=torch.float32, device="cuda:0")
    wk = raw[1024:1024 + n4]

    def refused(f, i, comps, match, work=True, filt=None):
        buf, out = pf.framed(torch, n4)
        p = motion_packed("rgb24")
        p.components = comps
        with pytest.raises(DspfftError, match=match):
            f.roundtrip_u8_packed_frames(i, src.data_ptr(), out.data_ptr(), wk.data_ptr() if work else 0, info["out_mul"], p, filter=filt, stream=pf.stream_of(torch))
        torch.cuda.synchronize()
        assert bool((buf == pf.MARK).all()) and bool(torch.isnan(raw).all()), match
    refused(fwd, inv, 3, "work buffer", work=False)
    refused(fwd, inv, 3, "bad filter parameters", filt=dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), preserve_dc=5))
    for comps in (1, 5):
        refused(fwd, inv, comps, "components must be 2, 3 or 4")
    refused(fwd, inv, 4, "unit-stride batch level counts 3")
    f64 = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=2, idist=h * w, odist=h * w, dtype="f64")
    refused(f64, inv, 3, "f32 plans")
    sf, si, _ = motion_grid_plans((16, 16, 88), (8, 8, 8), (8, 8, 8))
    refused(sf, si, 3, "dspfft_execute_roundtrip_u8_packed")
    cube = lambda kind: Plan.guru([(6, 720, 720), (12, 60, 60), (20, 3, 3)], [(3, 1, 1)], [kind] * 3, first_axis_first=kind == REDFT01)
    refused(cube(REDFT10), cube(REDFT01), 3, "one 3-D block")
    refused(fwd, motion_packed_frame_plans(2, h, w + 4, 3)[1], 3, "different forward / inverse extents")
    padded = Plan.guru([(h, 66, 66), (w, 3, 3)], [(3, 1, 1), (2, h * 66, h * 66)], [REDFT10] * 2)
    refused(padded, inv, 3, "dense in-place layout")
    oop = Plan.guru([(h, 60, 60), (w, 3, 3)], [(3, 1, 1), (2, 720, 1440)], [REDFT01] * 2, first_axis_first=True)
    refused(fwd, oop, 3, "dense in-place layout")
    refused(inv, inv, 3, "REDFT10 .forward. and REDFT01 .inverse.")
    row_first = Plan.guru([(h, w * 3, w * 3), (w, 3, 3)], [(3, 1, 1), (2, h * w * 3, h * w * 3)], [REDFT01] * 2)
    refused(fwd, row_first, 3, "column pass first")
    # the small-block entry goes on refusing the per-frame pair
    buf, out = pf.framed(torch, n4)
    with pytest.raises(DspfftError, match="per-frame and single-block plans have no block pass"):
        fwd.roundtrip_u8_packed(inv, src.data_ptr(), out.data_ptr(), info["out_mul"], motion_packed("rgb24"), stream=pf.stream_of(torch))
    torch.cuda.synchronize()
    assert bool((buf == pf.MARK).all())
