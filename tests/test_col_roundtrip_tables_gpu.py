"""GPU (-m gpu): the fused column roundtrip with its twiddle tables in LDS (spec_fused.h, ColSpecT::RT_TABLES) against the same call run
pass by pass under DSPFFT_NO_FUSED_ROUNDTRIP=1 (read per call), BIT FOR BIT.  The unfused column kernels load every twiddle from the plan's
tables in global memory, so a table entry staged at the wrong place, read at the wrong offset or read before the barrier that publishes it
changes bits here.

Heights: 256 on (16, 16) (one twiddled stage), 540 on (12, 5, 9), 1080 x 16 and 2160 x 8 (the benchmark's tiles), 4320 on (2, 12, 12, 15)
with K = 8 and K = 4 (three twiddled stages; their tables do not fit, so these are the listed tiles that keep their global loads) and 364 =
4 x 7 x 13, compiled at plan time.  Every image is three tiles wide and two frames deep: six workgroups.  Each height runs as an
execute_many forward/inverse pair, as roundtrip with a quantiser (the coded-coefficient count, kept in LDS beside the tables, must equal the
unfused count) and through the packed twin with another damp per component on rgb24."""
import numpy as np
import pytest

import oracle_lib as ol
import motion_packed_frames_ref as pf
from test_motion_packed_frames_gpu import unfused

pytestmark = pytest.mark.gpu

# (height, tile width K, threads T or None for a kernel compiled at plan time, tables in LDS)
HEIGHTS = [
    (256, 32, 128, True),
    (540, 16, 256, True),
    (1080, 16, 512, True),
    (2160, 8, 512, True),
    (4320, 8, 1024, False),
    (4320, 4, 512, False),
    (364, 16, None, True),
]
IDS = [f"{h}x{k}" for h, k, _, _ in HEIGHTS]
FRAMES = 2


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from dspfun_amd import _lib
    _lib.load()
    return torch


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one DSPFFT_JIT_CACHE for the module: the three tests of the plan-time height compile its kernels once"""
    return tmp_path_factory.mktemp("jit")


@pytest.fixture
def plan_env(monkeypatch, jit_cache):
    """what a height's plans are made under: DSPFFT_JIT=1 (read at plan time) where its kernel is compiled at plan time"""
    def set_for(t):
        if t is None:
            monkeypatch.setenv("DSPFFT_JIT", "1")
            monkeypatch.setenv("DSPFFT_JIT_CACHE", str(jit_cache))
    return set_for


def fused_launches():
    from dspfun_amd import _lib
    return int(_lib.load().dspfft_col_roundtrip_launches())


def check_column_kernel(plans, h, k, t, tables):
    """both plans run axis 0 on the column kernel of that tile: listed (COL*) or compiled at plan time (COL+)"""
    for plan in plans:
        col = [l for l in plan.describe().splitlines() if l.startswith("axis 0")]
        assert len(col) == 1, plan.describe()
        assert ("COL*" if t else "COL+") in col[0] and f" N={h} K={k} " in col[0], plan.describe()
        if t:
            assert f"threads={t} " in col[0], plan.describe()
        else:
            # the type compiled at plan time, "ColSpecT<float, N, K, T, radices...>": its tables fit by the rule the CPU test recomputes
            import re
            from test_col_roundtrip_tables_cpu import expected
            m = re.search(r"ColSpecT<float, (\d+), (\d+), (\d+)((?:, \d+)+)>", col[0])
            assert m and (int(m.group(1)), int(m.group(2))) == (h, k), col[0]
            radices = tuple(int(v) for v in m.group(4).split(",")[1:])
            assert (expected(h, k, radices) > 0) == tables, col[0]


def test_the_tiles_are_the_ones_the_library_reports(gpu):
    from dspfun_amd import _lib
    L = _lib.load()
    for h, k, t, tables in HEIGHTS:
        if t:
            assert (L.dspfft_col_roundtrip_table_bytes(h, k, t) > 0) == tables, (h, k, t)


def planar_plans(h, w):
    from dspfun_amd import Plan, REDFT10, REDFT01
    kw = dict(howmany=FRAMES, idist=h * w, odist=h * w)
    fwd = Plan.many_r2r([h, w], [REDFT10] * 2, **kw)
    inv = Plan.many_r2r([h, w], [REDFT01] * 2, first_axis_first=True, **kw).set_scale(1.0 / (4.0 * w * h))
    return fwd, inv


def clip(h, w):
    return ol.synth_u8(0xC01 + h, FRAMES * h * w).astype(np.float32).reshape(FRAMES, h, w)


@pytest.mark.parametrize("h,k,t,tables", HEIGHTS, ids=IDS)
def test_a_forward_inverse_pair_of_execute_many(gpu, plan_env, h, k, t, tables):
    from dspfun_amd.engine import Batch, Stream, many_fused_pairs
    w = 3 * k
    plan_env(t)
    fwd, inv = planar_plans(h, w)
    check_column_kernel((fwd, inv), h, k, t, tables)
    x = clip(h, w)
    stream = Stream()

    def run():
        d = gpu.from_numpy(x.copy()).to("cuda:0")
        gpu.cuda.synchronize()
        n0 = many_fused_pairs()
        Batch([(fwd, d.data_ptr(), None, stream.handle), (inv, d.data_ptr(), None, stream.handle)]).run()
        stream.synchronize()
        return d.cpu().numpy(), many_fused_pairs() - n0

    got, fused = run()
    with unfused():
        want, none = run()
    assert (fused, none) == (1, 0)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.abs(got - x).max() < 2e-3                       # and it is a roundtrip of samples of 0 .. 255 (the bound tests/test_gpu_parity.py pins)


@pytest.mark.parametrize("h,k,t,tables", HEIGHTS, ids=IDS)
def test_roundtrip_with_a_quantiser_and_its_coded_count(gpu, plan_env, h, k, t, tables):
    w = 3 * k
    plan_env(t)
    fwd, inv = planar_plans(h, w)
    check_column_kernel((fwd, inv), h, k, t, tables)
    x = clip(h, w)
    # unnormalised coefficients of bytes: a step that zeroes a good part of them and keeps the rest
    flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), damp=0.5, boost=1.0,
               quantizer=300.0 * float(np.sqrt(h * w)))

    def run():
        d = gpu.from_numpy(x.copy()).to("cuda:0")
        coded = gpu.zeros(1, dtype=gpu.int64, device="cuda:0")
        n0 = fused_launches()
        fwd.roundtrip(inv, d.data_ptr(), filter=flt, d_coded=coded.data_ptr())
        gpu.cuda.synchronize()
        return d.cpu().numpy(), int(coded.item()), fused_launches() - n0

    got, coded, fused = run()
    with unfused():
        want, wcoded, none = run()
    assert fused >= 1 and none == 0                            # the first call ran the fused kernel (once per slice of the clip), the second did not
    print(f"{h} x {w} x {FRAMES}: {coded} of {x.size} coefficients coded")
    assert 0 < wcoded < x.size
    assert coded == wcoded
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("h,k,t,tables", HEIGHTS, ids=IDS)
def test_the_packed_twin_with_a_damp_per_component(gpu, plan_env, h, k, t, tables):
    from dspfun_amd.engine import motion_packed, motion_packed_frame_plans
    w = k                                                      # rgb24: 3 k samples a row, three tiles that straddle pixels
    plan_env(t)
    fwd, inv, info = motion_packed_frame_plans(FRAMES, h, w, 3)
    check_column_kernel((fwd, inv), h, k, t, tables)
    src = pf.clip_of(FRAMES, h, w, 3)
    q = pf.quantizer_of(h, w)
    flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 1, 0), band_end=(1, h, w), threshold_lo=q / 8, threshold_hi=1e30,
               preserve_dc=1, quantizer=q, damp=99.0, boost=99.0, grey_add=99.0)     # (the packed call takes damp, boost and grey_add per component)
    packed = motion_packed("rgb24", boost=pf.BOOST[:3], damp=pf.DAMP[:3], dcstop=True, normalization=info["normalization"], scalefactor=info["scalefactor"])
    n0 = fused_launches()
    got, coded = pf.run_call(gpu, fwd, inv, src, info, packed, flt)
    n1 = fused_launches()
    with unfused():
        want, wcoded = pf.run_call(gpu, fwd, inv, src, info, packed, flt)
    # the packed twin is a listed kernel's only: the height compiled at plan time runs the call's unfused sequence both times
    assert (n1 - n0 >= 1) == (t is not None) and fused_launches() == n1
    assert 0 < wcoded < src.size and len(np.unique(want)) > 8
    assert coded == wcoded
    assert np.array_equal(got, want), int((got != want).sum())
