"""GPU (-m gpu): every transform length without a prime factor above 13 on the device (tests/length_cases.py), against the f64 port.

The other device tests run lengths that are products of 2, 3 and 5, or go through Bluestein; here the radix-7, -11 and -13 butterflies
run in every stage position of the runtime-geometry ROW and COL passes, of the kernels compiled at plan time and of the temporal block
kernel.  tests/test_lengths_cpu.py has shown every case right under the CPU emulation, so a failure here is the device's: code
generation of the 11- and 13-point butterflies, register arrays of 13 complex doubles, the static LDS tiles of unlisted shapes, thread
counts at odd tile sizes.

Every transform case is the "prime-nb01" variant of tests/geometry_cases.py where the shape allows it -- padded lines, nb0 and nb1 with
different gaps, out of place into another pitch, fused scales, a sentinel check of every position outside the index set -- and goes
through geometry_cases.verify.  The radices a case exercises are read from describe() and pinned to the restatement first.  Each test
prints one `GEOMETRY sweep` line per family with the worst error and the lengths that ran under that family."""
import math

import numpy as np
import pytest

import geometry_cases as gc
import length_cases as lc
import motion_grid_ref as gr
import motion_ref as mr
import motion_temporal_ref as tr
import oracle_lib as ol
from test_geometry_gpu import _run
from test_motion_temporal_gpu import run_u8, run_f32

pytestmark = pytest.mark.gpu
DTYPES = ["f32", "f64"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()   # fails loudly if the HIP library was not built
    return torch


def _check(torch, case):
    """run one case where describe() places it -> (max, rms)"""
    x0, x1, o0, o1 = _run(torch, case)
    return gc.verify(case, x0, x1, o0, o1)


def _describe(case):
    text = case.plan().describe()
    case.check_describe(text)
    return text


# ---- (a) ROW and COL on every length ----
@pytest.mark.parametrize("chunk", lc.chunks(lc.SMOOTH13), ids=lc.chunk_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_col_at_every_smooth_length(gpu, dtype, chunk, monkeypatch):
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    worst = lc.Worst()
    for N in chunk:
        for kind in lc.KINDS:
            case = lc.sweep_col(N, dtype, kind)
            text = _describe(case)
            assert lc.family_of(text) == "COL", text
            lc.pin_fft(text, N)
            worst.add("COL", dtype, N, *_check(gpu, case))
    worst.report("device")


@pytest.mark.parametrize("chunk", lc.chunks(lc.ROW_LENGTHS), ids=lc.chunk_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_at_every_even_smooth_length(gpu, dtype, chunk, monkeypatch):
    """C = 1 everywhere, C = 3 on the subset that still reaches every (radix, position) of L = N / 2; a length with a listed ROW* kernel
    runs there and is counted under that family"""
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    worst = lc.Worst()
    for N in chunk:
        for C in (1, 3) if N in lc.ROW_C3_LENGTHS else (1,):
            for kind in lc.KINDS:
                case = lc.sweep_row(N, C, dtype, kind)
                text = _describe(case)
                family = lc.family_of(text)
                assert family in ("ROW", "ROW*"), text
                if family == "ROW":
                    lc.pin_fft(text, N // 2)
                worst.add(f"{family} C={C}", dtype, N, *_check(gpu, case))
    worst.report("device")


def test_the_sweeps_reach_every_radix_in_every_position(gpu, monkeypatch):
    """from the strings describe() returns for the swept plans on this library: length_cases.COL_TABLE for COL, its analogue for ROW's L = N / 2
    (C = 1, and again over the C = 3 subset)"""
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    col = [lc.pin_fft(_describe(lc.sweep_col(N, "f32", gc.K10)), N) for N in lc.SMOOTH13]
    assert lc.table(lc.coverage(col)) == lc.COL_TABLE
    assert max(len(r) for r in col) == 4
    for C, lengths in ((1, lc.ROW_LENGTHS), (3, lc.ROW_C3_LENGTHS)):
        for dtype in DTYPES:
            row, listed = [], []
            for N in lengths:
                text = _describe(lc.sweep_row(N, C, dtype, gc.K10))
                if lc.family_of(text) == "ROW":
                    row.append(lc.pin_fft(text, N // 2))
                else:
                    listed.append(N)
            got = lc.table(lc.coverage(r for r in row if r))
            if C == 1:
                assert got == lc.ROW_TABLE, (dtype, listed)
            else:       # (N = 512, C = 3 has a listed kernel, and L = 256 = 16 x 16 is the only length with a radix 16 first)
                assert {r: got.get(r) for r in range(5, 14)} == {r: lc.ROW_TABLE[r] for r in range(5, 14)}, (dtype, listed, got)
            print(f"GEOMETRY sweep device ROW C={C} {dtype}: {len(row)} lengths on the runtime-geometry kernel, listed ROW* kernels at {listed}")
    for r in (7, 11, 13):
        assert lc.COL_TABLE[r] == lc.ROW_TABLE[r] == "only, first, mid, last"


# ---- (b) TINY ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_at_every_length(gpu, dtype):
    worst = lc.Worst()
    for N in lc.TINY:
        for kind in lc.KINDS:
            for case in lc.tiny_cases(N, dtype, kind):
                text = _describe(case)
                assert lc.family_of(text) == "TINY", text
                worst.add(case.family, dtype, N, *_check(gpu, case))
    worst.report("device")


# ---- (c) BLUE ----
@pytest.mark.parametrize("chunk", lc.chunks(lc.ROUGH, 64), ids=lc.chunk_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bluestein_at_every_rough_length(gpu, dtype, chunk, monkeypatch):
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")          # 17 ... 31 reach Bluestein only past the TINY pass
    worst = lc.Worst()
    for N in chunk:
        for kind in lc.KINDS:
            case = lc.sweep_blue(N, dtype, kind)
            text = _describe(case)
            conv = lc.pin_conv(text, N)
            assert not set(conv) & {11, 13}, text          # the inverse stages have no case for them
            worst.add("BLUE", dtype, N, *_check(gpu, case))
    worst.report("device")


def test_bluestein_convolution_radices(gpu, monkeypatch):
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    conv = set()
    for N in lc.ROUGH:
        conv |= set(lc.pin_conv(_describe(lc.sweep_blue(N, "f32", gc.K10)), N))
    assert {5, 6, 7, 8, 9, 10, 12, 15, 16} <= conv and not conv & {11, 13}, conv
    print(f"GEOMETRY sweep device BLUE: convolution radices over N in [17, 700): {sorted(conv)}")


# ---- (d) kernels compiled at plan time ----
@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one DSPFFT_JIT_CACHE for the module: the coverage test below plans the same kernels again and finds them compiled"""
    return tmp_path_factory.mktemp("jit")


def _jit_id(p):
    return f"{p[0]} N={p[1]}" + (f" C={p[2]}" if p[2] else "") + f" {p[3]}"


@pytest.mark.parametrize("param", lc.jit_params(), ids=_jit_id)
def test_plan_time_kernels_with_radix_7_11_13(gpu, param, monkeypatch, jit_cache):
    family, N, C, dtype = param
    monkeypatch.setenv("DSPFFT_JIT", "1")
    monkeypatch.setenv("DSPFFT_JIT_CACHE", str(jit_cache))
    worst = lc.Worst()
    for case in lc.jit_cases(family, N, C, dtype):
        text = _describe(case)
        assert lc.family_of(text) == family, text
        rad = lc.pin_spec(text, "Col" if family == "COL+" else "Row", lc.jit_fft_length(family, N))
        worst.add(f"{family} {'x'.join(map(str, rad))}", dtype, N, *_check(gpu, case))
    worst.report("device")


def test_plan_time_kernels_reach_7_11_13_first_mid_and_last(gpu, monkeypatch, jit_cache):
    monkeypatch.setenv("DSPFFT_JIT", "1")
    monkeypatch.setenv("DSPFFT_JIT_CACHE", str(jit_cache))
    for family in ("COL+", "ROW+"):
        cov = set()
        for fam, N, C, dtype in lc.jit_params():
            if fam == family and dtype == "f32":
                case = lc.jit_cases(family, N, C, dtype, tags=["one"])[0]
                rad = lc.parse_spec(_describe(case))
                assert len(rad) == 1, case.name
                cov |= lc.positions(rad[0][5])
        missing = {(r, p) for r in (7, 11, 13) for p in ("first", "mid", "last")} - cov
        assert not missing, (family, missing)
        print(f"GEOMETRY sweep device {family}: type strings reach {lc.table(cov)}")


# ---- (e) the compiled fused 8-bit pipeline at a radix-13 frame ----
FUSED_HW = (286, 364)           # columns 286 = 2 x 11 x 13; rows L = 182 = 2 x 7 x 13, 364 a multiple of 4
FUSED_FRAMES = 3
FUSED_QUANT = 74.0 / 0.15       # motion_temporal_ref's coarse quantiser: 0.15 standard deviations a step


def fused_case():
    """3 luma frames and the f64 chain of motion_ref.block_roundtrip per frame (motion_grid_ref.oracle with blocks of one frame); the
    seed is the first for which no coefficient / quantiser comes within motion_grid_ref.EDGE of a rounding boundary"""
    h, w = FUSED_HW
    ext = (1, h, w)
    q = float(np.float32(gr.quantizer_of(FUSED_QUANT, ext)))        # the float the C ABI takes ...
    quant = q / gr.quantizer_of(1.0, ext)                            # ... and the --quant that gives it (motion.c:570 backwards)
    for seed in range(500, 900):
        vol = ol.synth_u8(seed, FUSED_FRAMES * h * w).reshape(FUSED_FRAMES, h, w)
        _, _, act0 = gr.oracle(vol, ext, ext, 0.0)
        t = act0 / q
        edge = float(np.abs(np.abs(t - np.floor(t)) - 0.5).min())
        if edge <= gr.EDGE:
            continue
        out8, pel, act = gr.oracle(vol, ext, ext, quant)
        return dict(vol=vol, out8=out8, pel=pel, coded=int(np.count_nonzero(act)), edge=edge, quantizer=q)
    raise AssertionError("no seed keeps the coefficients off the quantiser's rounding boundaries")


def test_plan_time_kernels_run_motions_fused_pipeline_at_a_radix_13_frame(gpu, monkeypatch, tmp_path):
    """test_plan_time_kernels_run_motions_fused_pipeline's plan pair (tests/test_gpu_parity.py) with motion's scales, compiled (DSPFFT_JIT=1)
    and on the runtime-geometry kernels (=2), each against the f64 chain: bytes equal wherever the f64 pixel is farther than
    motion_temporal_ref.TOL from k + 1/2, within 1 elsewhere; the coded count exact"""
    from dspfun_amd import Plan, REDFT10, REDFT01
    monkeypatch.setenv("DSPFFT_JIT_CACHE", str(tmp_path / "jit"))
    h, w = FUSED_HW
    n = FUSED_FRAMES
    ref = fused_case()
    assert ref["edge"] > gr.EDGE and ref["coded"] > 0
    near = tr.near_half(ref["pel"])
    assert near.mean() <= 0.01
    flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), quantizer=ref["quantizer"])
    r2 = math.sqrt(2.0)
    sf, nm = mr.consts((1, h, w), (1, h, w))
    for jit in ("1", "2"):
        monkeypatch.setenv("DSPFFT_JIT", jit)
        # motion's scales for 2-D blocks (engine.motion_grid_plans: the unit axis of the reference's 3-D plans folded in)
        f2 = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=n, idist=h * w, odist=h * w).set_scale(2 * r2 * r2)
        i2 = Plan.many_r2r([h, w], [REDFT01] * 2, howmany=n, idist=h * w, odist=h * w, first_axis_first=True).set_scale(r2 / (2 * r2))
        for a in range(2):
            f2.set_axis_scale0(a, 1.0, 1.0 / r2)
            i2.set_axis_scale0(a, r2, 1.0)
        text = f2.describe()
        assert (text.count("compiled at plan time") == 2) == (jit == "1"), text
        if jit == "1":
            specs = {s[0]: s[5] for s in lc.parse_spec(text)}
            assert specs == {"Row": lc.jit_radices(lc.factorize(w // 2)), "Col": lc.jit_radices(lc.factorize(h))}, text
            assert 13 in specs["Row"] and 13 in specs["Col"]
        din = gpu.from_numpy(ref["vol"].copy()).to("cuda:0"); dout = gpu.zeros_like(din); work = gpu.empty(n * h * w, dtype=gpu.float32, device="cuda:0")
        coded = gpu.zeros(1, dtype=gpu.int64, device="cuda:0")
        f2.roundtrip_u8(i2, din.data_ptr(), dout.data_ptr(), work.data_ptr(), sf * nm * nm, filter=flt, d_coded=coded.data_ptr())
        gpu.cuda.synchronize()
        got = dout.cpu().numpy()
        diff = np.abs(got.astype(int) - ref["out8"].astype(int))
        print(f"GEOMETRY sweep device fused 8-bit pipeline {w}x{h} DSPFFT_JIT={jit}: {int((diff > 0).sum())} of {diff.size} bytes differ, max {diff.max()}; "
              f"{int(near.sum())} oracle pixels within {tr.TOL:.2e} of a half; coded {int(coded.item())} / {ref['coded']}")
        assert diff[~near].max() == 0 and diff.max() <= 1, (jit, int((diff[~near] > 0).sum()), int(diff.max()))
        assert int(coded.item()) == ref["coded"], (jit, int(coded.item()), ref["coded"])


# ---- (f) the temporal kernel ----
def _temporal_pin(D, monkeypatch):
    """the radices of the temporal kernel's FFT of D points are the column pass's: describe() of the forward plan (under DSPFFT_NO_TINY up
    to 32 points, where the plan itself is a TINY pass)"""
    from dspfun_amd.engine import motion_temporal_plans
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    fwd, _, _ = motion_temporal_plans((D,) + lc.TEMPORAL_HW, D)
    rad = lc.pin_fft(fwd.describe(), D)
    monkeypatch.delenv("DSPFFT_NO_TINY")
    return rad


def _temporal(torch, D, S):
    """8-bit and float, band filter -> (float error in pixels, tolerance)"""
    ref = lc.temporal_case(D, S)
    tol = lc.temporal_tol(D, S, tr.TOL)
    got = run_u8(torch, D, S, ref["vol"], flt=ref["filter"])
    tr.check_bytes(got, ref, tol)
    sf, nm = mr.consts((D, 1, 1), (S, 1, 1))
    src = torch.from_numpy(np.asarray(ref["vol"], dtype=np.float32)).to("cuda:0")
    f = run_f32(torch, D, S, ref["vol"], src, flt=ref["filter"]).cpu().numpy().astype(np.float64) * sf * nm * nm
    err = float(np.abs(f - ref["pel"]).max())
    rms = float(np.sqrt(np.mean((f - ref["pel"]) ** 2)))
    print(f"GEOMETRY temporal {D}-{S} float, band filter: max={err:.3e} rms={rms:.3e} pixels tol={tol:.3e}")
    assert err <= tol, (D, S, err, tol)
    return err, rms


@pytest.mark.parametrize("chunk", lc.chunks(lc.SMOOTH13), ids=lc.chunk_id)
def test_temporal_at_every_smooth_length(gpu, chunk, monkeypatch):
    cov, worst = set(), (0.0, 0.0, 0)
    for D in chunk:
        cov |= lc.positions(_temporal_pin(D, monkeypatch))
        worst = max(worst, _temporal(gpu, D, D) + (D,))
    print(f"GEOMETRY sweep device family='temporal float' D=D' in {chunk}: worst max={worst[0]:.3e} rms={worst[1]:.3e} pixels at D={worst[2]}; reaches {lc.table(cov)}")


@pytest.mark.parametrize("D,S", lc.TEMPORAL_RESCALED, ids=[tr.pair_id(p) for p in lc.TEMPORAL_RESCALED])
def test_temporal_at_rescaled_pairs(gpu, D, S, monkeypatch):
    _temporal_pin(D, monkeypatch); _temporal_pin(S, monkeypatch)
    err, rms = _temporal(gpu, D, S)
    print(f"GEOMETRY sweep device family='temporal float' {D}-{S}: max={err:.3e} rms={rms:.3e} pixels")


def test_temporal_with_a_quantiser_at_every_radix_position(gpu, monkeypatch):
    cov = set()
    for D in lc.TEMPORAL_QUANT:
        cov |= lc.positions(_temporal_pin(D, monkeypatch))
        ref = lc.temporal_case(D, D, "quant")
        assert ref["edge"] > gr.EDGE and ref["coded"] > 0
        got, coded = run_u8(gpu, D, D, ref["vol"], flt=ref["filter"], coded=True)
        tr.check_bytes(got, ref, lc.temporal_tol(D, D, tr.TOL))
        assert coded == ref["coded"], (D, coded, ref["coded"])
    assert lc.table(cov) == lc.COL_TABLE
    print(f"GEOMETRY sweep device family='temporal quant' D=D' in {lc.TEMPORAL_QUANT}: coded counts exact; reaches {lc.table(cov)}")
