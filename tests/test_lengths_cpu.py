"""CPU: every transform length without a prime factor above 13 (tests/length_cases.py), before anyone spends device time on them.

  1. the table itself: which (radix, stage position) pairs the planner's order reaches over the 245 lengths, from the Python restatement;
  2. the restatement against `Plan.describe()` for every swept length (ROW, COL, Bluestein's convolution), and the coverage asserted
     from describe()'s own strings;
  3. the CPU emulation of the ROW and COL kernel phases at every length, both kinds, f32 and f64, against the f64 port: a failure of
     tests/test_lengths_gpu.py at a length that passes here is the device's;
  4. the temporal kernel's phases (tests/temporal_shim.py) at every D = D' and the rescaled pairs, with a band filter -- a plain D = D'
     roundtrip returns the integer input and cannot see an error below half a pixel -- and the held-register budget the phases rely on;
  5. the oracle's share of pixels within the tolerance of k + 1/2, from the oracle alone."""
import numpy as np
import pytest

import geometry_cases as gc
import length_cases as lc
import motion_grid_ref as gr
import motion_ref as mr
import motion_temporal_ref as tr
from emul_lib import emul
from temporal_shim import HOLD, core, run_core, expected_tile, shim_radices  # noqa: F401  (core is a fixture)


def _aligned(n, dtype):
    """16-byte aligned host buffers, as the device's are (a numpy allocation does not promise that)"""
    it = np.dtype(dtype).itemsize
    raw = np.empty(n * it + 64, dtype=np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + n * it].view(dtype)


# ---- 1. the table ----
def test_the_length_table_and_its_coverage():
    assert len(lc.SMOOTH13) == 245 and lc.SMOOTH13[0] == 2 and lc.SMOOTH13[-1] == 1024
    assert lc.ROUGH[0] == 17 and lc.ROUGH[-1] == 699 and not set(lc.ROUGH) & set(lc.SMOOTH13)
    stages = {n: lc.factorize(n) for n in lc.SMOOTH13}
    assert all(f is not None and int(np.prod(f)) == n and f == sorted(f) and set(f) <= set(lc.RADICES) for n, f in stages.items())
    assert max(len(f) for f in stages.values()) == 4 and stages[686] == [2, 7, 7, 7]
    assert lc.table(lc.coverage(stages.values())) == lc.COL_TABLE
    # the ROW pass's L = N / 2 over the even lengths
    rows = lc.table(lc.coverage(lc.factorize(n // 2) for n in lc.ROW_LENGTHS if n > 2))
    assert rows == lc.ROW_TABLE
    # (L <= 512 leaves no room for a radix 12 between two others: 2 x 12 x 12 = 288 is 6 x 6 x 8 to the planner)
    assert rows == {**lc.COL_TABLE, 12: "only, first, last"}
    assert lc.table(lc.coverage(lc.factorize(n // 2) for n in lc.ROW_C3_LENGTHS)) == rows and len(lc.ROW_C3_LENGTHS) <= 32
    assert lc.table(lc.coverage(lc.factorize(n) for n in lc.TEMPORAL_QUANT)) == lc.COL_TABLE and len(lc.TEMPORAL_QUANT) <= 32
    # the compiled kernels' order: largest first, an odd radix last
    assert [lc.jit_radices(lc.factorize(L)) for L in lc.JIT_L] == [[7, 2, 7], [13, 2, 11], [13, 2, 13], [7, 7, 7], [7, 7, 2, 7], [13, 11, 7], [11, 11, 11], [13, 13, 13]]
    cov = lc.coverage(lc.jit_radices(lc.factorize(L)) for L in lc.JIT_L)
    assert {(r, p) for r in (7, 11, 13) for p in ("first", "mid", "last")} <= cov
    # Bluestein's convolution lengths over its range: 7-smooth, so never a radix its inverse stages have no case for
    conv = set()
    for N in lc.ROUGH:
        M, f = lc.blue_length(N)
        assert 2 * N - 1 <= M and int(np.prod(f)) == M
        conv |= set(f)
    assert {5, 6, 7, 8, 9, 10, 12, 15, 16} <= conv and not conv & {11, 13}, conv


# ---- 2. the restatement against describe(), the coverage from describe()'s strings ----
def test_describe_names_the_restated_radices_and_covers_every_position(monkeypatch):
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    col, row, listed = [], [], []
    for N in lc.SMOOTH13:
        text = lc.sweep_col(N, "f32", gc.K10).plan(lib=emul()).describe()
        assert lc.family_of(text) == "COL", text
        col.append(lc.pin_fft(text, N))
    for N in lc.ROW_LENGTHS:
        for C in (1, 3):
            text = lc.sweep_row(N, C, "f32", gc.K10).plan(lib=emul()).describe()
            if lc.family_of(text) == "ROW*":
                listed.append((N, C))
            elif C == 1:
                row.append(lc.pin_fft(text, N // 2))
    assert lc.table(lc.coverage(col)) == lc.COL_TABLE
    assert lc.table(lc.coverage(r for r in row if r)) == lc.ROW_TABLE
    # the listed ROW* kernels in range are 5-smooth: they take nothing from radix 7, 11 or 13
    assert listed and all(lc._smooth(N, (2, 3, 5)) for N, _ in listed), listed
    conv = set()          # (17 ... 31 reach Bluestein only past the TINY pass)
    for N in lc.ROUGH:
        text = lc.sweep_blue(N, "f32", gc.K10).plan(lib=emul()).describe()
        conv |= set(lc.pin_conv(text, N))
    assert {5, 6, 7, 8, 9, 10, 12, 15, 16} <= conv and not conv & {11, 13}, conv


# ---- 3. the emulation at every length ----
def _emulate(case):
    p = case.plan(lib=emul())
    text = p.describe()
    case.check_describe(text, emulation=True)
    x0 = case.make_input()
    x = _aligned(x0.size, x0.dtype); x[...] = x0
    o0 = case.make_output()
    o = _aligned(o0.size, o0.dtype); o[...] = o0
    p.execute(x.ctypes.data, o.ctypes.data)
    return text, gc.verify(case, x0, x, o0, o)


@pytest.mark.parametrize("chunk", lc.chunks(lc.SMOOTH13, 64), ids=lc.chunk_id)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_col_emulation_at_every_smooth_length(dtype, chunk, monkeypatch):
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    worst = lc.Worst()
    for N in chunk:
        for kind in lc.KINDS:
            text, (m, r) = _emulate(lc.sweep_col(N, dtype, kind))
            lc.pin_fft(text, N)
            worst.add("COL", dtype, N, m, r)
    worst.report("emulation")


@pytest.mark.parametrize("chunk", lc.chunks(lc.ROW_LENGTHS, 64), ids=lc.chunk_id)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_row_emulation_at_every_even_smooth_length(dtype, chunk, monkeypatch):
    monkeypatch.setenv("DSPFFT_NO_TINY", "1")
    worst = lc.Worst()
    for N in chunk:
        for C in (1, 3) if N in lc.ROW_C3_LENGTHS else (1,):
            for kind in lc.KINDS:
                text, (m, r) = _emulate(lc.sweep_row(N, C, dtype, kind))
                family = lc.family_of(text)
                if family == "ROW":
                    lc.pin_fft(text, N // 2)
                worst.add(family, dtype, N, m, r)
    worst.report("emulation")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_tiny_emulation_at_every_length(dtype):
    """packed out of place with fused scales (a dense f64 input: the reference must leave it alone) and strided"""
    worst = lc.Worst()
    for N in lc.TINY:
        for kind in lc.KINDS:
            for case in lc.tiny_cases(N, dtype, kind):
                text, (m, r) = _emulate(case)
                assert lc.family_of(text) == "TINY", text
                worst.add(case.family, dtype, N, m, r)
    worst.report("emulation")


# ---- 4. the temporal kernel's phases ----
def _phases(core, D, S):
    """8-bit (the byte rule) and float (within the tolerance of the f64 pixels), both with a band filter -> the float error in pixels"""
    tile = lc.temporal_tile(D, S)
    assert tile == expected_tile(D, S)
    assert (D // 2 + 1) * (tile[0] // 2) <= HOLD * tile[1], (D, S, tile)          # the held post items fit the threads' registers
    assert shim_radices(core, D) == lc.factorize(D) and shim_radices(core, S) == lc.factorize(S)
    tol = lc.temporal_tol(D, S, tr.TOL)
    ref = lc.temporal_case(D, S)
    got, _, ran = run_core(core, ref, D, S, flt=ref["filter"])
    assert ran == tile
    tr.check_bytes(got, ref, tol)
    f, _, _ = run_core(core, ref, D, S, u8=False, flt=ref["filter"])
    sf, nm = mr.consts((D, 1, 1), (S, 1, 1))
    err = float(np.abs(f.astype(np.float64) * sf * nm * nm - ref["pel"]).max())
    assert err <= tol, (D, S, err, tol)
    return err


@pytest.mark.parametrize("chunk", lc.chunks(lc.SMOOTH13, 32), ids=lc.chunk_id)
def test_temporal_phases_at_every_smooth_length(core, chunk):
    worst = max((_phases(core, D, D), D) for D in chunk)
    print(f"GEOMETRY sweep shim family='temporal float' D=D' in {chunk}: worst {worst[0]:.3e} pixels at D={worst[1]}")


@pytest.mark.parametrize("D,S", lc.TEMPORAL_RESCALED, ids=[tr.pair_id(p) for p in lc.TEMPORAL_RESCALED])
def test_temporal_phases_at_rescaled_pairs(core, D, S):
    print(f"GEOMETRY sweep shim family='temporal float' {D}-{S}: {_phases(core, D, S):.3e} pixels")


def test_temporal_phases_with_a_quantiser_at_every_radix_position(core):
    """the coded count is the oracle's exactly: no coefficient / quantiser of the chosen clips lies within EDGE of a rounding boundary"""
    cov = set()
    for D in lc.TEMPORAL_QUANT:
        ref = lc.temporal_case(D, D, "quant")
        assert ref["edge"] > gr.EDGE and ref["coded"] > 0
        got, coded, _ = run_core(core, ref, D, D, flt=ref["filter"])
        tr.check_bytes(got, ref, lc.temporal_tol(D, D, tr.TOL))
        assert coded == ref["coded"], (D, coded, ref["coded"])
        cov |= lc.positions(shim_radices(core, D))
    assert lc.table(cov) == lc.COL_TABLE


# ---- 5. what the 8-bit rule leaves open, from the oracle alone ----
def test_few_oracle_pixels_of_the_swept_cases_lie_within_the_tolerance_of_a_half():
    """expected: about 2 tol = 0.05 % of the pixels; the cap is test_few_oracle_pixels_lie_within_the_tolerance_of_a_half's 1 %"""
    cases = [(D, D, "band") for D in lc.SMOOTH13] + [(D, S, "band") for D, S in lc.TEMPORAL_RESCALED] + [(D, D, "quant") for D in lc.TEMPORAL_QUANT]
    top = 0.0
    for D, S, kind in cases:
        ref = lc.temporal_case(D, S, kind)
        share = float(tr.near_half(ref["pel"], lc.temporal_tol(D, S, tr.TOL)).mean())
        assert share <= 0.01, (D, S, kind, share)
        top = max(top, share)
    print(f"largest share of oracle pixels within the tolerance of a half: {top:.3%}")
