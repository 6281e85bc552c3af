"""CPU: the non-dense geometries of tests/geometry_cases.py through the test-only emulation backend, against the oracle.

Three things are established here, before anyone spends GPU time on the table (tests/test_geometry_gpu.py runs the same cases through the
HIP library):
  1. the reference itself: the port's handling of differing input and output layouts agrees with the direct definition;
  2. every case is valid: its output positions do not overlap, the planner routes it to the family the case names, the emulation of
     the kernel phases computes the oracle's result, leaves every position outside the plan's index set and an out-of-place input alone;
  3. every X(...) entry of spec_list.h has a case that selects it.
A case that fails here is a planner (or case) error; one that fails only on the device is a device addressing error."""
import numpy as np
import pytest

import geometry_cases as gc
import oracle_lib as ol
from emul_lib import emul

REDFT10, REDFT01 = ol.REDFT10, ol.REDFT01


def _aligned(n, dtype):
    """the listed kernels need 16-byte aligned buffers: a numpy allocation does not promise that"""
    it = np.dtype(dtype).itemsize
    raw = np.empty(n * it + 64, dtype=np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + n * it].view(dtype)


# ---- 1. the reference: impl="port" against impl="direct" with differing input and output geometry (lengths <= 60) ----
PORT_FORMS = [
    # name, n, howmany, (inembed, istride, idist), (onembed, ostride, odist)
    ("same padded layout", [24], 5, ([24], 1, 29), ([24], 1, 29)),
    ("other pitch and dist on the output", [12, 20], 3, ([12, 23], 1, 12 * 23 + 5), ([12, 28], 1, 12 * 28 + 9)),
    ("rows in, columns out", [37], 7, ([37], 1, 41), ([37], 9, 1)),
    ("columns in, rows out", [60], 6, ([60], 7, 1), ([60], 1, 64)),
    ("interleaved in, planar out", [10, 18], 3, ([10, 18], 3, 1), ([10, 21], 1, 10 * 21 + 4)),
    ("planar in, interleaved out", [9, 16], 4, ([9, 17], 1, 9 * 17 + 2), ([9, 16], 4, 1)),
    ("rank 3, other embedding out", [6, 5, 8], 2, ([6, 7, 9], 1, 6 * 7 * 9 + 3), ([6, 5, 12], 1, 6 * 5 * 12)),
]


@pytest.mark.parametrize("form", PORT_FORMS, ids=[f[0] for f in PORT_FORMS])
@pytest.mark.parametrize("kind", [REDFT10, REDFT01])
def test_port_matches_direct_with_differing_layouts(form, kind):
    _, n, howmany, (ie, istr, idist), (oe, ostr, odist) = form
    kinds = [kind if a % 2 == 0 else (REDFT10 + REDFT01 - kind) for a in range(len(n))]       # mixed kinds across the axes
    nin = ol._span(n, ie, istr, idist, howmany) + 3
    nout = ol._span(n, oe, ostr, odist, howmany) + 3
    x = ol.synth_f32(len(n) * 100 + howmany, nin).astype(np.float64) - 0.5
    sentinel = -1000.0 - np.arange(nout)
    kw = dict(howmany=howmany, inembed=ie, istride=istr, idist=idist, onembed=oe, ostride=ostr, odist=odist, out=sentinel)
    direct = ol.r2r_many(x, n, kinds, impl="direct", **kw)
    port = ol.r2r_many(x, n, kinds, impl="port", **kw)
    # positions the transform owns in the output
    idx = np.zeros(1, dtype=np.int64)
    mult = ostr
    for a in range(len(n) - 1, -1, -1):
        idx = (idx[None, :] + (np.arange(n[a]) * mult)[:, None]).ravel()
        mult *= oe[a]
    idx = (idx[None, :] + (np.arange(howmany) * odist)[:, None]).ravel()
    assert np.unique(idx).size == idx.size == howmany * int(np.prod(n))
    own = np.zeros(nout, dtype=bool); own[idx] = True
    assert np.array_equal(direct[~own], sentinel[~own]) and np.array_equal(port[~own], sentinel[~own])
    assert not np.any(direct[own] == sentinel[own])
    assert np.abs(port[own] - direct[own]).max() <= 1e-12 * np.abs(direct[own]).max()
    # and the gather / scatter reference the case table uses is the same computation
    how = [(howmany, idist, odist)] if howmany > 1 else []
    dims, si, so = [], istr, ostr
    for a in range(len(n) - 1, -1, -1):
        dims.insert(0, (n[a], si, so))
        si *= ie[a]; so *= oe[a]
    case = gc.Case("form", "form", dims, how, kinds, [], dtype="f64")
    xin = np.zeros(case.size(1)); xin[:min(nin, xin.size)] = x[:xin.size]
    ref = case.reference(xin)
    assert np.abs(ref.ravel() - direct[idx]).max() <= 1e-12 * np.abs(direct[own]).max()


# ---- 2. the table through the emulation ----
def test_table_covers_every_family_and_direction():
    fam = gc.family_counts()
    for want in ("TINY packed", "TINY", "ROW generic LPW>1", "ROW*", "ROW* channel lines", "COL generic tail tile", "COL generic misaligned pitch",
                 "COL generic transposing", "COL*", "BLUE", "DENSE", "DENSE staged", "BLOCK block-major", "BLOCK side by side", "ROW+ (JIT)", "COL+ (JIT)",
                 "ROW*2 + COL*/2 (split)", "ROW* + COL* (frames)", "volume (COL* 256)"):
        assert fam.get(want, 0) > 0, (want, fam)
    cases = gc.all_cases()
    for family in set(c.family for c in cases if not c.family.startswith("entry")):
        mine = [c for c in cases if c.family == family]
        assert any(c.scaled_axis is not None for c in mine) or "split" in family, f"{family}: no case with fused scales"
    for c in cases:
        assert c.samples <= (2 << 20) or c.family in ("ROW*2 + COL*/2 (split)", "ROW* + COL* (frames)"), (c.name, c.samples)
    # every rank-1 family runs out of place with its own output layout somewhere, and in place somewhere
    assert any(not c.inplace and any(d[1] != d[2] for d in c.dims + c.how) for c in cases)


@pytest.mark.parametrize("case", gc.all_cases(), ids=gc.case_ids())
def test_case_through_the_emulation(case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    p = case.plan(lib=emul())
    case.check_describe(p.describe(), emulation=True)
    own = case.owned(2)
    assert int(own.sum()) == case.samples, "output positions overlap"
    assert int(case.owned(1).sum()) == case.samples, "input positions overlap"
    if case.emul == "describe":
        return
    x0 = case.make_input()
    x = _aligned(x0.size, x0.dtype); x[...] = x0
    if case.inplace:
        p.execute(x.ctypes.data)
        gc.verify(case, x0, x, None, None)
    else:
        o0 = case.make_output()
        o = _aligned(o0.size, o0.dtype); o[...] = o0
        p.execute(x.ctypes.data, o.ctypes.data)
        gc.verify(case, x0, x, o0, o)


# ---- 3. spec_list.h: one case per entry ----
def test_every_spec_list_entry_has_a_case():
    cases, unreachable = gc.entry_cases()
    assert not unreachable, "spec_list.h entries no generated geometry selects: " + "; ".join(unreachable)
    assert len(cases) == gc.entry_count(), (len(cases), gc.entry_count())
    assert len(set(c.name for c in cases)) == len(cases)
    # the parser misses nothing: every X( of the file outside comments belongs to one of the macros it knows or to the lists this table
    # does not cover (half tiles, row pairs, zoom's and the chirp-z rows: their own tests)
    import re
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(gc.SPEC_LIST).read(), flags=re.S))
    others = 0
    for macro in ("DSPFFT_COL_HALF_SPECS", "DSPFFT_ROW_PAIR_SPECS", "DSPFFT_ZOOMX_SPECS", "DSPFFT_CZT_SPECS"):
        body = re.search(r"#define\s+" + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text).group(1)
        others += len(re.findall(r"X\(", body))
    assert len(re.findall(r"\bX\(\d", text)) == gc.entry_count() + others
