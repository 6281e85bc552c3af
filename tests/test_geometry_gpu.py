"""GPU (-m gpu): the non-dense geometries of tests/geometry_cases.py through the HIP library, against the f64 port.

The dense whole-frame tests cannot tell a batch stride from another or an output stride from an input one; these cases can: padded rows,
gaps between batches, nb0 / nb1 / host-loop batch levels, 1 / odd / ragged line counts, tail tiles, outputs laid out unlike the inputs.
tests/test_geometry_cpu.py has shown every case valid under the CPU emulation, so a failure here is a device addressing error.

Per case: describe() names the family BEFORE anything runs; every position outside the plan's index set is bit-identical afterwards (the
output buffer is pre-filled with a sentinel pattern, an in-place array keeps its gaps); an out-of-place input is bit-identical; the result
matches `oracle_lib.r2r_many(impl="port", threads=8)` in float64 within the tolerance of the dense test of the same family
(f32 1e-5 max and rms, f64 1e-13, f64 Bluestein 2e-13)."""
import numpy as np
import pytest

import geometry_cases as gc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

REDFT10, REDFT01 = ol.REDFT10, ol.REDFT01


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()   # fails loudly if the HIP library was not built
    return torch


def _setenv(case, monkeypatch, tmp_path):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if "DSPFFT_JIT" in case.env:
        monkeypatch.setenv("DSPFFT_JIT_CACHE", str(tmp_path / "jit"))


def _run(torch, case, stream=None):
    """-> (input before, input after, output before, output after) as host arrays; output_* are None in place"""
    x0 = case.make_input()
    d = torch.from_numpy(x0).to("cuda:0")
    p = case.plan()
    case.check_describe(p.describe())              # a case that lands on another kernel fails before it runs
    o0 = do = None
    if not case.inplace:
        o0 = case.make_output()
        do = torch.from_numpy(o0).to("cuda:0")
    torch.cuda.synchronize()
    handle = stream.cuda_stream if stream is not None else 0
    if case.inplace:
        p.execute(d.data_ptr(), stream=handle)
    else:
        p.execute(d.data_ptr(), do.data_ptr(), stream=handle)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return x0, d.cpu().numpy(), o0, (do.cpu().numpy() if do is not None else None)


@pytest.mark.parametrize("case", gc.all_cases(), ids=gc.case_ids())
def test_case_on_the_device(gpu, case, monkeypatch, tmp_path):
    _setenv(case, monkeypatch, tmp_path)
    x0, x1, o0, o1 = _run(gpu, case)
    gc.verify(case, x0, x1, o0, o1)


def _one_per_family():
    seen, out = set(), []
    for c in gc.all_cases():
        if c.family not in seen and not c.family.startswith("entry"):
            seen.add(c.family)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _one_per_family(), ids=[c.family for c in _one_per_family()])
def test_non_default_stream_gives_the_same_bits(gpu, case, monkeypatch, tmp_path):
    _setenv(case, monkeypatch, tmp_path)
    a = _run(gpu, case)
    b = _run(gpu, case, stream=gpu.cuda.Stream())
    for u, v in zip(a[1:], b[1:]):
        assert (u is None and v is None) or np.array_equal(u.view(np.uint8), v.view(np.uint8)), case.name
    gc.verify(case, *b)


def _along_axis(arr, axis, kind):
    """the port along one axis of a dense float64 array"""
    moved = np.ascontiguousarray(np.moveaxis(arr, axis, -1))
    n = moved.shape[-1]
    out = ol.r2r_many(moved.ravel(), [n], [kind], howmany=moved.size // n, idist=n, odist=n, impl="port", threads=8).reshape(moved.shape)
    return np.moveaxis(out, -1, axis)


@pytest.mark.parametrize("seed", range(16))
def test_random_guru_geometries_at_kernel_selecting_sizes(gpu, seed):
    """test_random_guru_geometries' shape (tests/test_kernel_logic_cpu.py) on the device with extents that select the listed, Bluestein and
    tile-tail kernels: a random subset of 1..3 axes of a dense array is transformed in place, the other axes are batch dimensions handed
    over in shuffled order.  Tolerance by sample type as in the table; a plan with a Bluestein pass gets that family's 2e-13 in double."""
    from dspfun_amd import Plan
    torch = gpu
    rng = np.random.default_rng(7000 + seed)
    nd = int(rng.integers(2, 6))
    shape = [int(rng.choice([2, 3, 8, 16, 37, 256, 540, 960, 1080])) for _ in range(nd)]
    while np.prod(shape, dtype=np.int64) > 4 << 20:
        shape[int(rng.integers(0, nd))] = int(rng.choice([2, 3, 8]))
    strides = [int(np.prod(shape[i + 1:], dtype=np.int64)) for i in range(nd)]
    rank = int(rng.integers(1, min(3, nd) + 1))
    taxes = sorted(rng.choice(nd, size=rank, replace=False).tolist())
    kinds = [int(rng.choice([REDFT10, REDFT01])) for _ in range(rank)]
    dims = [(shape[a], strides[a], strides[a]) for a in taxes]
    how = [(shape[a], strides[a], strides[a]) for a in range(nd) if a not in taxes]
    rng.shuffle(how)
    f64 = bool(seed % 2)
    x = ol.synth_f32(seed + 3, int(np.prod(shape))).reshape(shape)
    x = x.astype(np.float64) * (1 + 2.0 ** -30) if f64 else x
    p = Plan.guru(dims, how, kinds, dtype="f64" if f64 else "f32")
    desc = p.describe()
    d = torch.from_numpy(x).to("cuda:0")
    p.execute(d.data_ptr())
    torch.cuda.synchronize()
    ref = x.astype(np.float64)
    for a, k in zip(taxes, kinds):
        ref = _along_axis(ref, a, k)
    tol = gc.TOL_F32 if not f64 else gc.TOL_F64_BLUE if "BLUE" in desc else gc.TOL_F64
    m, r = gc.errors(d.cpu().numpy(), ref)
    print(f"GEOMETRY guru seed={seed} shape={shape} axes={taxes} kinds={kinds} {'f64' if f64 else 'f32'} max={m:.3e} rms={r:.3e} tol={tol:g}")
    assert m <= tol and r <= tol, (shape, taxes, kinds, m, r, desc)
