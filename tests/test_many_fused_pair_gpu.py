"""GPU (-m gpu): forward/inverse pairs of dspfft_execute_many_repeat as one roundtrip (engine.cpp many_pair_check) on the listed column
kernels -- the smallest frames that reach the tile the 4K benchmark runs, 2160 x 8 x 3 (inner extent 24: three tiles of COL* N=2160 K=8) and
2160 x 64 x 3 (24 tiles: more than one per XCD after xcd_remap), and 1080 x 16 x 3 on the K = 16 tile.  Plans as bench.py builds them.
The fused pairs must equal the same plans run pass by pass BITWISE, the counter must say that they ran fused, and a timed window must leave
its items unfused with every one of their passes bracketed."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

SHAPES = [(2160, 8, 3, "N=2160 K=8"), (2160, 64, 3, "N=2160 K=8"), (1080, 16, 3, "N=1080 K=16")]
ROUNDTRIP_TOL = 5e-6              # one in-place roundtrip of samples in [0, 1): the bound tests/test_gpu_parity.py pins


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


def setup(gpu, h, w, c, spec):
    from dspfun_amd import Plan, REDFT10, REDFT01
    fwd = Plan.image(h, w, c, REDFT10)
    inv = Plan.many_r2r([h, w], [REDFT01] * 2, howmany=c, istride=c, idist=1, ostride=c, odist=1, first_axis_first=True).set_scale(1.0 / (4.0 * w * h))
    # the column pass is the listed kernel in both plans, last in the forward and first in the inverse
    fcol, icol = fwd.describe().splitlines()[-1], inv.describe().splitlines()[1]
    assert "COL*" in fcol and spec in fcol, fwd.describe()
    assert "COL*" in icol and spec in icol, inv.describe()
    x = [ol.synth_f32(0xD5F0100 + f, h * w * c).reshape(h, w, c) for f in range(2)]
    return fwd, inv, x


def by_passes(gpu, fwd, inv, x, times):
    d = gpu.from_numpy(x.copy()).to("cuda:0")
    s = gpu.cuda.current_stream().cuda_stream
    for _ in range(times):
        fwd.execute(d.data_ptr(), stream=s)
        inv.execute(d.data_ptr(), stream=s)
    gpu.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("h,w,c,spec", SHAPES)
def test_repeated_pairs_are_the_passes_bitwise(gpu, h, w, c, spec):
    from dspfun_amd.engine import Batch, Stream, many_fused_pairs
    fwd, inv, x = setup(gpu, h, w, c, spec)
    want = [by_passes(gpu, fwd, inv, f, 3) for f in x]
    d = [gpu.from_numpy(f.copy()).to("cuda:0") for f in x]
    gpu.cuda.synchronize()
    streams = [Stream(), Stream()]
    batch = Batch([(pl, t.data_ptr(), None, streams[i].handle) for i, t in enumerate(d) for pl in (fwd, inv)])
    n0 = many_fused_pairs()
    batch.run_repeat(3, 2)
    for s in streams:
        s.synchronize()
    assert many_fused_pairs() - n0 == 3 * 2
    for t, wnt, f in zip(d, want, x):
        got = t.cpu().numpy()
        assert np.array_equal(got, wnt)
        err = np.abs(got - f).max()
        print(f"{h}x{w}x{c}: |3 roundtrips - input| max {err:.3e}")
        assert err <= 3 * ROUNDTRIP_TOL


@pytest.mark.parametrize("h,w,c,spec", SHAPES[:1] + SHAPES[2:])
def test_timed_window_runs_its_items_pass_by_pass(gpu, h, w, c, spec):
    from dspfun_amd.engine import Batch, Stream, Events, many_fused_pairs
    fwd, inv, x = setup(gpu, h, w, c, spec)
    npass = fwd.num_passes + inv.num_passes
    want = [by_passes(gpu, fwd, inv, f, 4) for f in x]
    d = [gpu.from_numpy(f.copy()).to("cuda:0") for f in x]
    gpu.cuda.synchronize()
    streams = [Stream(), Stream()]
    batch = Batch([(pl, t.data_ptr(), None, streams[i].handle) for i, t in enumerate(d) for pl in (fwd, inv)])
    # 4 repeats of 2 pairs; repeats 0 and 2 bracket a window of two items: frame 0's pair, then frame 1's
    ev = Events(2 * npass * 2)
    n0 = many_fused_pairs()
    batch.run_repeat(4, 0, 2, 2, ev)
    for s in streams:
        s.synchronize()
    assert many_fused_pairs() - n0 == 4 * 2 - 2
    for j in range(npass * 2):                     # every pass of the timed items has its own pair of recorded events around one kernel
        assert ev.elapsed_ms(2 * j, 2 * j + 1) > 0.0, j
    for t, wnt in zip(d, want):
        assert np.array_equal(t.cpu().numpy(), wnt)
