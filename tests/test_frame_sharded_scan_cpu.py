"""CPU: dist.FrameShardedScan -- scan's frame loop with --offset / --skip / --invert / --frames, its output frames spread over the ranks -- on
the test-only emulation backend.  One rank against a Python restatement of scan/scan.c:346-459 on the scan orders of host/libscanorders.so
(the harness-side library tests/scan_device_checks.py checks the device generators against), every emitted frame's sum; then gloo worlds of
2, 3, 4 and 8 ranks against the one-rank run."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle_lib as ol
import scan_device_checks as sd

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = [m for m in sd.METHODS if m != "box"]


def restated_frames(x, orders, step, offset=0, fill=True, invert=False, nframes=0):
    """scan.c:346-459 in float64: {loop frame i: sum after it} (the fill's sum under key None)"""
    h, w, c = x.shape
    co = ol.dct2d_interleaved(x.astype(np.float64), ol.REDFT10, impl="direct") / (4.0 * w * h)
    limit = len(orders)
    if not nframes or nframes > limit // step:                 # :347-348
        nframes = (limit + step - 1) // step
    s = np.broadcast_to(co[0, 0], co.shape).copy()           # :377-383
    if offset >= limit:                                       # :385-386
        offset = limit - 1

    def add(indices):
        m = np.zeros((h, w), dtype=bool)
        for j in indices:
            for (y, xx) in orders[j]:
                m[y, xx] = True
        m[0, 0] = False                                       # :406,445 clear DC
        return ol.dct2d_interleaved(np.where(m[:, :, None], co, 0.0), ol.REDFT01, impl="direct")

    out = {}
    if fill:                                                  # :389-417
        s += add([limit - i - 1 if invert else i for i in range(offset)])
        out[None] = s.copy()
    for i in range(offset, offset + nframes):                 # :421-459
        s += add([limit - q - 1 if invert else q for q in range(i * step, min(i * step + step, limit))])
        out[i] = s.copy()
    return out


@pytest.fixture(scope="module")
def so():
    return sd.host_lib()


def _image(h, w, c=3, seed=0xF5A1):
    return ol.synth_f32(seed + 7 * h + w, h * w * c).reshape(h, w, c)


def _run_all(eng):
    eng.start()
    frames = {}
    while True:
        i = eng.next_frame()
        if i is None:
            return frames
        frames[i] = eng.sum.numpy().copy()


# (step, offset, fill, invert, nframes) -- offset "mid" / "over" resolve against the method's limit; nframes "below", "at", "over" against limit/step
OPTIONS = [
    (1, 0, True, False, 0), (3, 0, True, False, 0), (1, 0, True, True, 0), (2, 0, True, True, 0),
    (1, "mid", True, False, "below"), (3, "mid", True, False, 0), (3, "mid", False, True, "at"), (2, "mid", True, True, "over"),
    (2, "over", True, False, 0), (1, "over", False, True, 0), (4, 1, True, True, "below"), (3, 2, False, False, "at"),
]


@pytest.mark.parametrize("w,h", [(7, 5), (6, 11)])
@pytest.mark.parametrize("method", METHODS)
def test_one_rank_matches_the_restatement(so, method, w, h):
    from emul_lib import emul
    from dspfun_amd.dist import FrameShardedScan
    m = sd.METHODS.index(method)
    orders = [[(y, xx) for (y, xx) in cs] for cs in sd.host_orders(so, m, w, h)]
    limit = len(orders)
    x = _image(h, w)
    for step, offset, fill, invert, nframes in OPTIONS:
        offset = {"mid": limit // 3, "over": limit + 5}.get(offset, offset)
        nframes = {"below": max(1, limit // step - 2), "at": limit // step, "over": limit // step + 4}.get(nframes, nframes)
        opts = dict(offset=offset, fill=fill, invert=invert, nframes=nframes)
        eng = FrameShardedScan(torch.from_numpy(x.copy()), step, method=method, lib=emul(), **opts)
        want = restated_frames(x, orders, step, **opts)
        got = _run_all(eng)
        assert sorted(got) == sorted(k for k in want if k is not None), (method, step, opts)
        for i, s in got.items():
            err = np.abs(s - want[i]).max()
            assert err < 1e-5, (method, w, h, step, opts, i, err)
        assert eng.owner(min(got)) == 0 and eng.owner(eng.offset + eng.nframes) is None


def test_full_scan_returns_the_image():
    from emul_lib import emul
    from dspfun_amd.dist import FrameShardedScan
    x = _image(24, 40)
    for invert in (False, True):
        eng = FrameShardedScan(torch.from_numpy(x.copy()), 37, method="radial", invert=invert, lib=emul())
        frames = _run_all(eng)
        assert len(frames) == eng.nframes
        assert np.abs(frames[max(frames)] - x).max() < 5e-6


def test_box_is_refused():
    from emul_lib import emul
    from dspfun_amd.dist import FrameShardedScan
    with pytest.raises(ValueError, match="scan_dev"):
        FrameShardedScan(torch.zeros(4, 4, 3), 1, method="box", lib=emul())


# ---- several ranks over gloo ----
CASES = [dict(), dict(invert=True), dict(offset=50, nframes=9), dict(offset=30, fill=False, invert=True)]
H, W, STEP = 24, 40, 23


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from emul_lib import emul
        from dspfun_amd.dist import FrameShardedScan
        x = _image(H, W)
        res = []
        for opts in CASES:
            eng = FrameShardedScan(torch.from_numpy(x.copy()), STEP, method="zigzag", lib=emul(), **opts)
            frames = _run_all(eng)
            assert all(eng.owner(i) == rank for i in frames)
            res.append(frames)
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_gloo_worlds_match_one_rank(world):
    from emul_lib import emul
    from dspfun_amd.dist import FrameShardedScan
    emul()                     # built once here, not in every worker
    x = _image(H, W)
    single = []
    for opts in CASES:
        eng = FrameShardedScan(torch.from_numpy(x.copy()), STEP, method="zigzag", lib=emul(), **opts)
        single.append((eng.nframes, _run_all(eng)))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    tol = 5e-6 * np.abs(x).max()
    for k, (nframes, ref) in enumerate(single):
        seen = {}
        for r in range(world):
            frames = got[r][k]
            if world <= nframes:
                assert frames, (world, k, r)             # idle ranks only when there are more ranks than frames
            seen.update(frames)
        assert sorted(seen) == sorted(ref), (world, k)
        for i, s in seen.items():
            assert np.abs(s - ref[i]).max() < tol, (world, k, i)
    # the first two cases scan everything: the last frame is the image
    for k in (0, 1):
        last = single[k][1]
        assert np.abs(last[max(last)] - x).max() < 5e-6
