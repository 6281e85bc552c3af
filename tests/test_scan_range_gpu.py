"""GPU (-m gpu): the range-masked fused scan step (dspfft_execute_masked_accumulate_range) on the natural 4K and 8K frames (split passes,
prepared tables with element ids), f32 and f64, against the oracle; host/scan_dev's --offset / --skip / --invert / --frames against a
restatement of scan/scan.c:346-459; dist.FrameShardedScan on one GPU against ChannelShardedScan's frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import scan_device_checks as sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
ZIGZAG = 2


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


_ORACLE = {}


def _oracle(co, sel, key):
    """unnormalised REDFT01^2 of the coefficients where sel, in f64 (cached: f32 and f64 plans share the coefficients)"""
    if key not in _ORACLE:
        m = np.where(sel[:, :, None], co.astype(np.float64), 0.0)
        _ORACLE[key] = ol.dct2d_interleaved(m, ol.REDFT01, impl="port", threads=8)
    return _ORACLE[key]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("h,w", [(2160, 3840), (4320, 7680)])
def test_range_on_large_frames(gpu, h, w, dtype):
    torch = gpu
    from dspfun_amd import Plan, REDFT10, REDFT01, _lib
    L = _lib.load()
    c, n = 3, w * h
    tdt = torch.float32 if dtype == "f32" else torch.float64
    x = ol.synth_f32(0x8A4E + h, n * c).reshape(h, w, c)
    d = torch.from_numpy(x).to("cuda:0")
    Plan.image(h, w, c, REDFT10).set_scale(1.0 / (4.0 * w * h)).execute(d.data_ptr())
    torch.cuda.synchronize()
    co = d.cpu().numpy()                                     # f32 coefficients; the f64 plan gets the same values widened
    dco = torch.from_numpy(co).to("cuda:0", dtype=tdt)
    del d
    inv = Plan.image(h, w, c, REDFT01, dtype=dtype)
    if dtype == "f32" and w == 7680:
        assert "COL*/2" in inv.describe()
    index = torch.empty(n, dtype=torch.int32, device="cuda:0")
    assert L.dspfft_scan_owner_index(index.data_ptr(), ZIGZAG, w, h, None) == 0
    index[0] = -1
    ids = torch.empty(n, dtype=torch.int32, device="cuda:0")
    assert L.dspfft_scan_frame_ids(ids.data_ptr(), ZIGZAG, w, h, (n + 31) // 32, None) == 0
    inv.scan_prepare(ids.data_ptr(), c)                      # tile ranges + 1-byte element ids (32 frames)
    acc, work = torch.empty_like(dco), torch.empty_like(dco)
    hidx = index.cpu().numpy().view(np.uint32).reshape(h, w)
    hids = ids.cpu().numpy().view(np.uint32).reshape(h, w)
    tol = 5e-6 if dtype == "f32" else 1e-10
    cases = [("index", index, hidx, n // 5, n // 2), ("ids", ids, hids, 3, 9), ("ids", ids, hids, 0, NONE)]
    for name, t, ht, lo, hi in cases:
        acc.zero_()
        inv.execute_masked_accumulate_range(dco.data_ptr(), work.data_ptr(), acc.data_ptr(), t.data_ptr(), lo, hi, c)
        torch.cuda.synchronize()
        sel = (ht.astype(np.int64) >= lo) & (ht.astype(np.int64) < hi) & (ht != NONE)
        ref = _oracle(co, sel, (h, name, lo, hi))
        err = float(np.abs(acc.cpu().numpy() - ref).max())
        assert err < tol, (h, w, dtype, name, lo, hi, err)
    # one id == the range of one, byte for byte (prepared table path)
    a, b = torch.zeros_like(dco), torch.zeros_like(dco)
    inv.execute_masked_accumulate(dco.data_ptr(), work.data_ptr(), a.data_ptr(), ids.data_ptr(), 5, c)
    inv.execute_masked_accumulate_range(dco.data_ptr(), work.data_ptr(), b.data_ptr(), ids.data_ptr(), 5, 6, c)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32 if dtype == "f32" else torch.int64), b.view(torch.int32 if dtype == "f32" else torch.int64))


# ---- host/scan_dev with the frame-loop options ----
class _OrderList(C.Structure):
    _fields_ = [("limit", C.c_size_t), ("max_interval", C.c_size_t), ("total", C.c_size_t), ("offset", C.POINTER(C.c_size_t)),
                ("yx", C.POINTER(C.c_size_t))]


def _orders(method, w, h):
    so = sd.host_lib()
    if method.startswith("random:"):
        so.scan_order_random.argtypes = [C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(_OrderList)]
        so.scan_order_list_free.argtypes = [C.POINTER(_OrderList)]
        fl = _OrderList()
        assert so.scan_order_random(w, h, int(method.split(":")[1]), C.byref(fl)) == 0
        out = [[(fl.yx[2 * k], fl.yx[2 * k + 1]) for k in range(fl.offset[i], fl.offset[i + 1])] for i in range(fl.limit)]
        so.scan_order_list_free(C.byref(fl))
        return out
    return sd.host_orders(so, sd.METHODS.index(method), w, h)


def _restated_sum(x, orders, step, offset, fill, invert, nframes):
    """scan.c:346-459 in f64: the final sum"""
    h, w, c = x.shape
    co = ol.dct2d_interleaved(x, ol.REDFT10, impl="direct") / (4.0 * w * h)
    limit = len(orders)
    if not nframes or nframes > limit // step:
        nframes = (limit + step - 1) // step
    if offset >= limit:
        offset = limit - 1
    m = np.zeros((h, w), dtype=np.int64)                     # how many times each coefficient is added

    def add(indices):
        f = np.zeros((h, w), dtype=bool)
        for j in indices:
            for (y, xx) in orders[j]:
                if y < h and xx < w:
                    f[y, xx] = True
        f[0, 0] = False
        m[...] += f
    if fill:
        add([limit - i - 1 if invert else i for i in range(offset)])
    for i in range(offset, offset + nframes):
        add([limit - q - 1 if invert else q for q in range(i * step, min(i * step + step, limit))])
    return co[0, 0] + ol.dct2d_interleaved(co * m[:, :, None], ol.REDFT01, impl="direct")


def _write_ppm(path, img):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(img.astype(np.uint8).tobytes())


def _read_pf(path, h, w):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        assert [int(v) for v in f.readline().split()] == [w, h]
        f.readline()
        return np.frombuffer(f.read(), dtype=np.float32).reshape(h, w, 3)


@pytest.mark.parametrize("method", ["zigzag", "radial", "box", "random:5"])
def test_scan_dev_options(gpu, tmp_path, method):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    w, h = 40, 24
    img = ol.synth_u8(0x5D + len(method), w * h * 3).reshape(h, w, 3)
    ppm, out = tmp_path / "in.ppm", tmp_path / "sum.pf"
    _write_ppm(ppm, img)
    x = img.astype(np.float64) / 255.0
    orders = _orders(method, w, h)
    limit = len(orders)
    for step, offset, fill, invert, nframes in ((7, 0, True, True, 0), (5, limit // 3, True, False, 0), (3, 40, False, True, 9),
                                                (4, 25, True, True, limit // 4), (6, limit + 3, True, False, 0)):
        args = [os.path.join(ROOT, "host", "scan_dev"), "--offset", str(offset), str(ppm), str(out), str(step), method]
        args += (["--skip"] if not fill else []) + (["--invert"] if invert else []) + ["--frames", str(nframes)]
        r = subprocess.run(args, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"device-resident" in r.stderr, r.stderr
        want = _restated_sum(x, orders, step, offset, fill, invert, nframes)
        err = np.abs(_read_pf(out, h, w) - want).max()
        assert err <= 5e-6, (method, step, offset, fill, invert, nframes, err)


def test_frame_sharded_one_gpu_matches_channel_sharded_8k(gpu):
    torch = gpu
    from dspfun_amd.dist import ChannelShardedScan, FrameShardedScan
    h, w, c = 4320, 7680, 3
    x = torch.from_numpy(ol.synth_f32(0xF5C8, h * w * c).reshape(h, w, c)).to("cuda:0")
    step = (w * h + 31) // 32
    ch = ChannelShardedScan(x, step)
    fr = FrameShardedScan(x, step)
    assert (fr.f0, fr.f1) == (0, 32)
    for k in range(32):
        assert ch.next_frame()
        assert fr.next_frame() == k
        err = float((ch.sums[0] - fr.sum).abs().max())
        assert err <= 1e-6, (k, err)
    assert fr.next_frame() is None
    assert float((fr.sum - x).abs().max()) <= 5e-6
