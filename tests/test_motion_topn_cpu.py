"""motion --coeff-limit per block, the parts that need no device: through the test-only emulation library the calls that ARE the plain ones
(keep = 0, keep >= the block's count) and the refusal of a keep in range (the selection kernels are HIP-only); through the product library
every rejection that comes before a launch, and the work-buffer sizes."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from dspfun_amd.engine import Plan, DspfftError

FAKE = C.c_void_p(4096)          # a non-null address for calls that are refused before anything reads it


def stack_plans(lib, n, nb, monkeypatch=None, no_block=False):
    if monkeypatch is not None:
        if no_block:
            monkeypatch.setenv("DSPFFT_NO_BLOCK", "1")
        else:
            monkeypatch.delenv("DSPFFT_NO_BLOCK", raising=False)
    vol = int(np.prod(n))
    nrm = 1.0 / np.prod([2.0 * v for v in n])
    fwd = Plan.many_r2r(n, [5] * len(n), howmany=nb, idist=vol, odist=vol, lib=lib)
    inv = Plan.many_r2r(n, [4] * len(n), howmany=nb, idist=vol, odist=vol, first_axis_first=True, lib=lib).set_scale(nrm)
    return fwd, inv


@pytest.mark.parametrize("no_block", [False, True])
def test_keep_zero_and_keep_at_the_count_are_the_plain_call_on_the_emulation(no_block, monkeypatch):
    from emul_lib import emul
    L = emul()
    n, nb = [8, 8, 8], 6
    fwd, inv = stack_plans(L, n, nb, monkeypatch, no_block)
    assert ("BLOCK" in fwd.describe()) == (not no_block)
    flt = dict(active=n, minbuf_hw=n[1:], block_depth=n[0], band_begin=(0, 1, 0), band_end=(8, 8, 7), damp=0.5, boost=1.25, preserve_dc=1, quantizer=3.0)
    u8 = ol.synth_u8(5, nb * 512)
    x = u8.astype(np.float32)
    outs = []
    for keep in (None, 0, 512, 513, 10 ** 9):
        kw = {} if keep is None else dict(coeff_limit=keep)
        o8 = np.zeros_like(u8); work = np.zeros(nb * 512, dtype=np.float32); coded = np.zeros(1, dtype=np.uint64)
        fwd.roundtrip_u8(inv, u8.ctypes.data, o8.ctypes.data, work.ctypes.data, 1.0, filter=flt, d_coded=coded.ctypes.data, **kw)
        of = np.zeros_like(x)
        fwd.roundtrip(inv, x.ctypes.data, of.ctypes.data, filter=None, **kw)          # (filter may be NULL)
        outs.append((o8, int(coded[0]), of))
    for o8, coded, of in outs[1:]:
        assert np.array_equal(o8, outs[0][0]) and coded == outs[0][1] and coded > 0 and np.array_equal(of, outs[0][2])


@pytest.mark.parametrize("no_block", [False, True])
def test_keep_in_range_is_refused_without_the_hip_kernels_and_nothing_is_written(no_block, monkeypatch):
    from emul_lib import emul
    L = emul()
    fwd, inv = stack_plans(L, [8, 8, 8], 4, monkeypatch, no_block)
    assert L.dspfft_roundtrip_topn_work_bytes(fwd._h, inv._h) == 0
    x = ol.synth_f32(6, 4 * 512)
    out = np.full_like(x, 7.0)
    rc = L.dspfft_execute_roundtrip_topn(fwd._h, inv._h, x.ctypes.data, out.ctypes.data, None, 64, None, 0, None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
    assert np.all(out == 7.0)
    u8 = ol.synth_u8(7, 4 * 512)
    o8 = np.full_like(u8, 9); work = np.full(4 * 512, 7.0, dtype=np.float32)
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8(inv, u8.ctypes.data, o8.ctypes.data, work.ctypes.data, 1.0, coeff_limit=511)
    assert np.all(o8 == 9) and np.all(work == 7.0)


def test_scaled_not_block_on_the_emulation():
    """one block with scaled != block: the count is the whole embedding (motion.c:657)"""
    from emul_lib import emul
    from test_motion_rescale import plans
    L = emul()
    block, scaled = (4, 12, 16), (4, 18, 24)
    minbuf = tuple(max(b, s) for b, s in zip(block, scaled))
    count = int(np.prod(minbuf))
    pix = ol.synth_u8(41, count).reshape(minbuf)
    fwd, inv = plans(Plan, block, scaled, minbuf, lib=L)
    res = []
    for keep in (None, 0, count, count - 1):
        out = np.zeros(minbuf, dtype=np.uint8); work = np.full(minbuf, 7.0, dtype=np.float32)
        try:
            fwd.roundtrip_u8(inv, pix.ctypes.data, out.ctypes.data, work.ctypes.data, 0.01, **({} if keep is None else dict(coeff_limit=keep)))
            res.append(out)
        except DspfftError as e:
            assert keep == count - 1 and "not built into this library" in str(e)
            assert not out.any() and np.all(work == 7.0)
            res.append(None)
    assert res[3] is None and np.array_equal(res[1], res[0]) and np.array_equal(res[2], res[0]) and res[0].any()


def test_topn_blocks_rejections_come_before_any_launch():
    from dspfun_amd import _lib
    L = _lib.load()
    err = L.dspfft_motion_last_error
    assert L.dspfft_motion_topn_blocks(None, 16, 1, 16, 3, None, 0, None) == -1 and b"bad arguments" in err()
    assert L.dspfft_motion_topn_blocks(FAKE, 0, 1, 16, 3, None, 0, None) == -1 and b"bad arguments" in err()
    assert L.dspfft_motion_topn_blocks(FAKE, 2 ** 32, 1, 2 ** 32, 3, FAKE, 1 << 40, None) == -1 and b"32-bit" in err()
    assert L.dspfft_motion_topn_blocks(FAKE, 64, 3, 63, 3, None, 0, None) == -1 and b"overlap" in err()
    need = L.dspfft_motion_topn_blocks_work_bytes(200_000, 7)
    assert need > 2 * 4 * 7 * 200_000
    assert L.dspfft_motion_topn_blocks(FAKE, 200_000, 7, 200_008, 3, FAKE, need - 1, None) == -1 and b"work buffer too small" in err()
    assert L.dspfft_motion_topn_blocks(FAKE, 200_000, 7, 200_008, 3, None, need, None) == -1 and b"work buffer" in err()
    # runs that are selected in LDS need none, and keep >= count is a no-op that touches nothing
    for count in (16, 64, 512, 4096):
        assert L.dspfft_motion_topn_blocks_work_bytes(count, 1000) == 0
    assert L.dspfft_motion_topn_blocks_work_bytes(2 ** 32, 1) == 0
    assert L.dspfft_motion_topn_blocks(FAKE, 64, 3, 64, 64, None, 0, None) == 0
    # the one-run call keeps its work area
    assert L.dspfft_motion_topn_work_bytes(200_000) == L.dspfft_motion_topn_blocks_work_bytes(200_000, 1) - 256


def test_roundtrip_topn_work_bytes_and_rejections_on_the_product_library(monkeypatch):
    """plans of 4-, 8- and 16-point axes need no device tables, so the product library plans them here"""
    from dspfun_amd import _lib
    L = _lib.load()
    fb, ib = stack_plans(L, [8, 8, 8], 10, monkeypatch, False)
    assert "BLOCK" in fb.describe() and L.dspfft_roundtrip_topn_work_bytes(fb._h, ib._h) == 0
    # a clip of 16 x 16 frames in planes of 16 x 512, every frame its own block: a run is a frame's embedding, 15 * 512 + 16 floats
    monkeypatch.setenv("DSPFFT_NO_BLOCK", "1")
    kw = dict(howmany=6, inembed=[16, 512], onembed=[16, 512], idist=16 * 512, odist=16 * 512, lib=L)
    fwd = Plan.many_r2r([16, 16], [5, 5], **kw)
    inv = Plan.many_r2r([16, 16], [4, 4], first_axis_first=True, **kw)
    assert "BLOCK" not in fwd.describe()
    count = 15 * 512 + 16
    need = L.dspfft_roundtrip_topn_work_bytes(fwd._h, inv._h)
    assert need == L.dspfft_motion_topn_blocks_work_bytes(count, 6) and need > 2 * 4 * 6 * count
    call = L.dspfft_execute_roundtrip_topn
    assert call(fwd._h, inv._h, FAKE, FAKE, None, 5, FAKE, need - 1, None, None) == -1 and b"work buffer too small" in L.dspfft_last_error()
    assert call(fwd._h, inv._h, FAKE, FAKE, None, 5, None, need, None, None) == -1 and b"work buffer too small" in L.dspfft_last_error()
    assert call(fwd._h, inv._h, None, FAKE, None, 5, FAKE, need, None, None) == -1 and b"null plan or buffer" in L.dspfft_last_error()
    assert call(None, inv._h, FAKE, FAKE, None, 5, FAKE, need, None, None) == -1 and b"null plan or buffer" in L.dspfft_last_error()
    assert L.dspfft_execute_roundtrip_u8_topn(fwd._h, inv._h, FAKE, FAKE, None, 1.0, None, 5, FAKE, need, None, None) == -1
    assert L.dspfft_roundtrip_topn_work_bytes(None, inv._h) == 0
    # interleaved batches are no contiguous runs: refused, whatever the work buffer
    kw = dict(howmany=3, istride=3, idist=1, ostride=3, odist=1, lib=L)
    fi = Plan.many_r2r([16, 16], [5, 5], **kw)
    ii = Plan.many_r2r([16, 16], [4, 4], first_axis_first=True, **kw)
    assert L.dspfft_roundtrip_topn_work_bytes(fi._h, ii._h) == 0
    assert call(fi._h, ii._h, FAKE, FAKE, None, 5, FAKE, 1 << 30, None, None) == -2 and b"contiguous run" in L.dspfft_last_error()
