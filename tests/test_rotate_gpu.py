"""rotate on the device (dspfun_amd/rotate.py -> dspfft_rotate): the fixture compiled from the reference's own lines, parity with the numpy
restatement on volumes around the tiles for every map and element size, bases that are only element-aligned, a round trip through the
computed inverse, -s as a view, and stream order.  Bytes match or they do not: every comparison is array_equal."""
import numpy as np
import pytest

import rotate_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def test_fixture_cases_byte_for_byte(torch):
    from dspfun_amd import rotate
    fx = rr.fixture()
    vol = dev(torch, fx["vol"])                      # [5][3][7][2]
    outs = [rotate.rotate(torch, vol, str(s)) for s in fx["spellings"]]
    for s, m, o, want in zip(fx["spellings"], fx["map"], outs, fx["out"]):
        assert tuple(o.shape) == (fx["vol"].shape[2 - m[2]], fx["vol"].shape[2 - m[1]], fx["vol"].shape[2 - m[0]], 2), s
        assert np.array_equal(o.cpu().numpy().ravel(), want), s


@pytest.mark.parametrize("E", [1, 2, 3, 4, "f32"])
def test_parity_with_numpy_for_every_map(torch, E):
    from dspfun_amd import rotate
    nb = 4 if E == "f32" else E
    for vi, (w, h, f) in enumerate(rr.volumes(nb)):
        raw = rr.pattern(3000 + 10 * nb + vi, w * h * f * nb).reshape(f, h, w, nb)
        if E == "f32":
            vol = torch.from_numpy(raw.view(np.float32).reshape(f, h, w).copy()).to("cuda:0")      # (any bit pattern: the bytes are only moved)
        elif E == 1 and vi % 2 == 0:
            vol = dev(torch, raw.reshape(f, h, w))                                                    # a planar 8-bit plane
        else:
            vol = dev(torch, raw)
        outs = [(spec, rotate.rotate(torch, vol, spec)) for spec in rr.maps48()]
        for spec, o in outs:
            m, inv = rr.parse(spec)
            want = rr.rotate(raw, m, inv)
            got = o.cpu().numpy()
            assert got.shape[:3] == want.shape[:3], (E, (w, h, f), spec)
            assert np.array_equal(got.view(np.uint8).reshape(want.shape), want), (E, (w, h, f), spec)


@pytest.mark.parametrize("E", [1, 3])
def test_bases_one_element_into_a_larger_allocation(torch, E):
    from dspfun_amd import rotate
    w, h, f = 65, 33, 17
    n = w * h * f * E
    raw = rr.pattern(4000 + E, n).reshape(f, h, w, E)
    src = torch.zeros(n + 2 * E + 64, dtype=torch.uint8, device="cuda:0")
    src[E:E + n] = dev(torch, raw.ravel())
    for spec in ("zyx", "-yxz", "y-xz", "-x-zy", "yzx", "-z-y-x"):
        m, inv = rr.parse(spec)
        want = rr.rotate(raw, m, inv)
        dst = torch.full((n + 2 * E + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        shape_in = (f, h, w) if E == 1 else (f, h, w, E)
        shape_out = want.shape[:3] if E == 1 else want.shape
        out = rotate.rotate(torch, src[E:E + n].view(shape_in), spec, out=dst[E:E + n].view(shape_out))
        assert out.data_ptr() == dst.data_ptr() + E
        got = dst.cpu().numpy()
        assert np.array_equal(got[E:E + n], want.ravel()), (E, spec)
        assert np.all(got[:E] == 0xA5) and np.all(got[E + n:] == 0xA5), (E, spec)


def test_round_trip_through_the_computed_inverse(torch):
    from dspfun_amd import rotate
    w, h, f = 130, 67, 5
    raw = rr.pattern(5000, w * h * f).reshape(f, h, w)
    vol = dev(torch, raw)
    for spec in ("zy-x", "-yzx", "z-xy", "-z-y-x", "x-zy"):
        m, inv = rotate.parse(spec)
        back = rr.inverse_spec(m, inv)
        once = rotate.rotate(torch, vol, spec)
        assert np.array_equal(once.cpu().numpy(), rr.rotate(raw[..., None], m, inv)[..., 0]), spec
        assert np.array_equal(rotate.rotate(torch, once, back).cpu().numpy(), raw), (spec, back)


def test_seek_and_frame_count_are_a_view(torch):
    from dspfun_amd import rotate
    w, h, f = 70, 9, 9
    for E in (1, 3):
        raw = rr.pattern(6000 + E, w * h * f * E).reshape(f, h, w, E)
        vol = dev(torch, raw if E > 1 else raw[..., 0])
        for spec in ("zyx", "-yzx", "x-zy"):
            m, inv = rr.parse(spec)
            got = rotate.rotate(torch, vol[2:5], spec).cpu().numpy()
            assert np.array_equal(got.reshape(-1), rr.rotate(raw[2:5], m, inv).reshape(-1)), (E, spec)


def test_two_rotations_on_a_side_stream_are_ordered(torch):
    from dspfun_amd import rotate
    w, h, f = 258, 67, 9
    raw = rr.pattern(7000, w * h * f).reshape(f, h, w)
    vol = dev(torch, raw)
    m1, i1 = rr.parse("zy-x")
    m2, i2 = rr.parse("-yxz")
    want = rr.rotate(rr.rotate(raw[..., None], m1, i1), m2, i2)[..., 0]
    mid = torch.empty(rotate.geometry("zy-x", (w, h, f))["out_shape"], dtype=torch.uint8, device="cuda:0")
    out = torch.empty(want.shape, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    rotate.rotate(torch, vol, "zy-x", out=mid, stream=side.cuda_stream)
    rotate.rotate(torch, mid, "-yxz", out=out, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
