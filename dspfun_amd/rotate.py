"""rotate (motion/rotate.c) over device memory: a clip's three axes permuted, with flips, in one dspfft_rotate call."""
import ctypes as C
from fractions import Fraction

from . import _lib
from .engine import DspfftError


def parse(spec):
    """rotate.c:74-89 through the C ABI: "zy-x" -> (map, invert), three ints each.  Output axis o (0 = x) runs over input axis map[o];
    input axis a is read backwards iff invert[map[a]].  ValueError for what the reference sends to usage() and for a non-permutation."""
    lib = _lib.load()
    m, inv = (C.c_int * 3)(), (C.c_int * 3)()
    raw = spec.encode() if isinstance(spec, str) else bytes(spec)
    if b"\0" in raw or lib.dspfft_rotate_parse(raw, m, inv) != 0:
        raise ValueError(f"rotate: {spec!r} is no arrangement of the axes x, y, z")
    return tuple(m), tuple(inv)


def geometry(spec, size, rate=None, same_duration=False):
    """size = (w, h, frames) -> {"out_shape": (frames', h', w'), "rate": Fraction | None}.  rate: the input's frame rate; with
    same_duration (-r same) the output's is len[map[2]] num / (len[2] den) (rotate.c:122-126), otherwise the input's."""
    m, _ = parse(spec)
    ln = tuple(int(v) for v in size)
    out_rate = None
    if rate is not None:
        r = Fraction(rate)
        out_rate = Fraction(ln[m[2]] * r.numerator, ln[2] * r.denominator) if same_duration else r
    return {"out_shape": (ln[m[2]], ln[m[1]], ln[m[0]]), "rate": out_rate}


def rotate(torch, vol, spec, out=None, stream=None):
    """vol: a contiguous device tensor [frames][h][w] (uint8 or float32) or [frames][h][w][c] uint8 with c <= 4.  Returns the rotated tensor
    [len[map[2]]][len[map[1]]][len[map[0]]] (with the same trailing c) in the input's kind; `out` must be such a tensor that shares no
    memory with vol.  Stream-ordered on `stream` (a raw stream handle; default: torch's current one)."""
    lib = _lib.load()
    m, inv = parse(spec)
    if vol.dim() not in (3, 4) or not vol.is_cuda or not vol.is_contiguous():
        raise ValueError("rotate: a contiguous device tensor [frames][h][w] or [frames][h][w][c]")
    if vol.dim() == 4:
        if vol.dtype != torch.uint8 or not 1 <= vol.shape[3] <= 4:
            raise ValueError("rotate: packed components are uint8, at most 4 of them")
        ebytes = int(vol.shape[3])
    elif vol.dtype in (torch.uint8, torch.float32):
        ebytes = vol.element_size()
    else:
        raise ValueError("rotate: uint8 or float32")
    ln = (int(vol.shape[2]), int(vol.shape[1]), int(vol.shape[0]))
    shape = (ln[m[2]], ln[m[1]], ln[m[0]]) + tuple(vol.shape[3:])
    if out is None:
        out = torch.empty(shape, dtype=vol.dtype, device=vol.device)
    elif tuple(out.shape) != shape or out.dtype != vol.dtype or out.device != vol.device or not out.is_contiguous():
        raise ValueError(f"rotate: out must be a contiguous {shape} tensor of the input's kind")
    if stream is None:
        stream = torch.cuda.current_stream(vol.device).cuda_stream
    rc = lib.dspfft_rotate(out.data_ptr(), vol.data_ptr(), (C.c_uint64 * 3)(*ln), ebytes, (C.c_int * 3)(*m), (C.c_int * 3)(*inv), stream)
    if rc != 0:
        raise DspfftError(lib.dspfft_motion_last_error().decode())
    return out
