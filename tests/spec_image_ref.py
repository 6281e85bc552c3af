"""TEST-ONLY: spec and ispec on 8-bit images restated in float64 (spec/spec.c:63-139, spec/ispec.c:84-167), the five-step compositions a caller
had to write before dspfft_execute_spec_u8 / dspfft_execute_ispec_u8 existed, and the shapes, parameter sets and bounds the CPU and GPU tests
of those calls share."""
import ctypes as C
import itertools

import numpy as np

import oracle_lib as ol

RANGES, SCALES, SIGNS = ("one", "dc", "dcs"), ("log", "linear"), ("abs", "shift", "saturate", "retain")
ALL_CODES = list(itertools.product(range(3), range(2), range(4)))          # (range, scale, sign) codes, as dspfft_spec_encode

# (h, w, c): what each exercises is in tests/test_spec_image_gpu.py
SHAPES = [(256, 256, 3), (480, 512, 3), (256, 256, 1), (16, 1024, 1), (24, 40, 3), (29, 37, 3), (16, 16, 4)]
# the parameter sets run on every shape: (range, scale, sign, sign map, restore_dc)
LISTED = [(1, 0, 0, True, 1), (1, 0, 0, False, 0), (0, 1, 1, False, 0), (2, 0, 2, False, 1)]


def shape_id(s):
    return "x".join(str(v) for v in s)


def image(shape):
    h, w, c = shape
    return ol.synth_u8(0x5BEC0000 + h * 4099 + w * 17 + c, h * w * c).reshape(h, w, c)


def native_gain(h, w):
    return 127.5 * np.sqrt(4.0 * w * h)


# ---- float64 ----
def coeffs64(img):
    """normalise(D2(p / 255)): the uniform-range coefficients spec.c:63-78 hands its encoding"""
    h, w, c = img.shape
    f = np.ascontiguousarray(ol.dct2d_interleaved(img.astype(np.float64) / 255.0, ol.REDFT10, impl="port", threads=8))
    ol.lib().oracle_spec_normalise_f64(f.ctypes.data, w, h, c)
    return f


def divisors64(f, gain, rng):
    """spec.c:92-110: max[] before the log (per channel)"""
    d = f.shape[-1]
    first = f.reshape(-1, d)[0] * gain
    if rng == 0:
        return np.full(d, float(gain))
    if rng == 1:
        return np.full(d, first.max())
    return first.copy()


def encode64(f, gain, rng, scale, sign):
    """spec.c:88-136 in double: the float the spectrogram image holds, and the encoding's largest slope d e / d f"""
    d = f.shape[-1]
    mx = divisors64(f, gain, rng)
    v = f * gain
    if scale == 0:
        m = np.log1p(mx)
        v = np.copysign(np.log1p(np.abs(v)), v) / m
    else:
        m = mx
        v = v / m
    slope = gain / np.abs(m).min()
    if sign == 0:
        v = np.abs(v)
    elif sign == 1:
        v = (v / 2.0 + 0.5) * 254 / 255
        slope *= 127.0 / 255
    elif sign == 2:
        flat = v.reshape(-1)
        flat[d:] = (~np.signbit(flat[d:])).astype(np.float64)
    return v, slope


def bytes_of(e):
    """the 8-bit writer: clamp(lround(255 e)) (half away from zero, as lround)"""
    p = 255.0 * np.asarray(e, dtype=np.float64)
    return np.clip(np.floor(np.clip(p, -1.0, 256.0) + 0.5), 0, 255).astype(np.uint8)


def decode64_values(v, signmap, gain, rng, scale, sign, dc, restore_dc):
    """ispec.c:84-163 in double on the values the reader hands over, (h, w, d): the coefficients REDFT01 takes"""
    h, w, d = v.shape
    v = np.array(v, dtype=np.float64).reshape(-1)
    if signmap is not None:
        s = signmap.reshape(-1).astype(np.int64) - 128
        v[d:] = np.copysign(v[d:], s[d:].astype(np.float64))
    if sign == 1:
        v = (v * 255.0 / 254 - 0.5) * 2
    elif sign == 2:
        v[d:] = v[d:] * 2 - 1
    if rng == 0:
        mx = np.full(d, float(gain))
    elif rng == 1:
        mx = np.full(d, (np.asarray(dc) * gain).max())
    else:
        mx = np.asarray(dc, dtype=np.float64) * gain
    z = np.arange(v.size) % d
    if scale == 0:
        v = np.copysign(np.expm1(np.abs(v * np.log1p(mx)[z])), v)
    else:
        v = v * mx[z]
    v = v / gain
    f = np.ascontiguousarray(v.reshape(h, w, d))
    ol.lib().oracle_ispec_denormalise_f64(f.ctypes.data, w, h, d)
    if restore_dc:
        f.reshape(-1)[:d] = dc
    return f


def decode64(b, signmap, gain, rng, scale, sign, dc, restore_dc, reader=np.float32):
    """the same on the bytes of a spectrogram.  reader: the type of the value the image reader hands ispec.c:81 -- `coeff`, a float in the
    build the device calls follow (dspfft_execute_ispec_u8 is specified on v = (float)(b / 255.0)); everything after it is double here.
    The rounding of b / 255 to float is part of the input, not of the arithmetic under test: under `shift` a byte of 127 decodes to
    2 (v 255 / 254 - 0.5), which is 0 for the double v and -5.9e-8 for the float v, the same on every sample that holds 127, and REDFT01 adds
    those up coherently next to pixel (0, 0) -- levels of difference there between the two readers, which the composition has as well."""
    v = (b.astype(np.float64) / 255.0).astype(reader).astype(np.float64)
    return decode64_values(v, signmap, gain, rng, scale, sign, dc, restore_dc)


def ispec64(b, signmap, gain, rng, scale, sign, dc, restore_dc, reader=np.float32):
    """the pixels (0..1) ispec reconstructs from the bytes, in double"""
    f = decode64(b, signmap, gain, rng, scale, sign, dc, restore_dc, reader)
    return ol.dct2d_interleaved(f, ol.REDFT01, impl="port", threads=8)


def forward_bound(f_ref, slope):
    """|byte - clamp(255 e_ref)| allowed: half a level of rounding + the float transform's standing tolerance (1e-5 max|f|) through the encoding"""
    return 0.5 + 255.0 * slope * 1e-5 * np.abs(f_ref).max()


def saturate_undecided(f_ref):
    """samples whose sign the float transform cannot be held to (first pixel apart): |f| within its tolerance of zero"""
    d = f_ref.shape[-1]
    u = (np.abs(f_ref) <= 1e-5 * np.abs(f_ref).max()).reshape(-1)
    u[:d] = False
    return u.reshape(f_ref.shape)


def inverse_bound(p_ref):
    return 0.5 + 255.0 * 1e-5 * np.abs(p_ref).max()


# ---- the compositions on the device: calls that exist without the fused ones ----
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def composition_forward(torch, L, fwd, d_img, codes, gain):
    """dspfft_u8_to_f32 -> plan -> dspfft_spec_encode -> dspfft_f32_to_u8(255), once with the caller's parameters and once with the `sign`
    preset: (bytes, sign map, DC) as host arrays"""
    h, w, c = d_img.shape
    n = h * w * c
    outs = []
    dc = None
    for (rng, scale, sign), g in ((tuple(codes), gain), ((0, 1, 2), 1.0)):
        f = torch.empty(n, dtype=torch.float32, device="cuda")
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert L.dspfft_u8_to_f32(_ptr(f), _ptr(d_img), n, None) == 0
        fwd.execute(f.data_ptr())
        if dc is None:
            dc = f[:c].cpu().numpy().astype(np.float64)
        assert L.dspfft_spec_encode(_ptr(f), h * w, c, g, rng, scale, sign, None) == 0
        assert L.dspfft_f32_to_u8(_ptr(out), _ptr(f), 255.0, n, None) == 0
        outs.append(out.cpu().numpy().reshape(h, w, c))
    return outs[0], outs[1], dc


def composition_inverse(torch, L, inv, b, signmap, codes, gain, dc, restore_dc):
    """host (b / 255) as float -> upload -> dspfft_ispec_signmap -> dspfft_ispec_decode -> plan -> dspfft_f32_to_u8(255)"""
    h, w, c = b.shape
    n = h * w * c
    rng, scale, sign = codes
    f = torch.from_numpy((b.astype(np.float64) / 255.0).astype(np.float32).reshape(-1)).to("cuda")
    if signmap is not None:
        m = torch.from_numpy(np.ascontiguousarray(signmap).reshape(-1)).to("cuda")
        assert L.dspfft_ispec_signmap(_ptr(f), _ptr(m), h * w, c, None) == 0
    dcp = None if dc is None else (C.c_double * c)(*[float(v) for v in dc])
    assert L.dspfft_ispec_decode(_ptr(f), h * w, c, gain, rng, scale, sign, dcp, int(restore_dc), None) == 0
    inv.execute(f.data_ptr())
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert L.dspfft_f32_to_u8(_ptr(out), _ptr(f), 255.0, n, None) == 0
    return out.cpu().numpy().reshape(h, w, c)
