"""spec / ispec on 8-bit images as one fused call each way (dspfft_execute_spec_u8 / dspfft_execute_ispec_u8), one GPU:

    python tools/bench_spec_u8.py [--out FILE] [--iters N]

For 3840 x 2160 x 3 and 256 x 256 x 3 (h x w x c rows: 2160 x 3840, 256 x 256), in one process, warm:
  spec fused          spec_u8 with sign map and DC (template abs: log, abs, range dc, native gain)
  spec composition    dspfft_u8_to_f32 -> dspfft_execute -> dspfft_spec_encode -> dspfft_f32_to_u8(255), then the same chain once more with
                      the `sign` preset for the sign map: only calls that exist without the fused ones
  spec fused, no map / spec composition, no map     the same without the sign map (one chain)
  ispec fused         ispec_u8 with the sign map and restore_dc
  ispec composition   upload-equivalent (b / 255 as floats, made on the device by dspfft_u8_to_f32 and one torch multiply -- a host upload would
                      only add to it) -> dspfft_ispec_signmap -> dspfft_ispec_decode -> dspfft_execute -> dspfft_f32_to_u8(255)
Device events around every call; the cases alternate inside every iteration; medians over the iterations with the spread (min .. max) and the
ratio composition / fused.  Before timing, the fused bytes are compared with the composition's (forward: bytes, sign map; inverse: against
tests/spec_image_ref.composition_inverse, which uploads b / 255 from the host): they must be equal."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_shape(torch, shape, iters, lines):
    import numpy as np
    import spec_image_ref as sr
    from dspfun_amd import _lib
    from dspfun_amd.engine import spec_image_plans, spec_image_params
    L = _lib.load()
    h, w, c = shape
    n = h * w * c
    stream = torch.cuda.current_stream().cuda_stream
    fwd, inv = spec_image_plans(h, w, c)
    p = spec_image_params(h, w, "abs")
    codes, gain = (p.rangetype, p.scaletype, p.signtype), p.gain
    img = torch.from_numpy(sr.image(shape).reshape(-1)).to("cuda")
    spec, smap, back, tmp8 = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(4))
    work = torch.empty(n, dtype=torch.float32, device="cuda")
    d_dc = torch.zeros(c, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def spec_fused(with_map=True):
        fwd.spec_u8(img.data_ptr(), spec.data_ptr(), work.data_ptr(), p, d_signmap=smap.data_ptr() if with_map else 0, d_dc=d_dc.data_ptr(), stream=stream)

    def spec_chain(out, rng, scale, sign, g):
        assert L.dspfft_u8_to_f32(P(work), P(img), n, stream) == 0
        fwd.execute(work.data_ptr(), stream=stream)
        assert L.dspfft_spec_encode(P(work), h * w, c, g, rng, scale, sign, stream) == 0
        assert L.dspfft_f32_to_u8(P(out), P(work), 255.0, n, stream) == 0

    def spec_comp(with_map=True):
        spec_chain(spec, *codes, gain)
        if with_map:
            spec_chain(smap, 0, 1, 2, 1.0)

    # equality first (and the DC values for the inverse side)
    spec_fused()
    torch.cuda.synchronize()
    got, got_map, dc = spec.cpu().numpy().copy(), smap.cpu().numpy().copy(), d_dc.cpu().numpy().copy()
    spec_comp()
    torch.cuda.synchronize()
    same_f = bool(np.array_equal(got, spec.cpu().numpy()) and np.array_equal(got_map, smap.cpu().numpy()))
    hdc = [float(v) / 255.0 for v in got_map[:c]]                                     # ispec.c:92-93
    dcp = (C.c_double * c)(*hdc)

    def ispec_fused():
        inv.ispec_u8(spec.data_ptr(), back.data_ptr(), work.data_ptr(), p, d_signmap=smap.data_ptr(), dc=hdc, restore_dc=True, stream=stream)

    def ispec_comp():
        assert L.dspfft_u8_to_f32(P(work), P(spec), n, stream) == 0
        work.mul_(1.0 / 255.0)
        assert L.dspfft_ispec_signmap(P(work), P(smap), h * w, c, stream) == 0
        assert L.dspfft_ispec_decode(P(work), h * w, c, gain, *codes, dcp, 1, stream) == 0
        inv.execute(work.data_ptr(), stream=stream)
        assert L.dspfft_f32_to_u8(P(tmp8), P(work), 255.0, n, stream) == 0

    ispec_fused()
    torch.cuda.synchronize()
    want = sr.composition_inverse(torch, L, inv, got.reshape(shape), got_map.reshape(shape), codes, gain, hdc, 1)
    same_i = bool(np.array_equal(back.cpu().numpy().reshape(shape), want))
    lines.append(f"{h}x{w}x{c}: fused bytes == composition bytes: forward {same_f}, inverse {same_i}")

    cases = {"spec fused": spec_fused, "spec composition": spec_comp, "spec fused, no map": lambda: spec_fused(False), "spec composition, no map": lambda: spec_comp(False),
             "ispec fused": ispec_fused, "ispec composition": ispec_comp}
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(iters):
        for name, f in cases.items():
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, v in times.items():
        lines.append(f"{h}x{w}x{c}  {name:26s} median {med[name] * 1e3:9.1f} us   min {min(v) * 1e3:9.1f}   max {max(v) * 1e3:9.1f}   ({iters} iterations)")
    for a, b in (("spec composition", "spec fused"), ("spec composition, no map", "spec fused, no map"), ("ispec composition", "ispec fused")):
        lines.append(f"{h}x{w}x{c}  {a} / {b}: {med[a] / med[b]:.2f}x")
    return same_f and same_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=60)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []
    ok = True
    for shape in ((2160, 3840, 3), (256, 256, 3)):
        ok = bench_shape(torch, shape, a.iters, lines) and ok
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
