"""Transfer characteristics on one MI355X: what an evaluation of iec61966-2-1 per sample costs the kernels that carry it, against the same
kernels with trc 0 (the kernels as they were).  Events around each call, warm-up, the median of --reps; one JSON line per leg.

  apply      dspfft_trc_apply_f32 on 3 x 7680 x 4320 floats (encode, decode), and every candidate evaluation behind the same streaming
             kernel (tools/trc_candidates.hip, built here into tools/libtrc_candidates.so): copy, plain (the device library's double pow),
             lean (trc_core.h's production evaluation), powf (single precision, misses the 1-ulp bar)
  compose    scan's compose at 7680 x 4320 without -i and with it, trc 0 and iec61966-2-1
  zoom       a 7680 x 4320 animation frame, planar (GBR) and interleaved, trc 0 and iec61966-2-1: the difference is the finish pass

  python tools/bench_trc.py [--reps N] [--baseline-only]

--baseline-only runs the trc 0 legs alone and touches none of the new entry points: with DSPFFT_LIB_PATH naming a build of the parent
commit it shows whether the trc 0 kernels have moved."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 7680, 4320
TRC = "iec61966-2-1"
CANDIDATES = ["copy", "plain", "lean", "powf"]


def candidates_lib():
    src, so = os.path.join(ROOT, "tools", "trc_candidates.hip"), os.path.join(ROOT, "tools", "libtrc_candidates.so")
    hdr = os.path.join(ROOT, "dspfun_amd", "csrc", "trc_core.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3", "-ffp-contract=on", "-fPIC", "-shared",
                               "--offload-arch=gfx950", src, "-o", so])
    lib = C.CDLL(so)
    lib.trc_candidate_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("no GPU visible", file=sys.stderr)
        return 2
    from dspfun_amd import ScanFrames, _lib
    from dspfun_amd.zoom import Zoom
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, npix = W * H * 3, W * H

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    def say(**kw):
        print(json.dumps(kw), flush=True)

    g = torch.Generator(device="cuda")
    g.manual_seed(0xD5F0007)
    img = torch.rand(n, device="cuda", generator=g) * 1.25 - 0.125          # a little below 0 and above 1, as reconstructions are
    out = torch.empty_like(img)
    trc = 0 if args.baseline_only else L.dspfft_trc_from_name(TRC.encode())

    # ---- apply, and the candidates behind the same kernel ----
    if not args.baseline_only:
        cl = candidates_lib()
        base = {}
        for inverse in (0, 1):
            for ci, name in enumerate(CANDIDATES):
                ms = timed(lambda: cl.trc_candidate_apply(ci, out.data_ptr(), img.data_ptr(), n, trc, inverse, st))
                base.setdefault(inverse, ms if name == "copy" else None)
                say(leg="candidate", evaluation=name, direction="decode" if inverse else "encode", floats=n, ms=round(ms, 4),
                    ratio_to_copy=round(ms / base[inverse], 3), GB_per_s=round(2 * 4 * n / ms / 1e6, 1))
            ms = timed(lambda: L.dspfft_trc_apply_f32(out.data_ptr(), img.data_ptr(), n, trc, inverse, st))
            say(leg="apply", direction="decode" if inverse else "encode", floats=n, ms=round(ms, 4), ratio_to_copy=round(ms / base[inverse], 3),
                GB_per_s=round(2 * 4 * n / ms / 1e6, 1))

    # ---- scan's compose ----
    for inter in (False, True):
        res = {}
        for t in ((0,) if args.baseline_only else (0, trc)):
            sf = ScanFrames(W, H, intermediates=inter, **({"trc": t} if t else {}))
            frame = torch.empty(sf.frame_floats, device="cuda")
            s = img.clone()
            image = torch.full((n,), -0.0, device="cuda") if inter else None
            sf.begin(frame, img, stream=st)
            res[t] = timed(lambda: sf.compose(frame, s, image, img, None, 0, stream=st))
            del sf, frame, s, image
            torch.cuda.empty_cache()
        say(leg="compose", intermediates=inter, size=f"{W}x{H}", samples_encoded=n * (2 if inter else 1), trc0_ms=round(res[0], 4),
            **({} if args.baseline_only else {"trc_ms": round(res[trc], 4), "ratio": round(res[trc] / res[0], 3)}))

    # ---- zoom's finish ----
    zi = torch.rand((1080, 1920, 3), device="cuda", generator=g)
    z = Zoom(torch, zi)
    anim = z.animation(W, H, 0)
    for layout in ("gbr", "rgb"):
        fr = torch.empty((3, H, W) if layout == "gbr" else (H, W, 3), device="cuda")
        res = {}
        for t in ((0,) if args.baseline_only else (0, trc)):
            if t:
                anim.set_trc(t)
            res[t] = timed(lambda: anim.frame((4.0, 1.0), (4.0, 1.0), 0.0, 0.0, 0, layout, out=fr))
        if not args.baseline_only:
            anim.set_trc(0)
        say(leg="zoom frame", layout=layout, size=f"{W}x{H}", samples_encoded=n, trc0_ms=round(res[0], 4),
            **({} if args.baseline_only else {"trc_ms": round(res[trc], 4), "finish_added_ms": round(res[trc] - res[0], 4), "ratio": round(res[trc] / res[0], 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
