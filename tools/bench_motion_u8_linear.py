"""motion --linear on 8-bit video on one MI355X: the 1920 x 1080 x 256 luma clip u8 -> u8 (motion's quantiser between the transforms)
  plain      trc 0: dspfft_execute_roundtrip_u8 as it was
  fused      iec61966-2-1 through dspfft_plan_set_u8_trc: the same launches, tables at the 8-bit ends
  composed   what the library offered before: dspfft_u8_to_f32 -> dspfft_trc_apply_f32 (decode) -> float roundtrip -> dspfft_trc_apply_f32
             (encode) -> dspfft_f32_to_u8, five sweeps and launches over the float clip
  flat       the new flat pair around the float roundtrip (the unfused fallback of the fused call)
Events around each call, warm-up, the median and the spread of --reps; one JSON line per leg.

  python tools/bench_motion_u8_linear.py [--reps N] [--baseline-only | --plain-only] [--frames F]

--baseline-only runs `plain` alone and touches none of the new entry points: with DSPFFT_LIB_PATH naming a build of the parent commit
(tools/ab_oldlib.sh) it is the parent's time on the same box, and --plain-only is this tree's leg to alternate it with; under rocprofv3 --kernel-trace --stats it lists the kernels of either build."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 1080, 1920
TRC = "iec61966-2-1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--plain-only", action="store_true", help="this tree's trc 0 leg alone (the partner of --baseline-only in an A/B)")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("no GPU visible", file=sys.stderr)
        return 2
    from dspfun_amd import Plan, _lib, engine
    L = _lib.load()
    frames, r2 = args.frames, math.sqrt(2.0)
    st = torch.cuda.current_stream().cuda_stream

    def plans():
        fwd = Plan.many_r2r([H, W], [5, 5], howmany=frames, idist=H * W, odist=H * W).set_scale(2 * r2)
        inv = Plan.many_r2r([H, W], [4, 4], howmany=frames, idist=H * W, odist=H * W, first_axis_first=True).set_scale(1.0 / (2 * r2) / (4.0 * H * W))
        for a in range(2):
            fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
            inv.set_axis_scale0(a, r2, 1.0)
        return fwd, inv

    g = torch.Generator(device="cuda")
    g.manual_seed(0xD5F0008)
    src = torch.randint(0, 256, (frames, H, W), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.zeros_like(src)
    work = torch.empty((frames, H, W), device="cuda")
    flt = dict(active=(1, H, W), minbuf_hw=(H, W), block_depth=1, band_begin=(0, 0, 0), band_end=(1, H, W), quantizer=20.0 * 8 * math.sqrt(W * H))

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
        return dict(ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    def say(**kw):
        print(json.dumps(kw), flush=True)

    lib = "the build named by DSPFFT_LIB_PATH" if os.environ.get("DSPFFT_LIB_PATH") else "this tree"
    fwd, inv = plans()
    run = lambda: fwd.roundtrip_u8(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), 1.0, filter=flt, stream=st)
    say(leg="plain", library=lib, frames=frames, **timed(run))
    if args.baseline_only or args.plain_only:
        return 0
    plain = dst.clone()
    trc = engine.trc_id(TRC)
    n = src.numel()

    def composed():
        L.dspfft_u8_to_f32(work.data_ptr(), src.data_ptr(), n, st)
        L.dspfft_trc_apply_f32(work.data_ptr(), work.data_ptr(), n, trc, 1, st)           # (the decode of x / 255, in units of 255: see below)
        fwd.roundtrip(inv, work.data_ptr(), filter=flt, stream=st)
        L.dspfft_trc_apply_f32(work.data_ptr(), work.data_ptr(), n, trc, 0, st)
        L.dspfft_f32_to_u8(dst.data_ptr(), work.data_ptr(), 1.0, n, st)
    # (the float function works on [0, 1] and the bytes are 0..255: the two extra scalings a caller would fold into these sweeps are left
    # out, so the composed leg is timed at its cheapest; its bytes are not the fused leg's and are not compared)
    say(leg="composed", sweeps=5, frames=frames, **timed(composed))

    def flat():
        engine.u8_to_f32_trc(src, trc, out=work, stream=st)
        fwd.roundtrip(inv, work.data_ptr(), filter=flt, stream=st)
        engine.f32_to_u8_trc(work, trc, 1.0, out=dst, stream=st)
    t = timed(flat)
    want = dst.clone()
    say(leg="flat", sweeps=3, frames=frames, **t)
    fwd.set_u8_trc(trc)
    inv.set_u8_trc(trc)
    t = timed(run)
    say(leg="fused", frames=frames, equals_flat=bool(torch.equal(dst, want)),
        differs_from_plain=float((dst != plain).float().mean()), **t)
    fwd.set_u8_trc(0)
    inv.set_u8_trc(0)
    t = timed(run)
    say(leg="plain again", frames=frames, equals_plain=bool(torch.equal(dst, plain)), **t)
    return 0


if __name__ == "__main__":
    sys.exit(main())
