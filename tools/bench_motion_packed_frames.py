"""motion's default block -b 0x0x1 on a 1920x1080x64 rgb24 clip (dspfft_execute_roundtrip_u8_packed_frames), one GPU:

    python tools/bench_motion_packed_frames.py [--out FILE] [--frames 64] [--accuracy]

ms per call, medians over rounds with the spread, for two filters
  q     -q 20: the quantiser alone (position-free, the same for every component: the planar fused column kernel runs it)
  band  -p 0x0x0-200x200x1 with -D 0.2:0.4:0.6 and -q 20: the fused column kernel's twin with the filter of packed pixels
each as
  1. fused       the call
  2. unfused     the call under DSPFFT_NO_FUSED_ROUNDTRIP=1: forward column pass, dspfft_motion_filter_packed, inverse column pass
  3. composed    what a caller writes without the call: de-interleave with torch (permute + contiguous), three planar Plan.roundtrip_u8 calls
                 on per-frame plans, interleave again
  4. planar      the three planar calls alone, on planes that are already apart
  5. copy        a device copy of the clip: the floor of anything that reads and writes it once
Device events around REPS calls after a warm-up of every variant; the variants alternate inside every round.  (1) and (2) must give the same
bytes, which is checked before any time is printed.

--accuracy: the shares of bytes that differ from the float64 reference (tests/motion_packed_frames_ref.py) on the cases of
tests/test_motion_packed_frames_gpu.py::test_the_call_against_the_float64_reference, for the PLANAR Plan.roundtrip_u8 calls on the component
planes (the test's constants PLANAR_SHARE) and for the packed call."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS, REPS = 7, 10
H, W, C = 1080, 1920, 3
QUANT = 20.0
DAMP = (0.2, 0.4, 0.6)


def timed(torch, runs):
    t = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for key, run in runs.items():
            run()                                            # (a variant's first call of the round: not timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                run()
            e1.record()
            e1.synchronize()
            t[key].append(e0.elapsed_time(e1) / REPS)
    return t


def variants(torch, frames, which):
    from dspfun_amd.engine import motion_packed, motion_packed_frame_plans
    import motion_spec_ref as sr
    block = (1, H, W)
    fwd, inv, k = motion_packed_frame_plans(frames, H, W, C)
    pfwd, pinv = sr.stack_plan(block, frames, sr.ol.REDFT10), sr.stack_plan(block, frames, sr.ol.REDFT01)
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, (frames, H, W, C), dtype=torch.uint8, device="cuda", generator=gen)
    dst, dst2 = torch.zeros_like(src), torch.zeros_like(src)
    planes_in = src.permute(3, 0, 1, 2).contiguous()
    planes_out = torch.zeros_like(planes_in)
    work = torch.empty(src.numel(), dtype=torch.float32, device="cuda")
    quantizer = QUANT * 8 * math.sqrt(float(H * W))          # motion.c:570
    base = dict(active=block, minbuf_hw=(H, W), block_depth=1, quantizer=quantizer)
    if which == "q":
        filt = dict(base, band_begin=(0, 0, 0), band_end=block)
        pk = motion_packed("rgb24", damp=1.0)
        per_plane = [dict(filt, damp=1.0, boost=1.0)] * C
    else:
        filt = dict(base, band_begin=(0, 0, 0), band_end=(1, 200, 200))
        pk = motion_packed("rgb24", damp=DAMP, normalization=k["normalization"], scalefactor=k["scalefactor"])
        per_plane = [dict(filt, damp=pk.damp[i], boost=pk.boost[i]) for i in range(C)]
    stream = torch.cuda.current_stream().cuda_stream
    mul = k["out_mul"]

    def run_fused():
        fwd.roundtrip_u8_packed_frames(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), mul, pk, filter=filt, stream=stream)

    def run_unfused():
        os.environ["DSPFFT_NO_FUSED_ROUNDTRIP"] = "1"
        try:
            fwd.roundtrip_u8_packed_frames(inv, src.data_ptr(), dst2.data_ptr(), work.data_ptr(), mul, pk, filter=filt, stream=stream)
        finally:
            del os.environ["DSPFFT_NO_FUSED_ROUNDTRIP"]

    def planar(pin, pout):
        for i in range(C):
            pfwd.roundtrip_u8(pinv, pin[i].data_ptr(), pout[i].data_ptr(), work.data_ptr(), mul, filter=per_plane[i], stream=stream)

    def run_planar():
        planar(planes_in, planes_out)

    def run_composed():
        pin = src.permute(3, 0, 1, 2).contiguous()
        planar(pin, planes_out)
        dst2.copy_(planes_out.permute(1, 2, 3, 0))

    def run_copy():
        dst2.copy_(src)
    run_fused()
    run_unfused()
    torch.cuda.synchronize()
    differ = int((dst != dst2).sum())
    if differ:
        raise SystemExit(f"bench_motion_packed_frames: {which}: the fused call's bytes differ from the unfused call's in {differ} places")
    run_composed()
    torch.cuda.synchronize()
    differ = int((dst != dst2).sum())
    runs = dict(fused=run_fused, unfused=run_unfused, composed=run_composed, planar=run_planar, copy=run_copy)
    return runs, src.numel(), differ, fwd.describe()


def accuracy(torch, lines):
    import motion_packed_frames_ref as pf
    from dspfun_amd.engine import motion_packed_frame_plans
    fwd, inv, info = motion_packed_frame_plans(pf.REF_FRAMES, pf.REF_H, pf.REF_W, 3)
    lines.append(f"# share of bytes that differ from the float64 reference, {pf.REF_FRAMES} x {pf.REF_H} x {pf.REF_W} rgb24, seeds {pf.ref_seeds()}; max byte difference in brackets")
    lines.append("# filter   planar Plan.roundtrip_u8 calls on the planes   packed call")
    shares = {}
    for kind in pf.REF_KINDS:
        clip, refs = pf.ref_case(kind)
        filt, packed = pf.ref_packed(kind, info)
        got, coded = pf.run_call(torch, fwd, inv, clip, info, packed, filt)
        planar = [pf.planar_roundtrip(torch, clip[..., k], refs[k]["filt"]) for k in range(3)]
        rows = [pf.ref_shares([p[0] for p in planar], refs), pf.ref_shares([got[..., k] for k in range(3)], refs)]
        shares[kind] = rows[0][1] / rows[0][2]
        lines.append(f"{str(kind):7s} " + "   ".join(f"{n:5d} of {size:5d} = {n / size:.6e} [{mx}]" for mx, n, size in rows) +
                     f"   coded: reference {sum(r['coded'] for r in refs)}, planar {sum(p[1] for p in planar)}, packed {coded}")
    lines.append("# PLANAR_SHARE: " + ", ".join(f"{k}: {v:.5e}" for k, v in shares.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_packed_frames: no GPU visible", file=sys.stderr)
        return 2
    lines = []
    if args.accuracy:
        accuracy(torch, lines)
    else:
        lines += [f"# motion -b 0x0x1 on rgb24, {W}x{H}x{args.frames}, {torch.cuda.get_device_name(0)}",
                  f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); GB/s of the clip read once and written once"]
        tags = {"fused": "1. the call, fused", "unfused": "2. the call, DSPFFT_NO_FUSED_ROUNDTRIP=1", "composed": f"3. split + {C} planar calls + interleave",
                "planar": f"4. {C} planar calls alone", "copy": "5. device copy of the clip"}
        for which in ("q", "band"):
            runs, nbytes, differ, desc = variants(torch, args.frames, which)
            name = f"-q {QUANT:g}" if which == "q" else f"-p 0x0x0-200x200x1 -D {':'.join(map(str, DAMP))} -q {QUANT:g}"
            if which == "q":
                lines += [f"# {l}" for l in desc.splitlines() if l.startswith("ax")]
            lines.append(f"# {which} = {name}: {differ} of {nbytes} packed bytes differ from the composed planar calls' (another rounding in the last place of the transform)")
            t = timed(torch, runs)
            med = {k: statistics.median(v) for k, v in t.items()}
            for key, v in t.items():
                lines.append(f"{which:5s} {tags[key]:44s} {med[key]:8.3f} ms ({min(v):.3f} .. {max(v):.3f})  {2 * nbytes / med[key] / 1e6:8.1f} GB/s")
            lines.append(f"{which:5s} unfused / fused = {med['unfused'] / med['fused']:.3f}, composed / fused = {med['composed'] / med['fused']:.2f}, planar / fused = {med['planar'] / med['fused']:.2f}")
            del runs
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
