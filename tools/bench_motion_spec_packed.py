"""motion --spectrogram on a 1920x1080x64 rgb24 clip (dspfft_execute_spectrogram_u8_packed), one GPU:

    python tools/bench_motion_spec_packed.py [--out FILE] [--frames 64] [--accuracy]

ms per call, medians over rounds with the spread, for the two plan families and the types shift and abs:
  A. -b 8x8x8       small blocks: block_spec_packed.hip's one kernel, 2 C bytes per pixel
  B. -b 0x0x1       full frames: the interleaved plan's passes and motion_spec_packed.hip's kernel
each as
  1. packed      the packed call
  2. composed    what a caller writes without it: de-interleave with torch (permute + contiguous), C planar Plan.spectrogram calls, interleave
                 again (permute + contiguous)
  3. planar      the C planar calls alone, on planes that are already apart
  4. copy        a device copy of the clip: the floor of anything that reads and writes it once
(A)'s packed bytes are checked against (2) before any time is printed ((B)'s interleaved kernels round differently from the planar ones in the
last place: tests/test_motion_spec_packed_gpu.py holds both against the float64 reference).  Device events around REPS calls after a
warm-up of every variant; the variants alternate inside every round.

--accuracy: the shares of bytes that differ from the float64 reference (tests/motion_spec_ref.py) on the cases of
tests/test_motion_spec_packed_gpu.py::test_full_frames_against_the_float64_reference, for the PLANAR calls on the component planes (the
test's constants PLANAR_SHARE: the worst filter case per mode) and for the packed call."""
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


def family(torch, frames, which, mode):
    """the four variants of one plan family and type on the same clip"""
    from dspfun_amd.engine import motion_grid_plans, motion_packed, motion_packed_frame_plans, motion_spec_constants
    import motion_spec_ref as sr
    block = (8, 8, 8) if which == "A" else (1, H, W)
    if which == "A":
        packed_plan, _, _ = motion_grid_plans((frames, H, W), block, block)
        planar_plan = packed_plan
        k = motion_spec_constants(block)
    else:
        packed_plan, _, k = motion_packed_frame_plans(frames, H, W, C)
        planar_plan = sr.stack_plan(block, frames, sr.ol.REDFT10)
    pk = motion_packed("rgb24", normalization=k["normalization"], scalefactor=k["scalefactor"])
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, (frames, H, W, C), dtype=torch.uint8, device="cuda", generator=gen)
    dst, dst2 = torch.zeros_like(src), torch.zeros_like(src)
    planes_in = src.permute(3, 0, 1, 2).contiguous()
    planes_out = torch.zeros_like(planes_in)
    work = torch.empty(src.numel() if which == "B" else frames * H * W, dtype=torch.float32, device="cuda")
    quantizer = QUANT * 8 * math.sqrt(float(block[0] * block[1] * block[2]))          # motion.c:570
    filt = dict(active=block, minbuf_hw=block[1:], block_depth=block[0], band_begin=(0, 0, 0), band_end=block, damp=0.0, boost=1.0, quantizer=quantizer)
    stream = torch.cuda.current_stream().cuda_stream
    sf, nm, c = k["scalefactor"], k["normalization"], k["c"]

    def run_packed():
        packed_plan.spectrogram_packed(src.data_ptr(), dst.data_ptr(), mode, sf, nm, pk, c=c, d_work=work.data_ptr() if which == "B" else 0, filter=filt, stream=stream)

    def planar(pin, pout):
        for i in range(C):
            planar_plan.spectrogram(pin[i].data_ptr(), pout[i].data_ptr(), mode, sf, nm, c, d_work=work.data_ptr() if which == "B" else 0, filter=filt, stream=stream)

    def run_planar():
        planar(planes_in, planes_out)

    def run_composed():
        pin = src.permute(3, 0, 1, 2).contiguous()
        planar(pin, planes_out)
        dst2.copy_(planes_out.permute(1, 2, 3, 0))

    def run_copy():
        dst2.copy_(src)
    run_packed()
    run_composed()
    torch.cuda.synchronize()
    differ = int((dst != dst2).sum())
    if which == "A" and differ:
        raise SystemExit(f"bench_motion_spec_packed: {mode}: the packed bytes differ from the composed planar calls in {differ} places")
    return dict(packed=run_packed, composed=run_composed, planar=run_planar, copy=run_copy), src.numel(), differ, packed_plan.describe()


def accuracy(torch, lines):
    import numpy as np
    import motion_spec_ref as sr
    import test_motion_spec_packed_gpu as tp
    from dspfun_amd.engine import motion_packed_frame_plans
    h, w = tp.REF_BLOCK[1:]
    fwd, inv, info = motion_packed_frame_plans(tp.REF_FRAMES, h, w, 3)
    lines.append(f"# share of bytes that differ from the float64 reference, {tp.REF_FRAMES} x {h} x {w} rgb24, seeds {tp.REF_SEEDS}; max byte difference in brackets")
    lines.append("# dir   mode   filter   planar calls on the planes        packed call")
    worst = {}
    for inverse, modes in ((False, tp.SPEC_MODES), (True, tp.ISPEC_MODES)):
        planar_plan = sr.stack_plan(tp.REF_BLOCK, tp.REF_FRAMES, sr.ol.REDFT01 if inverse else sr.ol.REDFT10)
        for mode in modes:
            for kind in (None, "band", "full", "q"):
                clip, refs = tp.ref_case(inverse, mode, kind)
                filt = refs[0]["filt"]
                got, _ = tp.run_packed(torch, inv if inverse else fwd, inverse, clip, mode, info, tp.packed_of(filt), filt, work=True)
                row = []
                for out in ([sr.fused(torch, planar_plan, inverse, clip[..., k], tp.REF_BLOCK, mode, filt, with_work=True)[0] for k in range(3)], [got[..., k] for k in range(3)]):
                    mx = n = size = 0
                    for k, ref in enumerate(refs):
                        m, d, s = sr.share_of(out[k], ref["out8"], ref["tie"])
                        mx, n, size = max(mx, m), n + d, size + s
                    row.append((mx, n, size))
                d = "ispec" if inverse else "spec"
                worst[(d, mode)] = max(worst.get((d, mode), 0.0), row[0][1] / row[0][2])
                lines.append(f"{d:6s} {mode:6s} {str(kind):7s} " + "   ".join(f"{n:5d} of {size:5d} = {n / size:.6e} [{mx}]" for mx, n, size in row))
    lines.append("# PLANAR_SHARE (the worst filter case per mode): " + ", ".join(f"{d} {m}: {v:.5e}" for (d, m), v in worst.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_spec_packed: no GPU visible", file=sys.stderr)
        return 2
    lines = []
    if args.accuracy:
        accuracy(torch, lines)
    else:
        lines += [f"# motion --spectrogram -q {QUANT:g} on rgb24, {W}x{H}x{args.frames}, {torch.cuda.get_device_name(0)}",
                  f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); GB/s of the clip read once and written once"]
        for which in ("A", "B"):
            for mode in ("shift", "abs"):
                runs, nbytes, differ, desc = family(torch, args.frames, which, mode)
                name = "-b 8x8x8" if which == "A" else "-b 0x0x1"
                if mode == "shift":
                    lines += [f"# {which} {name}: {l}" for l in desc.splitlines() if l.startswith("ax")]
                if which == "B":
                    lines.append(f"# {which} {mode}: {differ} of {nbytes} packed bytes differ from the composed planar calls' (another rounding in the last place of the transform)")
                t = timed(torch, runs)
                med = {k: statistics.median(v) for k, v in t.items()}
                for key, v in t.items():
                    tag = {"packed": "1. packed call", "composed": f"2. split + {C} planar calls + interleave", "planar": f"3. {C} planar calls alone", "copy": "4. device copy of the clip"}[key]
                    lines.append(f"{which} {name} {mode:5s} {tag:40s} {med[key]:8.3f} ms ({min(v):.3f} .. {max(v):.3f})  {2 * nbytes / med[key] / 1e6:8.1f} GB/s")
                lines.append(f"{which} {name} {mode:5s} composed / packed = {med['composed'] / med['packed']:.2f}, planar / packed = {med['planar'] / med['packed']:.2f}")
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
