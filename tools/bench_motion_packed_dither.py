"""motion -d on packed 8-bit pixels, 1920x1080x64 rgb24 and rgba, one GPU:

    python tools/bench_motion_packed_dither.py [--out FILE] [--frames 64] [--blocks 8x8x8,1x8x8] [--no-frames]

Small blocks (-b 8x8x8 -q 20 -d and -b 1x8x8 -q 20 -d), ms per call for
  a. one launch        dspfft_execute_roundtrip_u8_packed_dither: the dither runs in the block kernel's LDS tile, 2 C bytes per pixel
  b. composed          what a user had before: de-interleave with torch, C planar roundtrip_u8_dither calls on the same plan pair (each a block
                       kernel that writes floats and a dither kernel that reads them back), interleave again
  c. planar            the C planar dithered calls alone, on planes that are already apart
  d. undithered        dspfft_execute_roundtrip_u8_packed: the floor
Full frames (-b 0x0x1 -q 20 -d), rgb24:
  a. one call          dspfft_execute_roundtrip_u8_packed_frames_dither
  b. composition       dspfft_u8_to_f32 -> execute(fwd) -> motion_filter_packed -> execute(inv) -> dspfft_motion_dither_u8_packed
  c. composed planar   de-interleave, C planar per-frame roundtrip_u8_dither calls, interleave
  d. undithered        dspfft_execute_roundtrip_u8_packed_frames: the floor
(a)'s bytes are checked against (b)'s before any time is printed (full frames: against the composition; the planar per-frame kernels round in
the last place differently from the interleaved ones, and error diffusion amplifies that).  Device events around REPS calls after a warm-up call
of every variant; the variants alternate inside every round; medians over the rounds with the spread; random non-zero data."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS, REPS = 5, 8
HEIGHT, W = 1080, 1920
QUANT = 20.0


def timed(torch, runs, keys, reps):
    t = {k: [] for k in keys}
    for _ in range(ROUNDS):
        for key in keys:
            runs[key]()                                          # (a variant's first call of the round: not timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                runs[key]()
            e1.record()
            e1.synchronize()
            t[key].append(e0.elapsed_time(e1) / reps)
    return t


def report(lines, fmt, t, tags, nbytes):
    for key, v in t.items():
        med = statistics.median(v)
        lines.append(f"{fmt:6s} {tags[key]:50s} {med:8.3f} ms ({min(v):.3f} .. {max(v):.3f})  {2 * nbytes / med / 1e6:8.1f} GB/s  ({2 * nbytes / 1e6:.1f} MB)")


def block_case(torch, frames, fmt, BLOCK):
    from dspfun_amd.engine import motion_grid_plans, motion_packed
    H = HEIGHT // BLOCK[1] * BLOCK[1]
    fwd, inv, info = motion_grid_plans((frames, H, W), BLOCK, BLOCK)
    packed = motion_packed(fmt, normalization=info["normalization"], scalefactor=info["scalefactor"])
    comps = packed.components
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, (frames, H, W, comps), dtype=torch.uint8, device="cuda", generator=gen)
    dst, dst2 = torch.zeros_like(src), torch.zeros_like(src)
    planes_in = src.permute(3, 0, 1, 2).contiguous()
    planes_out = torch.zeros_like(planes_in)
    work = torch.empty((frames, H, W), dtype=torch.float32, device="cuda")
    quantizer = QUANT * 8 * math.sqrt(float(BLOCK[0] * BLOCK[1] * BLOCK[2]))          # motion.c:570
    filt = dict(active=BLOCK, minbuf_hw=BLOCK[1:], block_depth=BLOCK[0], band_begin=(0, 0, 0), band_end=BLOCK, damp=0.0, boost=1.0, quantizer=quantizer)
    stream = torch.cuda.current_stream().cuda_stream
    sf, nm, mul = info["scalefactor"], info["normalization"], info["out_mul"]

    def run_one():
        fwd.roundtrip_u8_packed_dither(inv, src.data_ptr(), dst.data_ptr(), sf, nm, packed, filter=filt, stream=stream)

    def planar(pin, pout):
        for c in range(comps):
            fwd.roundtrip_u8_dither(inv, pin[c].data_ptr(), pout[c].data_ptr(), work.data_ptr(), sf, nm, filter=filt, stream=stream)

    def run_planar():
        planar(planes_in, planes_out)

    def run_composed():
        pin = src.permute(3, 0, 1, 2).contiguous()
        planar(pin, planes_out)
        dst2.copy_(planes_out.permute(1, 2, 3, 0))

    def run_plain():
        fwd.roundtrip_u8_packed(inv, src.data_ptr(), dst2.data_ptr(), mul, packed, filter=filt, stream=stream)
    run_one()
    run_composed()
    torch.cuda.synchronize()
    if not torch.equal(dst, dst2):
        raise SystemExit(f"bench_motion_packed_dither: {fmt} {BLOCK}: the one launch's bytes differ from the composed planar dithered calls in {int((dst != dst2).sum())} places")
    run_plain()
    torch.cuda.synchronize()
    moved = float((dst != dst2).float().mean())
    runs = dict(one=run_one, composed=run_composed, planar=run_planar, plain=run_plain)
    tags = dict(one="a. one launch (dither in the LDS tile)", composed=f"b. split + {comps} planar dithered calls + interleave", planar=f"c. {comps} planar dithered calls alone",
                plain="d. undithered packed call")
    return runs, tags, src.numel(), moved


def frames_case(torch, frames):
    from dspfun_amd import _lib
    from dspfun_amd.engine import motion_dither_u8_packed, motion_filter_packed, motion_packed, motion_packed_frame_plans
    import motion_spec_ref as sr
    L = _lib.load()
    H, C = HEIGHT, 3
    block = (1, H, W)
    fwd, inv, k = motion_packed_frame_plans(frames, H, W, C)
    pfwd, pinv = sr.stack_plan(block, frames, sr.ol.REDFT10), sr.stack_plan(block, frames, sr.ol.REDFT01)
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, (frames, H, W, C), dtype=torch.uint8, device="cuda", generator=gen)
    dst, dst2 = torch.zeros_like(src), torch.zeros_like(src)
    planes_out = torch.zeros((C, frames, H, W), dtype=torch.uint8, device="cuda")
    work = torch.empty(src.numel(), dtype=torch.float32, device="cuda")
    quantizer = QUANT * 8 * math.sqrt(float(H * W))
    filt = dict(active=block, minbuf_hw=(H, W), block_depth=1, quantizer=quantizer, band_begin=(0, 0, 0), band_end=block)
    pk = motion_packed("rgb24", damp=1.0)
    per_plane = dict(filt, damp=1.0, boost=1.0)
    stream = torch.cuda.current_stream().cuda_stream
    sf, nm, mul = k["scalefactor"], k["normalization"], k["out_mul"]
    n = src.numel()

    def run_one():
        fwd.roundtrip_u8_packed_frames_dither(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), sf, nm, pk, filter=filt, stream=stream)

    def run_composition():
        if L.dspfft_u8_to_f32(work.data_ptr(), src.data_ptr(), n, stream):
            raise SystemExit("dspfft_u8_to_f32 failed")
        fwd.execute(work.data_ptr(), stream=stream)
        motion_filter_packed(work, H, W, C, frames, pk, filt, stream=stream)
        inv.execute(work.data_ptr(), stream=stream)
        motion_dither_u8_packed(dst2.data_ptr(), work.data_ptr(), (1, H, W), C, nblocks=(frames, 1, 1), block_step=(H * W, 0, 0), scalefactor=sf, normalization=nm, stream=stream)

    def run_composed():
        pin = src.permute(3, 0, 1, 2).contiguous()
        for i in range(C):
            pfwd.roundtrip_u8_dither(pinv, pin[i].data_ptr(), planes_out[i].data_ptr(), work.data_ptr(), sf, nm, filter=per_plane, stream=stream)
        dst2.copy_(planes_out.permute(1, 2, 3, 0))

    def run_plain():
        fwd.roundtrip_u8_packed_frames(inv, src.data_ptr(), dst2.data_ptr(), work.data_ptr(), mul, pk, filter=filt, stream=stream)
    run_one()
    run_composition()
    torch.cuda.synchronize()
    if not torch.equal(dst, dst2):
        raise SystemExit(f"bench_motion_packed_dither: full frames: the call's bytes differ from its composition's in {int((dst != dst2).sum())} places")
    run_composed()
    torch.cuda.synchronize()
    planar_differ = float((dst != dst2).float().mean())
    run_plain()
    torch.cuda.synchronize()
    moved = float((dst != dst2).float().mean())
    runs = dict(one=run_one, composition=run_composition, composed=run_composed, plain=run_plain)
    tags = dict(one="a. one call (_packed_frames_dither)", composition="b. composition with dspfft_motion_dither_u8_packed", composed=f"c. split + {C} planar dithered calls + interleave",
                plain="d. undithered packed-frames call")
    return runs, tags, n, moved, planar_differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--blocks", default="8x8x8,1x8x8", help="comma-separated block extents DxHxW")
    ap.add_argument("--no-frames", action="store_true", help="small blocks only")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_packed_dither: no GPU visible", file=sys.stderr)
        return 2
    lines = [f"# motion -q {QUANT:g} -d on packed 8-bit pixels, {W}x{HEIGHT}x{args.frames}, {torch.cuda.get_device_name(0)}",
             f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); GB/s of the clip read once and written once",
             "# (a)'s bytes equal (b)'s in every case (checked before timing)"]
    for spec in args.blocks.split(","):
        block = tuple(int(v) for v in spec.split("x"))
        for fmt in ("rgb24", "rgba"):
            runs, tags, nbytes, moved = block_case(torch, args.frames, fmt, block)
            lines.append(f"# -b {spec} (DxHxW) {fmt}: the dither moves {moved:.1%} of the undithered call's bytes")
            report(lines, fmt, timed(torch, runs, list(runs), REPS), tags, nbytes)
            del runs
            torch.cuda.empty_cache()
    if not args.no_frames:
        runs, tags, nbytes, moved, planar_differ = frames_case(torch, args.frames)
        lines.append(f"# -b 0x0x1 (full frames) rgb24: the dither moves {moved:.1%} of the undithered call's bytes; {planar_differ:.1%} of (c)'s bytes differ from (a)'s "
                     "(the planar kernels round in the last place differently, and the diffusion amplifies it)")
        report(lines, "rgb24", timed(torch, runs, list(runs), max(1, REPS // 4)), tags, nbytes)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
