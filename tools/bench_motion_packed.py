"""motion -b 8x8x8 -q 20 -c pixel_format=rgb24 (and rgba) on a 1920x1080x64 packed 8-bit clip (block_packed.hip's kernel), one GPU:

    python tools/bench_motion_packed.py [--out FILE] [--g 0,1,2,4] [--frames 64] [--block 8x8x8]

ms per call, medians over rounds with the spread, for
  1. packed      the packed call, dspfft_execute_roundtrip_u8_packed: 2 C bytes per pixel
  2. composed    what a user had before: de-interleave with torch (permute + contiguous), C planar roundtrip_u8 calls on the same plan pair,
                 interleave again (permute + contiguous): about 6 C bytes per pixel
  3. planar      the C planar calls alone, on planes that are already apart: 2 C bytes per pixel
  4. copy        a device copy of the clip: 2 C bytes per pixel, the floor of anything that reads and writes it once
The packed bytes are checked against (2) before any time is printed.  Device events around REPS calls after a warm-up of every variant; the
variants alternate inside every round.  --g: pixel blocks per workgroup to try (DSPFFT_PACKED_G, read on every call; 0: the engine's rule).
--block DxHxW: other block extents (the tile-size sweeps behind the engine's rule)."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, REPS = 7, 20
HEIGHT, W = 1080, 1920
QUANT = 20.0


def cases(torch, frames, fmt, BLOCK):
    from dspfun_amd.engine import motion_grid_plans, motion_packed
    # (rows that fill no whole block are left off: 1080 rows are whole 8-row blocks; with a remainder and several blocks along time the planar
    # pair of 16- and 32-row blocks is no pair of the fused block pass today, for the planar call either)
    H = HEIGHT // BLOCK[1] * BLOCK[1]
    fwd, inv, info = motion_grid_plans((frames, H, W), BLOCK, BLOCK)
    packed = motion_packed(fmt, normalization=info["normalization"], scalefactor=info["scalefactor"])
    comps = packed.components
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, (frames, H, W, comps), dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.zeros_like(src)
    dst2 = torch.zeros_like(src)
    planes_in = src.permute(3, 0, 1, 2).contiguous()
    planes_out = torch.zeros_like(planes_in)
    work = torch.empty((frames, H, W), dtype=torch.float32, device="cuda")
    quantizer = QUANT * 8 * math.sqrt(float(BLOCK[0] * BLOCK[1] * BLOCK[2]))          # motion.c:570
    filt = dict(active=BLOCK, minbuf_hw=BLOCK[1:], block_depth=BLOCK[0], band_begin=(0, 0, 0), band_end=BLOCK, damp=0.0, boost=1.0, quantizer=quantizer)
    stream = torch.cuda.current_stream().cuda_stream
    mul = info["out_mul"]

    def run_packed():
        fwd.roundtrip_u8_packed(inv, src.data_ptr(), dst.data_ptr(), mul, packed, filter=filt, stream=stream)

    def planar(pin, pout):
        for c in range(comps):
            fwd.roundtrip_u8(inv, pin[c].data_ptr(), pout[c].data_ptr(), work.data_ptr(), mul, filter=filt, stream=stream)

    def run_planar():
        planar(planes_in, planes_out)

    def run_composed():
        pin = src.permute(3, 0, 1, 2).contiguous()
        planar(pin, planes_out)
        dst2.copy_(planes_out.permute(1, 2, 3, 0))

    def run_copy():
        dst2.copy_(src)
    # rows below the last whole block are written by nobody: zero in both results
    run_packed()
    run_composed()
    torch.cuda.synchronize()
    if not torch.equal(dst, dst2):
        raise SystemExit(f"bench_motion_packed: {fmt}: the packed bytes differ from the composed planar calls in {int((dst != dst2).sum())} places")
    return dict(packed=run_packed, composed=run_composed, planar=run_planar, copy=run_copy), src.numel(), comps, next(l for l in fwd.describe().splitlines() if "BLOCK" in l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--g", default="0", help="comma-separated pixel blocks per workgroup to try; 0: the engine's rule")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--block", default="8x8x8", help="block extents DxHxW")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_packed: no GPU visible", file=sys.stderr)
        return 2
    from dspfun_amd.engine import DspfftError
    gs = [int(v) for v in args.g.split(",")]
    block = tuple(int(v) for v in args.block.split("x"))
    lines = [f"# motion -b {args.block} (DxHxW) -q {QUANT:g} on packed 8-bit pixels, {W}x{HEIGHT // block[1] * block[1]}x{args.frames}, {torch.cuda.get_device_name(0)}",
             f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); GB/s of the clip read once and written once",
             "# every format's packed bytes equal the composed planar calls' (checked before timing)"]
    for fmt in ("rgb24", "rgba"):
        os.environ.pop("DSPFFT_PACKED_G", None)
        try:
            runs, nbytes, comps, desc = cases(torch, args.frames, fmt, block)
        except DspfftError as e:                                 # (16x16x16 at four components does not fit LDS)
            lines.append(f"# {fmt}: refused: {e}")
            continue
        lines.append(f"# {fmt}: planar plan: {desc}")
        keys = [("packed", g) for g in gs] + [("composed", 0), ("planar", 0), ("copy", 0)]
        t = {k: [] for k in keys}
        for _ in range(ROUNDS):
            for key in keys:
                if key[0] == "packed" and key[1]:
                    os.environ["DSPFFT_PACKED_G"] = str(key[1])
                else:
                    os.environ.pop("DSPFFT_PACKED_G", None)
                run = runs[key[0]]
                run()                                            # (a variant's first call of the round: not timed)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    run()
                e1.record()
                e1.synchronize()
                t[key].append(e0.elapsed_time(e1) / REPS)
        os.environ.pop("DSPFFT_PACKED_G", None)
        for key, v in t.items():
            med = statistics.median(v)
            tag = {"packed": f"1. packed call G'={key[1] or 'rule'}", "composed": f"2. split + {comps} planar calls + interleave", "planar": f"3. {comps} planar calls alone",
                   "copy": "4. device copy of the clip"}[key[0]]
            lines.append(f"{fmt:6s} {tag:42s} {med:8.3f} ms ({min(v):.3f} .. {max(v):.3f})  {2 * nbytes / med / 1e6:8.1f} GB/s  ({2 * nbytes / 1e6:.1f} MB)")
        del runs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
