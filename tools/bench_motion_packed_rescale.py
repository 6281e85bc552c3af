"""motion -b with -s -q 20 -c pixel_format=rgb24 (and rgba) over the block grid of a 1920x1080x64 packed 8-bit clip
(block_rescale_packed.hip's kernel), one GPU:

    python tools/bench_motion_packed_rescale.py [--out FILE] [--g 1,2,4,...] [--frames 64] [--pairs 8x8x8-4x4x4,...] [--coeff-limit N] [-d]

ms per call, medians over rounds with the spread, for every pair (rgb24; rgba too for the first)
  1. launch      the one launch, dspfft_execute_roundtrip_u8_packed_rescale: C (input pixels + output pixels) bytes
  2. composed    what a user had before: de-interleave with torch (permute + contiguous), C planar grid calls (roundtrip_u8 on the same
                 pair), interleave again (permute + copy): about three times the bytes
  3. planar      the C planar grid calls alone, on planes that are already apart
GB/s is always against the bytes the call must move, C (input pixels + output pixels).  The launch's bytes are checked against (2) before
any time is printed.  Device events around REPS calls after an untimed call of the variant; the variants alternate inside every round.
--coeff-limit N, -d: the same rows for motion --coeff-limit N and / or -d on that grid (block_rescale_packed_limit.hip, block_rescale_packed_dither.hip:
dspfft_execute_roundtrip_u8_packed_rescale_limit / _dither against roundtrip_u8_limit / roundtrip_u8_dither per plane, the latter through one float
work buffer), and a fourth row, the plain packed rescaled call without either, as the floor.
--g: the pixel blocks per workgroup of the sweep (DSPFFT_PACKED_G, read on every call), run once per pair behind the main rounds; values
whose tile and tables do not fit 64 KB of LDS are left out (the engine would lower them)."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, REPS = 7, 10
SWEEP_ROUNDS = 3
HEIGHT, W = 1080, 1920
QUANT = 20.0
PAIRS = "8x8x8-4x4x4,4x4x4-8x8x8,1x8x8-1x16x16"
TABLES = 256 * 8 + 256 * 4 + 16


def cases(torch, frames, fmt, block, scaled, keep=0, dither=False):
    from dspfun_amd.engine import motion_grid_plans, motion_packed
    fwd, inv, info = motion_grid_plans((frames, HEIGHT, W), block, scaled)
    packed = motion_packed(fmt, normalization=info["normalization"], scalefactor=info["scalefactor"])
    comps = packed.components
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, tuple(info["in_shape"]) + (comps,), dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.zeros(tuple(info["out_shape"]) + (comps,), dtype=torch.uint8, device="cuda")
    dst2 = torch.zeros_like(dst)
    planes_in = src.permute(3, 0, 1, 2).contiguous()
    planes_out = torch.zeros((comps,) + tuple(info["out_shape"]), dtype=torch.uint8, device="cuda")
    minbuf = [max(b, s) for b, s in zip(block, scaled)]
    quantizer = QUANT * 8 * math.sqrt(float(scaled[0] * scaled[1] * scaled[2]))          # motion.c:570
    filt = dict(active=info["active"], minbuf_hw=minbuf[1:], block_depth=minbuf[0], band_begin=(0, 0, 0), band_end=info["active"], damp=0.0, boost=1.0,
                quantizer=quantizer)
    stream = torch.cuda.current_stream().cuda_stream
    mul = info["out_mul"]

    sf, nm, omul = info["scalefactor"], info["normalization"], info["limit_outside_mul"]
    work = torch.zeros(tuple(info["out_shape"]), dtype=torch.float32, device="cuda") if dither else None          # (the planar dithered call's, one plane at a time)

    def run_floor():
        fwd.roundtrip_u8_packed_rescale(inv, src.data_ptr(), dst.data_ptr(), mul, packed, filter=filt, stream=stream)

    def run_launch():
        if dither:
            fwd.roundtrip_u8_packed_rescale_dither(inv, src.data_ptr(), dst.data_ptr(), sf, nm, packed, filter=filt, coeff_limit=keep, outside_mul=omul, stream=stream)
        else:
            fwd.roundtrip_u8_packed_rescale(inv, src.data_ptr(), dst.data_ptr(), mul, packed, filter=filt, stream=stream, coeff_limit=keep, outside_mul=omul)

    def planar(pin, pout):
        for c in range(comps):
            if dither:
                fwd.roundtrip_u8_dither(inv, pin[c].data_ptr(), pout[c].data_ptr(), work.data_ptr(), sf, nm, filter=filt, stream=stream, coeff_limit=keep, outside_mul=omul)
            elif keep:
                fwd.roundtrip_u8_limit(inv, pin[c].data_ptr(), pout[c].data_ptr(), None, mul, coeff_limit=keep, outside_mul=omul, filter=filt, stream=stream)
            else:
                fwd.roundtrip_u8(inv, pin[c].data_ptr(), pout[c].data_ptr(), None, mul, filter=filt, stream=stream)

    def run_planar():
        planar(planes_in, planes_out)

    def run_composed():
        pin = src.permute(3, 0, 1, 2).contiguous()
        planar(pin, planes_out)
        dst2.copy_(planes_out.permute(1, 2, 3, 0))

    run_launch()
    run_composed()
    torch.cuda.synchronize()
    if not torch.equal(dst, dst2):
        raise SystemExit(f"bench_motion_packed_rescale: {fmt}: the launch's bytes differ from the composed planar calls in {int((dst != dst2).sum())} places")

    def check():
        torch.cuda.synchronize()
        return torch.equal(dst, dst2)
    runs = dict(launch=run_launch, composed=run_composed, planar=run_planar)
    if keep or dither:
        runs["floor"] = run_floor
    return runs, check, src.numel() + dst.numel(), comps


def timed(torch, run):
    run()                                            # (a variant's first call of the round: not timed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--g", default="1,2,3,4,5,6,7,8,10,12,16,20,24,32", help="comma-separated pixel blocks per workgroup of the sweep; empty: no sweep")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--pairs", default=PAIRS, help="comma-separated block-scaled pairs, DxHxW-DxHxW")
    ap.add_argument("--coeff-limit", type=int, default=0, help="motion --coeff-limit: coefficients kept per component block (0: none)")
    ap.add_argument("-d", dest="dither", action="store_true", help="motion -d: the Floyd-Steinberg store")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_packed_rescale: no GPU visible", file=sys.stderr)
        return 2
    gs = [int(v) for v in args.g.split(",") if v]
    pairs = [tuple(tuple(int(v) for v in side.split("x")) for side in p.split("-")) for p in args.pairs.split(",")]
    mode = (f" --coeff-limit {args.coeff_limit}" if args.coeff_limit else "") + (" -d" if args.dither else "")
    wide = bool(args.coeff_limit or args.dither)
    lines = [f"# motion -b with -s (DxHxW) -q {QUANT:g}{mode} on packed 8-bit pixels, {W}x{HEIGHT}x{args.frames}, {torch.cuda.get_device_name(0)}",
             f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); GB/s of C (input pixels + output pixels) bytes",
             f"# the sweep over DSPFFT_PACKED_G: median of {SWEEP_ROUNDS} rounds, run once behind the main rounds",
             "# every case's launch bytes equal the composed planar calls' (checked before timing, and again after the sweep)"]
    todo = [("rgb24", p) for p in pairs] + [("rgba", pairs[0])]
    for fmt, (block, scaled) in todo:
        name = "x".join(map(str, block)) + " -> " + "x".join(map(str, scaled))
        os.environ.pop("DSPFFT_PACKED_G", None)
        runs, check, nbytes, comps = cases(torch, args.frames, fmt, block, scaled, args.coeff_limit, args.dither)
        keys = ["launch", "composed", "planar"] + (["floor"] if wide else [])
        t = {k: [] for k in keys}
        for _ in range(ROUNDS):
            for key in keys:
                t[key].append(timed(torch, runs[key]))
        med = {k: statistics.median(v) for k, v in t.items()}
        tags = {"launch": "1. the one launch (G: the rule)", "composed": f"2. split + {comps} planar grid calls + interleave", "planar": f"3. {comps} planar grid calls alone",
                "floor": "4. the plain packed rescaled call (floor)"}
        for key in keys:
            v = t[key]
            lines.append(f"{fmt:6s} {name:22s} {tags[key]:44s} {med[key]:8.3f} ms ({min(v):.3f} .. {max(v):.3f})  {nbytes / med[key] / 1e6:8.1f} GB/s  ({nbytes / 1e6:.1f} MB)")
        verdict = "no slower than" if med["launch"] <= med["composed"] else "SLOWER than"
        if wide:          # the requirement: faster than the composition by more than the spread of either
            verdict = "faster than" if max(t["launch"]) < min(t["composed"]) else "NOT faster than"
        vs_planar = "" if not wide else (" (faster)" if max(t["launch"]) < min(t["planar"]) else " (NOT faster)")
        lines.append(f"{fmt:6s} {name:22s} the launch is {verdict} the composition: {med['composed'] / med['launch']:.2f} x; against the planar calls alone: {med['planar'] / med['launch']:.2f} x{vs_planar}")
        # the tile's columns per component block: the active ones; with a limit the embedding's, with -d alone `scaled`'s
        tw = max(block[2], scaled[2]) if args.coeff_limit else scaled[2] if args.dither else min(block[2], scaled[2])
        block_bytes = max(block[0], scaled[0]) * max(block[1], scaled[1]) * tw * comps * 4
        sweep = []
        for g in gs:
            lanes = min(64, math.ceil(scaled[0] * comps * g / 4))          # block_packed_core.h: packed_dither_lanes
            behind = (256 + 4 * lanes * scaled[2]) * 8 if args.dither else 0          # the error table and the rows of one lane per plane (the larger layout:
            # block_rs_packed_wide_core.h, rs_packed_wide_dither_bytes; the engine lowers a group that does not fit)
            if g * block_bytes + TABLES + behind > 64 * 1024 or g > W // block[2]:
                continue
            os.environ["DSPFFT_PACKED_G"] = str(g)
            v = [timed(torch, runs["launch"]) for _ in range(SWEEP_ROUNDS)]
            sweep.append(f"G={g}: {statistics.median(v):.3f}")
        os.environ.pop("DSPFFT_PACKED_G", None)
        if sweep:
            runs["launch"]()
            if not check():
                raise SystemExit(f"bench_motion_packed_rescale: {fmt} {name}: the bytes changed after the sweep")
            lines.append(f"{fmt:6s} {name:22s} sweep, ms: " + "  ".join(sweep))
        del runs, check
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
