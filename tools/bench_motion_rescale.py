"""motion -b with -s over a block grid on a 1920x1080x64 8-bit luma clip (volume layout, block_rescale.hip's kernel), one GPU:

    python tools/bench_motion_rescale.py [--out FILE] [--g 0,4,16] [--coeff-limit N]

ms per call and GB/s of (input + output bytes) for 8x8x8 -> 4x4x4, 8x8x8 -> 16x16x8, 8x8x1 -> 16x16x1 and 16x16x16 -> 8x8x8 (1072 of the
1080 rows: 1080 is no multiple of 16), and 8x8x8 -> 8x8x8 beside them: the block == scaled kernel (block_fused.hip), the yardstick.  Every
shape is measured for each G of --g (blocks per workgroup, DSPFFT_BLOCK_G at plan time; 0: the engine's own rule).  Device events around
REPS calls after a warm-up of every shape; the shapes alternate inside every round and the medians over the rounds are reported with
the spread (min .. max).
--coeff-limit N: motion --coeff-limit beside it (block_rescale_topn.hip's kernel through dspfft_execute_roundtrip_u8_limit): for 8x8x8 -> 4x4x4,
16x16x16 -> 8x8x8, 4x4x4 -> 8x8x8 and 2-D 32x32 -> 16x16 the plain grid call and the call with keep = N alternate inside every round, and
the ratio of their medians is reported: what the unpruned forward passes and the selection's 31 ballot rounds cost."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, REPS = 9, 5
CLIP = (64, 1080, 1920)
LIMIT_PAIRS = [((8, 8, 8), (4, 4, 4)), ((16, 16, 16), (8, 8, 8)), ((4, 4, 4), (8, 8, 8)), ((1, 32, 32), (1, 16, 16))]
PAIRS = [((8, 8, 8), (8, 8, 8)), ((8, 8, 8), (4, 4, 4)), ((8, 8, 8), (8, 16, 16)), ((1, 8, 8), (1, 16, 16)), ((16, 16, 16), (8, 8, 8))]


def name(block, scaled):
    return "x".join(str(v) for v in reversed(block)) + " -> " + "x".join(str(v) for v in reversed(scaled))


def case(torch, block, scaled, G, keep=0):
    """a closure that runs one call (keep: with that coefficient limit), and the bytes it moves; None when the plans are refused under this G"""
    from dspfun_amd import DspfftError
    from dspfun_amd.engine import motion_grid_plans
    if G:
        os.environ["DSPFFT_BLOCK_G"] = str(G)
    else:
        os.environ.pop("DSPFFT_BLOCK_G", None)
    # (2-D blocks: whole blocks only -- 1056 of the 1080 rows for 32 x 32 --, or the dense output volume's planes and rows of blocks merge into
    # one batch axis where the cropped input's do not, and the pair is refused)
    clip = CLIP if block[0] > 1 else (CLIP[0], CLIP[1] // block[1] * block[1], CLIP[2] // block[2] * block[2])
    try:
        fwd, inv, info = motion_grid_plans(clip, block, scaled)
    finally:
        os.environ.pop("DSPFFT_BLOCK_G", None)
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(0, 256, clip, dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.empty(info["out_shape"], dtype=torch.uint8, device="cuda")
    same = tuple(block) == tuple(scaled)
    if same and info["out_shape"] != CLIP:
        return None
    work = torch.empty(CLIP, dtype=torch.float32, device="cuda") if same else None      # (block == scaled: today's call takes a work buffer)
    st = dict(fwd=fwd, inv=inv, src=src, dst=dst, work=work, mul=info["out_mul"], stream=torch.cuda.current_stream().cuda_stream)

    def run():
        if keep:
            st["fwd"].roundtrip_u8_limit(st["inv"], st["src"].data_ptr(), st["dst"].data_ptr(), None, st["mul"], coeff_limit=keep,
                                         outside_mul=info["limit_outside_mul"], stream=st["stream"])
            return
        st["fwd"].roundtrip_u8(st["inv"], st["src"].data_ptr(), st["dst"].data_ptr(), st["work"].data_ptr() if st["work"] is not None else None,
                               st["mul"], stream=st["stream"])
    try:
        run()
        torch.cuda.synchronize()
    except DspfftError as e:
        print(f"# {name(block, scaled)} G={G}: refused ({e})")
        return None
    nbytes = int(torch.tensor(info["in_shape"]).prod()) + int(torch.tensor(info["out_shape"]).prod())
    return run, nbytes, fwd.describe().splitlines()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--g", default="0", help="comma-separated blocks per workgroup to try; 0: the engine's rule")
    ap.add_argument("--coeff-limit", type=int, default=0, help="also time every pair of the limit list with this many coefficients kept per block")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_rescale: no GPU visible", file=sys.stderr)
        return 2
    gs = [int(v) for v in args.g.split(",")]
    lines = [f"# motion -b with -s over a block grid, 8-bit ends, volume layout, {CLIP[2]}x{CLIP[1]}x{CLIP[0]} luma, {torch.cuda.get_device_name(0)}",
             f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); GB/s of input + output bytes; G = blocks per workgroup (0: the engine's rule)"]
    for G in gs:
        runs = {}
        for block, scaled in (LIMIT_PAIRS if args.coeff_limit else PAIRS):
            for keep in ((0, args.coeff_limit) if args.coeff_limit else (0,)):
                c = case(torch, block, scaled, G, keep)
                if c:
                    runs[(block, scaled) + ((keep,) if keep else ())] = c
        for run, _, _ in runs.values():
            for _ in range(2):
                run()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, (run, _, _) in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    run()
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1) / REPS)
        for k, (run, nbytes, _) in runs.items():
            med = statistics.median(t[k])
            tag = name(*k[:2]) + (f" keep {k[2]}" if len(k) > 2 else "")
            if len(k) > 2 and k[:2] in t:
                tag += f" ({med / statistics.median(t[k[:2]]):.2f}x plain)"
            lines.append(f"G={G:<3d} {tag:24s} {med:8.3f} ms ({min(t[k]):.3f} .. {max(t[k]):.3f})  {nbytes / med / 1e6:8.1f} GB/s  ({nbytes / 1e6:.1f} MB per call)")
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
