"""motion -b 1x1xD (-s 1x1xD') on a 1920x1080x256 8-bit luma clip (temporal_rt.hip's kernel), one GPU:

    python tools/bench_motion_temporal.py [--out FILE] [--k 0,16,32] [--frames 256]

ms per call and GB/s against the 2 B/sample of compulsory traffic (input + output bytes) for D -> D' = 256 -> 256, 8 -> 8 and 24 -> 30
(240 of the 256 frames: 256 is no multiple of 24), each beside its comparator, the only thing the plans' own passes can run on this layout:
dspfft_u8_to_f32, the rank-1 forward plan, the rank-1 inverse plan, dspfft_f32_to_u8, no filter -- at least 18 B/sample.  For 24 -> 30 the
comparator's inverse runs in place over the 300 output frames' floats: the bytes a rescale would have to move at the very least, not its
result (the plans' own passes cannot rescale a batch).  Device events around REPS calls after a warm-up of every shape; the new call and its
comparator alternate inside every round and the medians over the rounds are reported with the spread (min .. max).
--k: tile widths to try (DSPFFT_TEMPORAL_K, read on every call; 0: the engine's rule, the widest of 128, 64, 32, 16 within 64 KB).  Each line
names the K in effect, the threads per workgroup and the workgroups a CU holds by LDS (160 KB) and threads (2048)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, REPS = 7, 3
H, W = 1080, 1920
PAIRS = [(256, 256), (8, 8), (24, 30)]
TABLES = 3072 + 16           # the transfer characteristic's tables and the coded count behind the tile


def tile(D, S, forced):
    m = max(D, S)
    k = 128
    while k > 16 and m * k * 4 > 64 * 1024:
        k //= 2
    if forced:
        k = min(k, forced)
    nthr = 512 if m * k > 8192 else 256
    return k, nthr, min((160 * 1024) // (m * k * 4 + TABLES), 2048 // nthr)


def cases(torch, frames, D, S):
    from dspfun_amd.engine import motion_temporal_plans, u8_to_f32_trc, f32_to_u8_trc
    fwd, inv, info = motion_temporal_plans((frames, H, W), D, S)
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(0, 256, (frames, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.empty(info["out_shape"], dtype=torch.uint8, device="cuda")
    nin, nout = info["in_shape"][0], info["out_shape"][0]
    work = torch.empty((max(nin, nout), H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def new():
        fwd.roundtrip_u8(inv, src.data_ptr(), dst.data_ptr(), None, info["out_mul"], stream=stream)

    def old():
        u8_to_f32_trc(src[:nin], None, out=work[:nin], stream=stream)
        fwd.execute(work.data_ptr(), stream=stream)
        inv.execute(work.data_ptr(), stream=stream)
        f32_to_u8_trc(work[:nout], None, mul=info["out_mul"], out=dst, stream=stream)
    nbytes = (nin + nout) * H * W
    return new, old, nbytes, fwd.describe().splitlines()[1] + " | " + inv.describe().splitlines()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--k", default="0", help="comma-separated tile widths to try; 0: the engine's rule")
    ap.add_argument("--frames", type=int, default=256)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_temporal: no GPU visible", file=sys.stderr)
        return 2
    ks = [int(v) for v in args.k.split(",")]
    lines = [f"# motion -b 1x1xD (-s 1x1xD'), 8-bit ends, {W}x{H}x{args.frames} luma, {torch.cuda.get_device_name(0)}",
             f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); GB/s of input + output bytes (2 B/sample)",
             "# comparator: dspfft_u8_to_f32 + rank-1 forward plan + rank-1 inverse plan + dspfft_f32_to_u8, no filter, same run"]
    for D, S in PAIRS:
        new, old, nbytes, desc = cases(torch, args.frames, D, S)
        lines.append(f"# {D} -> {S}: the plans' own passes: {desc}")
        os.environ.pop("DSPFFT_TEMPORAL_K", None)
        for _ in range(2):
            new(); old()
        torch.cuda.synchronize()
        t = {("old", 0): []}
        for k in ks:
            t[("new", k)] = []
        for _ in range(ROUNDS):
            for key in t:
                if key[0] == "new" and key[1]:
                    os.environ["DSPFFT_TEMPORAL_K"] = str(key[1])
                else:
                    os.environ.pop("DSPFFT_TEMPORAL_K", None)
                run = new if key[0] == "new" else old
                run()                                            # (a tile width's first call: not timed)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    run()
                e1.record()
                e1.synchronize()
                t[key].append(e0.elapsed_time(e1) / REPS)
        os.environ.pop("DSPFFT_TEMPORAL_K", None)
        base = statistics.median(t[("old", 0)])
        for key, v in t.items():
            med = statistics.median(v)
            if key[0] == "old":
                tag = "comparator (4 calls)"
            else:
                k, nthr, per_cu = tile(D, S, key[1])
                tag = f"fused K={k} threads={nthr} wg/CU={per_cu} ({base / med:.2f}x)"
            lines.append(f"{D:4d} -> {S:<4d} {tag:44s} {med:8.3f} ms ({min(v):.3f} .. {max(v):.3f})  {nbytes / med / 1e6:8.1f} GB/s  ({nbytes / 1e6:.1f} MB per call)")
        del new, old
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
