"""motion -b 8x8x8 --coeff-limit N on a 1920x1080x256 8-bit clip (volume layout, the fused block kernel), one GPU:

    python tools/bench_motion_topn.py [--out profiles/r07_motion_topn.txt]

  (a) roundtrip_u8 with a quantiser: block_roundtrip_kernel, the kernel without a selection stage
  (b) roundtrip_u8 with coeff_limit = 16 and the same filter: block_roundtrip_topn_kernel
  (c) coeff_limit = 16 on 16x16x16 blocks (1072 of the 1080 rows: 1080 is no multiple of 16) and coeff_limit = 2 on 4x4x1 blocks (16 of a
      block's 16 coefficients is the plain call), each beside its plain kernel
Device events around REPS calls, after a warm-up of every shape; (a) and (b) alternate inside every round and the medians over the
rounds are reported with the spread (min .. max).  Each call moves 2 B/sample of HBM traffic (8-bit in, 8-bit out)."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, REPS, KEEP, QUANT = 9, 5, 16, 20.0


def case(torch, block, D, H, W):
    from dspfun_amd import Plan
    bd, bh, bw = block
    dims = [d for d in [(bd, H * W, H * W), (bh, W, W), (bw, 1, 1)] if d[0] > 1]
    how = [(D // bd, bd * H * W, bd * H * W), (H // bh, bh * W, bh * W), (W // bw, bw, bw)]
    n = [d[0] for d in dims]
    r2 = math.sqrt(2.0)
    fwd = Plan.guru(dims, how, [5] * len(n)).set_scale(2 * r2)
    inv = Plan.guru(dims, how, [4] * len(n)).set_scale(1.0 / (2 * r2) / math.prod(2.0 * v for v in n))
    for a in range(len(n)):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
    assert "side by side" in fwd.describe(), fwd.describe()
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(0, 256, (D, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    flt = dict(active=block, minbuf_hw=(bh, bw), block_depth=bd, band_begin=(0, 0, 0), band_end=block,
               quantizer=QUANT * 8 * math.sqrt(bd * bh * bw))                      # motion.c:570
    st = dict(fwd=fwd, inv=inv, src=src, dst=torch.empty_like(src), work=torch.empty(D * H * W, device="cuda"), flt=flt,
              coded=torch.zeros(1, dtype=torch.int64, device="cuda"), stream=torch.cuda.current_stream().cuda_stream)

    def run(keep):
        st["fwd"].roundtrip_u8(st["inv"], st["src"].data_ptr(), st["dst"].data_ptr(), st["work"].data_ptr(), 1.0, filter=st["flt"],
                               d_coded=st["coded"].data_ptr(), stream=st["stream"], coeff_limit=keep)
    return run, D * H * W


def measure(torch, run, keeps):
    """ms per call for every keep in `keeps`, alternating inside each round: {keep: [one figure per round]}"""
    for k in keeps:
        for _ in range(2):
            run(k)
    torch.cuda.synchronize()
    out = {k: [] for k in keeps}
    for _ in range(ROUNDS):
        for k in keeps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                run(k)
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / REPS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_topn: no GPU visible", file=sys.stderr)
        return 2
    lines = [f"# motion --coeff-limit in the fused block kernel, 8-bit ends, volume layout, {torch.cuda.get_device_name(0)}",
             f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max); plain = the kernel without a selection stage"]
    for name, block, (D, H, W), keep in (("(a)/(b) 8x8x8 blocks, 1920x1080x256", (8, 8, 8), (256, 1080, 1920), KEEP),
                                         ("(c) 16x16x16 blocks, 1920x1072x256", (16, 16, 16), (256, 1072, 1920), KEEP),
                                         ("(c) 4x4x1 blocks, 1920x1080x256", (1, 4, 4), (256, 1080, 1920), 2)):
        run, samples = case(torch, block, D, H, W)
        t = measure(torch, run, (0, keep))
        med = {k: statistics.median(v) for k, v in t.items()}
        for k, label in ((0, "plain, quantiser"), (keep, f"keep = {keep}, quantiser")):
            lines.append(f"{name:38s} {label:24s} {med[k]:8.3f} ms ({min(t[k]):.3f} .. {max(t[k]):.3f})  {samples / med[k] / 1e6:8.1f} Gsamples/s  "
                         f"{2 * samples / med[k] / 1e6:7.1f} GB/s")
        lines.append(f"{name:38s} {'keep / plain':24s} {med[keep] / med[0]:8.3f}")
        del run
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
