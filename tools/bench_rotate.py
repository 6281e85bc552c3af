"""rotate on a 1920x1080x64 clip (rotate.hip's kernels) at one-byte and four-byte elements, one GPU:

    python tools/bench_rotate.py [--out FILE] [--frames 64] [--reps 20]

For the 6 axis orders x 8 sign sets: ms per dspfft_rotate call (the C ABI call with its arguments made once; median of --reps timed calls, each
between its own pair of device events, after 5 warm-up calls; the call and torch's alternate inside every round) beside, in the same process
on the same buffers,
  copy   a device-to-device copy of the same bytes: the floor, nothing that reads and writes every byte once beats it
  torch  torch.flip(...).permute(...).contiguous() for the same map (a clone for the unsigned identity): what a user has without this call
and the two ratios: rotate / copy, and torch / rotate (above 1: the new call is faster).  Every rotated clip is compared with torch's, byte
for byte, before it is timed.  Random non-zero bytes.  A map on which the new call is more than 3 % slower than torch is marked LOSES."""
import argparse
import ctypes as C
import itertools
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
WARM = 5


def once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(torch, fns, reps):
    """fns alternate inside every round; (median, min, max) ms per function"""
    for fn in fns:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(once(torch, fn))
    return [(statistics.median(v), min(v), max(v)) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--orders", default="xyz,xzy,yxz,yzx,zxy,zyx")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_rotate: no GPU visible", file=sys.stderr)
        return 2
    from dspfun_amd import rotate, _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    reps = max(20, args.reps)
    lines = [f"# rotate, {W}x{H}x{args.frames}, {torch.cuda.get_device_name(0)}",
             f"# ms per call: median of {reps} calls, each between its own device events, after {WARM} warm-ups (min .. max); rotate and torch alternate",
             "# copy: device-to-device copy of the same bytes; torch: flip / permute / contiguous for the same map; same process, same buffers"]
    gen = torch.Generator(device="cuda").manual_seed(15)
    losers = []
    for E in (1, 4):
        raw = torch.randint(1, 256, (args.frames, H, W * E), dtype=torch.uint8, device="cuda", generator=gen)
        vol = raw if E == 1 else raw.view(torch.float32)
        nbytes = raw.numel()
        dst = torch.empty_like(vol)
        copy_ms = timed(torch, [lambda: dst.copy_(vol)], reps)[0]
        lines.append(f"# E = {E} ({'uint8' if E == 1 else 'float32'}): {nbytes / 1e6:.1f} MB each way; copy {copy_ms[0]:.3f} ms ({copy_ms[1]:.3f} .. {copy_ms[2]:.3f}), "
                     f"{2 * nbytes / copy_ms[0] / 1e6:.0f} GB/s read + written")
        lines.append(f"# {'map':8s} {'rotate ms':>10s} {'(min .. max)':>18s} {'GB/s':>7s} {'/copy':>6s} {'torch ms':>10s} {'torch/rotate':>12s}")
        for order in args.orders.split(","):
            for signs in itertools.product(("", "-"), repeat=3):
                spec = "".join(s + l for s, l in zip(signs, order))
                m, inv = rotate.parse(spec)
                flips = [2 - a for a in range(3) if inv[m[a]]]
                perm = (2 - m[2], 2 - m[1], 2 - m[0])

                def by_torch():
                    v = torch.flip(vol, flips) if flips else vol
                    return v.permute(perm).contiguous() if (flips or perm != (0, 1, 2)) else v.clone()
                out = torch.empty(rotate.geometry(spec, (W, H, args.frames))["out_shape"], dtype=vol.dtype, device="cuda")
                rotate.rotate(torch, vol, spec, out=out)
                want = by_torch()
                same = torch.equal(out.view(torch.uint8), want.view(torch.uint8))
                del want
                if not same:
                    lines.append(f"  {spec:8s} WRONG BYTES")
                    losers.append((E, spec, "wrong bytes"))
                    continue
                # the C ABI call itself, its arguments made once: at 0.04 ms a call the Python wrapper's own time would be what is measured
                cargs = (out.data_ptr(), vol.data_ptr(), (C.c_uint64 * 3)(W, H, args.frames), E, (C.c_int * 3)(*m), (C.c_int * 3)(*inv), stream)
                r, t = timed(torch, [lambda: lib.dspfft_rotate(*cargs), by_torch], reps)
                lose = r[0] > 1.03 * t[0]
                if lose:
                    losers.append((E, spec, f"{r[0] / t[0]:.2f}x torch's time"))
                lines.append(f"  {spec:8s} {r[0]:10.3f} {f'({r[1]:.3f} .. {r[2]:.3f})':>18s} {2 * nbytes / r[0] / 1e6:7.0f} {r[0] / copy_ms[0]:6.2f} {t[0]:10.3f} {t[0] / r[0]:12.2f}"
                             + ("  LOSES" if lose else ""))
                del out
        del raw, vol, dst
        torch.cuda.empty_cache()
    lines.append(f"# maps more than 3 % slower than torch: {losers if losers else 'none'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
