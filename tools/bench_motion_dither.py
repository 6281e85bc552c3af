"""motion's -d on the device: the C5 luma clip (1920x1080x256) dithered against undithered, as one 3-D block and as per-frame blocks (the
sliced path), and the dither kernel alone (dspfft_motion_dither_u8 over the clip's 256 planes).  Prints one JSON line.
Kernel rows: run under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_motion_dither.py` in a run of its own.
DSPFFT_DITHER_WAVES=1 selects the one-wave-per-plane schedule for an A/B run."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dspfun_amd import Plan, REDFT10, REDFT01  # noqa: E402
from dspfun_amd.engine import motion_dither_u8  # noqa: E402


def timeit(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    d_, h, w = 256, 1080, 1920
    r2 = math.sqrt(2.0)
    nm = 1 / math.sqrt(8.0 * d_ * h * w)
    res = {"clip": f"{w}x{h}x{d_} u8", "dither_waves": os.environ.get("DSPFFT_DITHER_WAVES", "16")}
    src = torch.randint(0, 256, (d_, h, w), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    work = torch.empty((d_, h, w), device="cuda")
    # one 3-D block (motion -b 1920x1080x256)
    fwd = Plan.many_r2r([d_, h, w], [REDFT10] * 3).set_scale(2 * r2)
    inv = Plan.many_r2r([d_, h, w], [REDFT01] * 3, first_axis_first=True).set_scale(1.0 / (2 * r2) / (8.0 * d_ * h * w) / nm / nm)
    for a in range(3):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
        inv.set_axis_scale0(a, r2, 1.0)
    res["block3d_undithered_ms"] = round(timeit(lambda: fwd.roundtrip_u8(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), nm * nm)), 3)
    res["block3d_dithered_ms"] = round(timeit(lambda: fwd.roundtrip_u8_dither(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), 1.0, nm)), 3)
    del fwd, inv
    # per-frame blocks (motion's default -b 0x0x1; the sliced path)
    nm2 = 1 / math.sqrt(8.0 * h * w)
    fwd = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=d_, idist=h * w, odist=h * w).set_scale(2.0)
    inv = Plan.many_r2r([h, w], [REDFT01] * 2, howmany=d_, idist=h * w, odist=h * w, first_axis_first=True).set_scale(1.0 / 2.0 / (4.0 * h * w) / nm2 / nm2)
    for a in range(2):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
        inv.set_axis_scale0(a, r2, 1.0)
    res["frames_undithered_ms"] = round(timeit(lambda: fwd.roundtrip_u8(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), nm2 * nm2)), 3)
    res["frames_dithered_ms"] = round(timeit(lambda: fwd.roundtrip_u8_dither(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), 1.0, nm2)), 3)
    res["frames_path"] = "sliced" if "roundtrip_u8 in slices of" in fwd.describe() else "whole"
    # the dither kernel alone over the clip's planes
    work.uniform_(-20.0, 275.0)
    res["dither_kernel_ms"] = round(timeit(lambda: motion_dither_u8(dst.data_ptr(), work.data_ptr(), (d_, h, w), scalefactor=1.0, normalization=1.0)), 3)
    res["dither_kernel_GBps"] = round(d_ * h * w * 5 / res["dither_kernel_ms"] / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
