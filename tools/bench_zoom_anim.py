"""zoom's animation loop on one MI355X: ms per frame of the animation object (dspfft_zoomanim_*, a new scale every frame) against
Zoom.frame(method="czt") called with the same per-frame scales (today's route: a chirp-z object created, and the least recently used
one destroyed, per new scale) and against a fixed-scale dspfft_zoomczt frame of the same geometry.  Prints one JSON line per case.
Run alone for timings; under rocprofv3 --kernel-trace --stats for the per-kernel split.

  python tools/bench_zoom_anim.py [--frames N] [--replan-frames N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fn, n):
    """host clock around n calls, synchronised at both ends: ms per call"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--replan-frames", type=int, default=24)
    a = ap.parse_args()
    import torch
    import oracle_lib as ol
    from dspfun_amd.zoom import Zoom, INTERPOLATED
    n = a.frames
    # (name, source w x h, view vw x vh, basis, per-frame (xscale, vx, vy) of frame i of n)
    cases = [
        ("zoom-in 1x..4x, 1080p view", 1920, 1080, 1920, 1080, INTERPOLATED, lambda i: (1.0 + 3.0 * i / (n - 1), 0.5 * i, 0.25 * i)),
        ("config 3, scales 3.9..4.1", 1920, 1080, 7680, 4320, INTERPOLATED, lambda i: (3.9 + 0.2 * i / (n - 1), 0.0, 0.0)),
        ("pan at 4x, 1080p view", 1920, 1080, 1920, 1080, INTERPOLATED, lambda i: (4.0, 3.0 * i, 2.0 * i)),
    ]
    for name, w, h, vw, vh, btype, state in cases:
        x = torch.from_numpy(ol.synth_f32(0xD5F2C00, h * w * 3).reshape(h, w, 3)).to("cuda:0")
        z = Zoom(torch, x)
        anim = z.animation(vw, vh, btype)
        out = torch.empty((vh, vw, 3), dtype=torch.float32, device="cuda:0")
        outp = torch.empty((3, vh, vw), dtype=torch.float32, device="cuda:0")

        def anim_frame(i, layout="rgb", show=0):
            s, vx, vy = state(i % n)
            anim.frame((s, 1.0), (s, 1.0), vx, vy, show, layout, out=out if layout == "rgb" else outp)
        anim_frame(0)
        ms_anim = timed(torch, anim_frame, n)
        ms_gbr = timed(torch, lambda i: anim_frame(i, "gbr"), n)
        ms_grid = timed(torch, lambda i: anim_frame(i, "gbr", 2), n)
        s0, vx0, vy0 = state(n // 2)
        z.frame(vw, vh, (s0, 1.0), (s0, 1.0), vx0, vy0, btype, method="czt")
        ms_fixed = timed(torch, lambda i: z.frame(vw, vh, (s0, 1.0), (s0, 1.0), state(i % n)[1], state(i % n)[2], btype, method="czt"), n)
        m = a.replan_frames

        def replan(i):
            s, vx, vy = state((i * n) // m)
            z.frame(vw, vh, (s, 1.0), (s, 1.0), vx, vy, btype, method="czt")
        replan(0)
        ms_replan = timed(torch, lambda i: replan(i + 1), m - 1)
        print(json.dumps({"case": name, "view": f"{vw}x{vh}", "frames": n, "anim_ms": round(ms_anim, 3), "anim_gbr_ms": round(ms_gbr, 3),
                          "anim_gbr_grid_ms": round(ms_grid, 3), "fixed_scale_czt_ms": round(ms_fixed, 3),
                          "replan_czt_ms": round(ms_replan, 3), "replan_frames": m - 1,
                          "anim_over_fixed": round(ms_anim / ms_fixed, 3), "replan_over_anim": round(ms_replan / ms_anim, 2)}), flush=True)
        del anim, z
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
