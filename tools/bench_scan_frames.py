"""scan's output frames on the device at config 4 (7680x4320 RGB, zigzag, step 2^20: 32 frames): ms per frame for the fused step alone and
for step + frame composition (dspfft_scanframes_*) in each mode (plain, -v, -s, -i, -M, -P, all), and the host/scan_dev --video loop.
Prints one JSON line per mode.  Run alone for timings; under rocprofv3 --kernel-trace --stats for the per-kernel split.

  python tools/bench_scan_frames.py [--frames N] [--video-frames N]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, STEP = 7680, 4320, 1 << 20
MODES = [("plain", {}), ("v", dict(visualize=True)), ("s", dict(spectrogram=True)), ("i", dict(intermediates=True)),
         ("M", dict(max_intermediates=True)), ("P", dict(parity_depth=8)),
         ("all", dict(spectrogram=True, max_intermediates=True, parity_depth=8))]
BW = 6.1e12          # the model's sustained HBM bandwidth (bytes / s)


def model_bytes(o):
    """bytes compose (+ mark) moves per frame: sum read (+ write with -i), top-left written; -i: image read + refilled, bottom-left written,
    -M: image read once more; -P: original read; -v: the owner table read, the frame's marks written (a 2^20 / 33 M sliver)"""
    n = W * H * 3 * 4
    b = 2 * n
    i = o.get("intermediates") or o.get("max_intermediates")
    if i:
        b += n + 3 * n
    if o.get("max_intermediates"):
        b += n
    if o.get("parity_depth"):
        b += n
    if o.get("visualize") or o.get("spectrogram"):
        b += W * H * 4 + (3 if i else 2) * STEP * 3 * 4
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--video-frames", type=int, default=8)
    args = ap.parse_args()
    import torch
    from dspfun_amd import Plan, REDFT10, REDFT01, ScanFrames
    from dspfun_amd import _lib
    L = _lib.load()
    n, npix = W * H * 3, W * H
    g = torch.Generator(device="cuda"); g.manual_seed(0xD5F0004)
    img = torch.rand(n, device="cuda", generator=g)
    co = img.clone()
    Plan.image(H, W, 3, REDFT10).set_scale(1.0 / (4.0 * W * H)).execute(co.data_ptr())
    ids = torch.empty(npix, dtype=torch.int32, device="cuda")
    owner = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_frame_ids(ids.data_ptr(), 2, W, H, STEP, None) == 0
    assert L.dspfft_scan_owner_index(owner.data_ptr(), 2, W, H, None) == 0
    inv = Plan.image(H, W, 3, REDFT01)
    inv.scan_prepare(ids.data_ptr(), 3)
    work = torch.empty(n, device="cuda")
    nframes = min(args.frames, (npix + STEP - 1) // STEP)
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        fn(0)                                   # warm: kernels loaded
        torch.cuda.synchronize()
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            for f in range(nframes):
                fn(f)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / nframes * 1e3
            best = dt if best is None else min(best, dt)
        return best

    s = co[:3].repeat(npix).contiguous()
    step_ms = timed(lambda f: inv.execute_masked_accumulate(co.data_ptr(), work.data_ptr(), s.data_ptr(), ids.data_ptr(), f, 3, stream=st))
    del s
    for name, o in MODES:
        sf = ScanFrames(W, H, **o)
        frame = torch.empty(sf.frame_floats, device="cuda")
        s = co[:3].repeat(npix).contiguous()
        image = torch.full((n,), -0.0, device="cuda") if sf.intermediates else None
        sf.begin(frame, co, stream=st)

        def one(f):
            if sf.visualize:
                sf.mark_range(frame, co, owner, f * STEP, (f + 1) * STEP, True, stream=st)
            acc = image if image is not None else s
            inv.execute_masked_accumulate(co.data_ptr(), work.data_ptr(), acc.data_ptr(), ids.data_ptr(), f, 3, stream=st)
            sf.compose(frame, s, image, co, img if o.get("parity_depth") else None, f, stream=st)
        ms = timed(one)
        model = model_bytes(o) / BW * 1e3
        print(json.dumps({"mode": name, "size": f"{W}x{H}", "frames": nframes, "step_ms": round(step_ms, 4), "step_plus_frame_ms": round(ms, 4),
                          "frame_ms": round(ms - step_ms, 4), "model_frame_ms": round(model, 4), "ratio_to_model": round((ms - step_ms) / model, 2),
                          "frame_bytes": sf.frame_floats * 4}), flush=True)
        del sf, frame, s, image
        torch.cuda.empty_cache()
    # host/scan_dev --video: the D2H copy of every frame (1.6 GB with -v -i) bounds it
    if args.video_frames:
        with tempfile.TemporaryDirectory() as tmp:
            pf = os.path.join(tmp, "in.pf")
            with open(pf, "wb") as f:
                f.write(b"PF\n%d %d\n-1.0\n" % (W, H))
                f.write(img.cpu().numpy().astype("<f4").tobytes())
            for opts in (["-v"], ["-v", "-i"]):
                times = []
                for nf in (2, 2 + args.video_frames):
                    cmd = [os.path.join(ROOT, "host", "scan_dev"), pf, os.path.join(tmp, "out.pf"), str(STEP), "zigzag", "--frames", str(nf),
                           "--video", "/dev/null"] + opts
                    t0 = time.perf_counter()
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                    times.append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr
                fb = 3 * W * 2 * H * (2 if "-i" in opts else 1) * 4
                ms = (times[1] - times[0]) / args.video_frames * 1e3
                print(json.dumps({"mode": "video " + " ".join(opts), "frames": args.video_frames, "ms_per_frame": round(ms, 2), "frame_bytes": fb,
                                  "GB_per_s": round(fb / ms / 1e6, 1), "note": "difference of two whole runs (2 and 2 + N frames) over N; frames to /dev/null"}),
                      flush=True)


if __name__ == "__main__":
    main()
