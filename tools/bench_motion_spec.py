"""motion --spectrogram / --ispectrogram as one fused call on a 1920x1080x64 8-bit luma clip, one GPU:

    python tools/bench_motion_spec.py [--out FILE]          timing
    python tools/bench_motion_spec.py --accuracy [--out FILE]   the acceptance table of tests/test_motion_spec_gpu.py

Timing: ms per call and GB/s of the bytes each call has to move (input + output pixels) for abs and shift, both directions (abs has no
inverse type), on 8x8x8 blocks (one kernel, block_spec.hip) and on per-frame blocks (the plan's passes and motion_ops.hip's kernel over all
frames); beside them, in the same process, the composition a caller had to write before these calls existed, for shift -- 8-bit -> float,
dspfft_execute, the stand-alone store or load -- and the 8x8x8 roundtrip (Plan.roundtrip_u8) as the yardstick.  Under abs that composition
needs one host read per block for its c (motion.c:755); the count is reported instead of a time.  No filter on either side: the stand-alone
filter takes one block per call.  Device events around REPS calls after a warm-up; the cases alternate inside every round and the medians
over the rounds are reported with the spread (min .. max).

--accuracy: the share of bytes that differ from the float64 reference (tests/motion_spec_ref.py), off the quantiser's ties, and the float
pixels' max error over max|ref|, for the composition and for the fused calls over the cases of tests/test_motion_spec_gpu.py: worst case per
path, direction and mode.  The composition's column is what that file holds as COMPOSITION_SHARE / COMPOSITION_FLOAT."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS, REPS = 7, 3
CLIP = (64, 1080, 1920)


def timing(torch, lines):
    import motion_spec_ref as sr
    from dspfun_amd import _lib
    L = _lib.load()
    n = CLIP[0] * CLIP[1] * CLIP[2]
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(1, 256, CLIP, dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.empty_like(src)
    work = torch.empty(n, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    I3, I2 = C.c_int * 3, C.c_int * 2
    runs = {}
    for label, block in (("8x8x8", (8, 8, 8)), ("1920x1080x1", (1, 1080, 1920))):
        sf, nm, c = sr.constants(block)
        if block[0] == 1:
            fwd, inv = sr.stack_plan(block, CLIP[0], sr.ol.REDFT10), sr.stack_plan(block, CLIP[0], sr.ol.REDFT01)
        else:
            fwd, inv = sr.volume_plan(block, CLIP, sr.ol.REDFT10), sr.volume_plan(block, CLIP, sr.ol.REDFT01)
        w = work.data_ptr() if block[0] == 1 else 0
        for mode in ("abs", "shift"):
            runs[f"{label} spectrogram {mode} fused"] = (lambda fwd=fwd, mode=mode, sf=sf, nm=nm, c=c, w=w: fwd.spectrogram(src.data_ptr(), dst.data_ptr(), mode, sf, nm, c, d_work=w, stream=stream), fwd)
        runs[f"{label} ispectrogram shift fused"] = (lambda inv=inv, sf=sf, nm=nm, c=c, w=w: inv.ispectrogram(src.data_ptr(), dst.data_ptr(), "shift", sf, nm, c, d_work=w, stream=stream), inv)
        # the composition on the same plan: dspfft_u8_to_f32, dspfft_execute, dspfft_motion_store_u8 / dspfft_motion_load_u8, dspfft_execute, dspfft_f32_to_u8
        # (the pointwise ends see the clip as one region of CLIP[0] planes: shift's c is one constant)

        def comp_spec(fwd=fwd, sf=sf, nm=nm, c=c):
            assert L.dspfft_u8_to_f32(work.data_ptr(), src.data_ptr(), n, stream) == 0
            fwd.execute(work.data_ptr(), stream=stream)
            assert L.dspfft_motion_store_u8(dst.data_ptr(), work.data_ptr(), I3(*CLIP), I2(CLIP[1], CLIP[2]), 2, sf, nm, c, stream) == 0

        def comp_ispec(inv=inv, sf=sf, nm=nm, c=c):
            assert L.dspfft_motion_load_u8(work.data_ptr(), src.data_ptr(), I3(*CLIP), I2(CLIP[1], CLIP[2]), 2, c, nm, stream) == 0
            inv.execute(work.data_ptr(), stream=stream)
            assert L.dspfft_f32_to_u8(dst.data_ptr(), work.data_ptr(), sf * nm * nm, n, stream) == 0
        runs[f"{label} spectrogram shift composition"] = (comp_spec, fwd)
        runs[f"{label} ispectrogram shift composition"] = (comp_ispec, inv)
        if block[0] == 8:
            runs["8x8x8 roundtrip_u8 (yardstick)"] = (lambda fwd=fwd, inv=inv, sf=sf, nm=nm: fwd.roundtrip_u8(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), sf * nm * nm, stream=stream), fwd)
        nblocks = n // (block[0] * block[1] * block[2])
        lines.append(f"# {label}: abs through the composition needs {nblocks} host reads of a block's DC per clip (one synchronisation each); the fused call needs none")
    for run, _ in runs.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, (run, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                run()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / REPS)
    for k in runs:
        med = statistics.median(t[k])
        lines.append(f"{k:46s} {med:8.3f} ms ({min(t[k]):.3f} .. {max(t[k]):.3f})  {2 * n / med / 1e6:8.1f} GB/s of input + output pixels")
    for k in ("8x8x8 spectrogram shift", "8x8x8 ispectrogram shift", "1920x1080x1 spectrogram shift", "1920x1080x1 ispectrogram shift"):
        lines.append(f"# {k}: composition / fused = {statistics.median(t[k + ' composition']) / statistics.median(t[k + ' fused']):.2f}x")


def accuracy(torch, lines):
    import numpy as np
    import motion_grid_ref as gr
    import motion_spec_ref as sr
    T, PASSES = sr, sr.PASSES
    from dspfun_amd import _lib
    L = _lib.load()
    worst = {}

    def note(key, mode, who, fl, value):
        k = (key, mode if not fl else "f32", who)
        worst[k] = max(worst.get(k, 0.0), value)

    def both(key, inverse, block, vol_shape, mode, plan, with_work, skip_full=False):
        nbk = sr.nblocks_of(block, vol_shape)
        for kind, fl, ref, pix in T.cases_of(inverse, block, vol_shape, mode):
            if skip_full and kind:
                continue
            got, _ = T.fused(torch, plan, inverse, pix, block, mode, ref["filt"], with_work=with_work)
            comp = gr.from_blocks(T.composition(torch, L, inverse, gr.to_blocks(pix, block), block, mode, ref["filt"]), block, nbk)
            for who, out in (("fused", got), ("composition", comp)):
                if fl:
                    note(key, mode, who, True, T.float_err(out, ref["pel"], ref["tie"]))
                else:
                    mx, n, size = T.share_of(out, ref["out8"], ref["tie"])
                    assert mx <= 1 or who == "composition", (key, mode, kind, who, mx)
                    note(key, mode, who, False, n / size)
                    note(key, mode, who + " bytes", False, float(n))
    for inverse in (False, True):
        kind_of = sr.ol.REDFT01 if inverse else sr.ol.REDFT10
        d = "ispec" if inverse else "spec"
        for mode in (sr.ISPEC_MODES if inverse else sr.SPEC_MODES):
            for block, vol_shape in sr.SHAPES:
                both(("blocks", d), inverse, block, vol_shape, mode, sr.volume_plan(block, vol_shape, kind_of), False)
            for block, nb in PASSES:
                big = block[1] == 540
                both(("passes", d), inverse, block, (nb * block[0], block[1], block[2]), mode, sr.stack_plan(block, nb, kind_of), True, skip_full=big and mode in ("flat", "copy"))
    lines.append("# worst case over the cases of tests/test_motion_spec_gpu.py; 8-bit: share of bytes that differ from the float64 reference (most bytes in one case);")
    lines.append("# f32: max error / max|ref|.  cap = 1.5 x the composition's share + 4 bytes; f32: 2 x the composition's")
    for key in sorted({k[0] for k in worst}):
        for mode in ("abs", "shift", "flat", "copy", "f32"):
            if (key, mode, "fused") not in worst:
                continue
            f, c = worst[(key, mode, "fused")], worst[(key, mode, "composition")]
            if mode == "f32":
                lines.append(f"{key[0]:7s} {key[1]:6s} {mode:6s} fused {f:.3e}   composition {c:.3e}")
            else:
                lines.append(f"{key[0]:7s} {key[1]:6s} {mode:6s} fused {f:.6%} ({int(worst[(key, mode, 'fused bytes')])} bytes)   composition {c:.6%} ({int(worst[(key, mode, 'composition bytes')])} bytes)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_motion_spec: no GPU visible", file=sys.stderr)
        return 2
    lines = [f"# motion --spectrogram / --ispectrogram, 8-bit pixels, {CLIP[2]}x{CLIP[1]}x{CLIP[0]} luma, {torch.cuda.get_device_name(0)}"]
    if args.accuracy:
        accuracy(torch, lines)
    else:
        lines.append(f"# ms per call: median of {ROUNDS} rounds of {REPS} calls between device events (min .. max)")
        timing(torch, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
