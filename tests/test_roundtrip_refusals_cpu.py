"""Every refusal of the roundtrip entries (dspfft_execute_roundtrip and its _u8, _topn, _u8_topn, _limit, _u8_limit, _u8_dither,
_u8_dither_limit and _u8_packed twins), its code and the whole text of dspfft_last_error(), on the product library and on the CPU emulation
library.  Needs no device: every call is one the library refuses before it launches anything, made with fake non-null pointers on plans of
4-, 8-, 12-, 16-, 17- and 20-point axes, which need no device tables.  The emulation library has none of the HIP-only kernels and says so with
-3 -- after everything it can say about the call itself (-1, -2), which is part of the record: the rows at the end are calls only it refuses."""
import ctypes as C

from dspfun_amd import _lib
from dspfun_amd.engine import Plan, motion_grid_plans, motion_temporal_plans, _spec_params, REDFT01, REDFT10

A = 4096          # a non-null, 16-byte aligned address for calls that are refused before anything reads it
BIG = 1 << 20     # a coefficient limit at or above every block's count: no limit
FLOAT = ("rt", "topn", "limit")
U8 = ("u8", "u8_topn", "u8_limit")
DITHER = ("u8_dither", "u8_dither_limit")
LIMIT = ("limit", "u8_limit", "u8_dither_limit")
KEEP = ("topn", "u8_topn") + LIMIT
PLANAR = FLOAT + U8 + DITHER
PACKED = ("u8_packed",)
ALL = PLANAR + PACKED
SPEC = ("spec_u8", "spec_f32", "ispec_u8", "ispec_f32")          # the spectrogram halves share the filter's check
BAD_FILTERS = {"dc3": dict(preserve_dc=3), "minbuf0": dict(minbuf_hw=(0, 1)), "depth0": dict(block_depth=0)}


def plans(L):
    """name -> (fwd, inv): the smallest pairs that reach each check"""
    P = {}
    P["block"] = motion_grid_plans((16, 16, 16), (8, 8, 8), (8, 8, 8), lib=L)[:2]
    P["grid"] = motion_grid_plans((16, 16, 16), (8, 8, 8), (4, 4, 4), lib=L)[:2]
    P["block16"] = motion_grid_plans((32, 32, 32), (16, 16, 16), (16, 16, 16), lib=L)[:2]
    P["temporal"] = motion_temporal_plans((16, 2, 4), 8, 4, lib=L)[:2]

    def temporal(D, S, pitch):
        how = lambda n: [(2, n * pitch, n * pitch), (pitch, 1, 1)]
        return Plan.guru([(D, pitch, pitch)], how(D), [REDFT10], lib=L), Plan.guru([(S, pitch, pitch)], how(S), [REDFT01], lib=L)
    P["temporal pitch 6"] = temporal(8, 4, 6)
    P["temporal 17"] = temporal(17, 8, 8)

    def frames(n, kind, first_axis_first, howmany=4, dist=240, embed=None, stride=1):
        return Plan.many_r2r(n, [kind, kind], howmany=howmany, inembed=embed, istride=stride, idist=dist, onembed=embed, ostride=stride, odist=dist, lib=L,
                             first_axis_first=first_axis_first)
    f = frames([12, 20], REDFT10, False)
    P["frames"] = (f, frames([12, 20], REDFT01, True))
    # the same frames in planes of 12 x 512: a frame's run of 11 * 512 + 20 floats is more than the 4096 a wave selects from without a work buffer
    P["frames, pitch 512"] = tuple(frames([12, 20], k, o, embed=[12, 512], dist=12 * 512) for k, o in ((REDFT10, False), (REDFT01, True)))
    P["frames, pass order"] = (f, frames([12, 20], REDFT01, False))
    P["frames, batch layout"] = (f, frames([12, 20], REDFT01, True, dist=480))
    P["frames, howmany"] = (f, frames([12, 20], REDFT01, True, howmany=3))
    P["frames, rescaled"] = (f, frames([6, 10], REDFT01, True, embed=[12, 20]))
    P["one block, two embeddings"] = (Plan.many_r2r([8, 8], [REDFT10] * 2, inembed=[8, 8], onembed=[8, 16], lib=L),
                                      Plan.many_r2r([4, 4], [REDFT01] * 2, inembed=[8, 16], onembed=[8, 16], lib=L, first_axis_first=True))
    P["interleaved"] = (frames([12, 20], REDFT10, False, howmany=3, dist=1, stride=3), frames([12, 20], REDFT01, True, howmany=3, dist=1, stride=3))
    how4 = [(2, 1024, 1024), (2, 512, 512), (2, 128, 128), (2, 8, 8)]
    P["four batch axes"] = tuple(Plan.guru([(8, 16, 16), (8, 1, 1)], how4, [k, k], lib=L) for k in (REDFT10, REDFT01))
    f64 = Plan.many_r2r([8, 8, 8], [REDFT10] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
    P["f64"] = (f64, f64)
    return P


def filter_params(name):
    fp = _lib.MotionFilterParams()
    fp.active = (C.c_int * 3)(4, 4, 4); fp.minbuf_hw = (C.c_int * 2)(8, 8); fp.block_depth = 8
    fp.band_begin = (C.c_int * 3)(0, 0, 0); fp.band_end = (C.c_int * 3)(4, 4, 4)
    fp.damp = fp.boost = 1.0
    for k, v in BAD_FILTERS[name].items():
        setattr(fp, k, (C.c_int * 2)(*v) if isinstance(v, tuple) else v)
    return fp


def call(L, P, entry, pair, fwd="", inv="", d_in=A, d_out=A, d_work=A, fp=None, keep=BIG, cl="", packed=3, sf=1.0, norm=1.0):
    """One call of `entry` on the plans of `pair` with fake buffers -> (code, dspfft_last_error).  fwd / inv: None, or the pair to take that
    plan from; fp: a BAD_FILTERS name; cl: None, or (keep, outside_mul) (default: (keep, 1), the packed entry: None); packed: components or None."""
    h = lambda side, k: None if side is None else P[side or pair][k]._h
    v = C.c_void_p
    fpo = filter_params(fp) if fp else None
    fpp = C.byref(fpo) if fpo is not None else None
    if cl == "":
        cl = None if entry == "u8_packed" else (keep, 1.0)
    clo = None
    if cl is not None:
        clo = _lib.CoeffLimit()
        clo.keep, clo.outside_mul, clo.d_work, clo.work_bytes = cl[0], cl[1], None, 0
    clp = C.byref(clo) if clo is not None else None
    head = (h(fwd, 0), h(inv, 1), v(d_in), v(d_out))
    tail = (None, None)          # d_coeffs_coded, stream
    if entry in SPEC:
        sp = _spec_params("shift", 1.0, 1.0, 0.0)
        inverse = entry.startswith("i")
        args = (h(fwd, 1 if inverse else 0), v(d_in), v(d_out), v(d_work), C.byref(sp), fpp) + ((1.0,) if inverse else ()) + tail
        fn = getattr(L, "dspfft_execute_" + entry.replace("spec", "spectrogram"))
    else:
        fn = getattr(L, "dspfft_execute_roundtrip" + ("" if entry == "rt" else "_" + entry))
        if entry == "u8_packed":
            pk = None
            if packed is not None:
                pk = _lib.MotionPacked()
                pk.components = packed
            mid = (1.0, fpp, C.byref(pk) if pk is not None else None, clp)
        else:
            mid = ((v(d_work),) if entry.startswith("u8") else ()) + ((sf, norm) if entry in DITHER else (1.0,) if entry in U8 else ())
            mid += (fpp,) + ((keep, None, 0) if entry.endswith("topn") else (clp,) if entry in LIMIT else ())
        args = head + mid + tail
    rc = fn(*args)
    return rc, L.dspfft_last_error().decode() if rc else ""


# ---- the record: what the library answers, and what the emulation library answers where that is something else ----
NULL = "null plan or buffer"
FILTER = "bad filter parameters"
PK = "roundtrip on packed 8-bit pixels"
GRID = "roundtrip with different forward / inverse extents over a grid of blocks"
TIME = "roundtrip over blocks along time (motion -b 1x1xD)"
ALIGN = ": float buffers must be 16-byte aligned, 8-bit buffers 4-byte aligned"
ORDER = "the forward plan's last pass and the inverse plan's first pass must run along the same axis (create the inverse with dspfft_plan_many_r2r_ordered(..., 1))"
NO_GRID_PAIR = GRID + ": every extent of both plans must be 4, 8 or 16 (2-D blocks: 32 too), x contiguous, all strides multiples of 4 (a single block goes with howmany = 1)"
EMBEDDING = "roundtrip with different forward / inverse extents needs ONE embedding for input, work and output (motion.c:535-552)"
OUTSIDE_MUL = "coefficient limit: outside_mul must be finite and > 0 (1 for motion's 3-D blocks)"
SF = "dither: scalefactor and normalization must be > 0"
COMPONENTS = PK + ": components must be 2, 3 or 4 bytes per pixel, got %d (one component is the planar call)"
PK_GRID = PK + ": different forward / inverse extents (a rescaled block grid, motion -s) are not implemented on packed pixels"
PK_PAIR = PK + (" needs the plan pair of the fused block pass: matching REDFT10 / REDFT01 small-block plans (every extent 4, 8 or 16, 2-D blocks up to 32; "
                "per-frame and single-block plans have no block pass)")
PK_KEEP = PK + ": coefficient limit: keep must be at least 1 (pass NULL for no limit)"
PK_ALIGN = PK + ": the buffers must be 4-byte aligned"
NO_DITHER = (-3, "dithered 8-bit store: not in this build (the dither kernel is HIP-only, motion_dither.hip)")
NO_GRID = (-3, GRID + ": not built into this library (the kernel is HIP-only, block_rescale.hip)")
NO_TIME = (-3, TIME + ": not built into this library (the kernel is HIP-only, temporal_rt.hip)")
NO_TOPN = (-3, "roundtrip with a coefficient limit: not built into this library (the selection kernels are HIP-only, block_topn.hip and motion_ops.hip)")
NO_PACKED = (-3, PK + ": not built into this library (the kernel is HIP-only, block_packed.hip)")

ROWS = []          # (what, pair, entries, call's keywords, (code, text), the emulation library's (code, text))


def row(what, pair, entries, rc, text, emul=None, **kw):
    ROWS.append((what, pair, entries, kw, (rc, text), emul or (rc, text)))


def emul_only(what, pair, entries, emul, **kw):
    ROWS.append((what, pair, entries, kw, None, emul))


# null plan, each null buffer, f64: every entry
for kw in (dict(fwd=None), dict(inv=None), dict(d_in=None), dict(d_out=None)):
    row("null", "block", PLANAR, -1, NULL, **kw)
    row("null", "block", PACKED, -1, PK + ": " + NULL, **kw)
row("null", "block", U8 + DITHER, -1, NULL, d_work=None)
for kw in (dict(fwd="f64"), dict(inv="f64")):
    row("f64", "block", FLOAT + U8, -1, "the fused roundtrip takes f32 plans", **kw)
    row("f64", "block", DITHER, -1, "the dithered roundtrip takes f32 plans", **kw)
    row("f64", "block", PACKED, -1, PK + " takes f32 plans", **kw)
# bad filter parameters: on a block pair, a grid pair, a temporal pair, a spectrogram call and the packed call
for bad in BAD_FILTERS:
    row("filter", "block", FLOAT + U8, -1, FILTER, fp=bad)
    row("filter", "block", DITHER, -1, FILTER, emul=NO_DITHER, fp=bad)
    row("filter", "grid", FLOAT + U8, -1, FILTER, emul=NO_GRID, fp=bad)
    row("filter", "grid", DITHER, -1, FILTER, emul=NO_DITHER, fp=bad)
    row("filter", "temporal", PLANAR, -1, FILTER, fp=bad)
    row("filter", "block", PACKED, -1, PK + ": " + FILTER, fp=bad)
    row("filter", "block", SPEC, -1, FILTER, fp=bad)
# the dspfft_coeff_limit of the _limit entries, ahead of everything else about the call
row("limit", "block", LIMIT, -1, "coefficient limit: null dspfft_coeff_limit (the entries without one take none)", cl=None)
row("limit", "block", LIMIT, -1, "coefficient limit: null dspfft_coeff_limit (the entries without one take none)", cl=None, d_in=None)
row("limit", "block", LIMIT, -1, "coefficient limit: keep must be at least 1 (the entries without a dspfft_coeff_limit take none)", cl=(0, 1.0))
for mul in (0.0, -1.0, float("nan"), float("inf")):
    row("limit", "block", LIMIT, -1, OUTSIDE_MUL, cl=(7, mul))
# a grid pair: buffers off by 2 bytes and, float buffers, by 4; a limit through an entry without a dspfft_coeff_limit
for off in (2, 4):
    row("alignment", "grid", FLOAT, -2, GRID + ALIGN, emul=NO_GRID, d_in=A + off)
    row("alignment", "grid", FLOAT, -2, GRID + ALIGN, emul=NO_GRID, d_out=A + off)
    row("alignment", "grid", DITHER, -2, GRID + ALIGN, emul=NO_DITHER, d_work=A + off)
row("alignment", "grid", U8, -2, GRID + ALIGN, emul=NO_GRID, d_in=A + 2)
row("alignment", "grid", DITHER, -2, GRID + ALIGN, emul=NO_DITHER, d_in=A + 2)
row("alignment", "grid", U8, -2, GRID + ALIGN, emul=NO_GRID, d_out=A + 2)
row("limit through a _topn entry", "grid", ("topn", "u8_topn"), -2,
    GRID + ": a coefficient limit is not implemented here (the reference selects over the whole embedding, motion.c:652-668)", emul=NO_GRID, keep=7)
row("limit and alignment", "grid", ("limit", "u8_limit"), -2, GRID + ALIGN, emul=NO_GRID, keep=7, d_in=A + 2)
row("limit and alignment", "grid", ("u8_dither_limit",), -2, GRID + ALIGN, emul=NO_DITHER, keep=7, d_in=A + 2)
# a temporal pair (the dither entries send it on as the plain 8-bit call)
row("limit below max(D, D')", "temporal", KEEP, -2, TIME + ": a coefficient limit is not implemented here", keep=7)
row("frame pitch", "temporal pitch 6", PLANAR, -2, TIME + ": the samples per frame (the frame pitch), 6, must be a multiple of 4")
row("length", "temporal 17", PLANAR, -2, TIME + ": lengths 17 and 8 must have no prime factor above 13 (the fused kernel has no Bluestein pass)")
row("alignment", "temporal", PLANAR, -2, TIME + ALIGN, d_in=A + 2)
row("alignment", "temporal", FLOAT, -2, TIME + ALIGN, d_in=A + 4)
row("alignment", "temporal", FLOAT + U8, -2, TIME + ALIGN, d_out=A + 2)
# pairs that are none
for pair, rc, text in (("frames, pass order", -1, ORDER), ("frames, batch layout", -1, "roundtrip: batch layouts differ"), ("frames, howmany", -1, ORDER),
                       ("frames, rescaled", -2, NO_GRID_PAIR), ("one block, two embeddings", -2, EMBEDDING)):
    row("mismatch", pair, FLOAT + U8, rc, text)
    row("mismatch", pair, DITHER, rc, text, emul=NO_DITHER)
# top-N
TOO_SMALL = "roundtrip with a coefficient limit: work buffer too small (dspfft_roundtrip_topn_work_bytes)"
row("work buffer too small", "frames, pitch 512", ("topn", "u8_topn", "limit", "u8_limit"), -1, TOO_SMALL, emul=NO_TOPN, keep=7)
row("work buffer too small", "frames, pitch 512", ("u8_dither_limit",), -1, TOO_SMALL, emul=NO_DITHER, keep=7)
# dither
for kw in (dict(sf=0.0), dict(sf=-1.0), dict(sf=float("nan")), dict(norm=0.0)):
    row("dither", "block", DITHER, -1, SF, emul=NO_DITHER, **kw)
    row("dither", "temporal", DITHER, -1, SF, **kw)
row("dither", "interleaved", DITHER, -2, "dithered store: the contiguous axis must be the plan's last (planar layout)", emul=NO_DITHER)
row("dither", "four batch axes", DITHER, -2, "dithered store: more than three batch axes", emul=NO_DITHER)
row("dither", "block", DITHER, -1, "the dithered roundtrip takes f32 plans", sf=0.0, fwd="f64")
# packed pixels: each refusal, and pairs of faults that show the order of the refusals
row("packed", "block", PACKED, -1, PK + ": null dspfft_motion_packed", packed=None)
row("packed", "block", PACKED, -1, PK + ": null dspfft_motion_packed", packed=None, fwd="f64")
row("packed", "block", PACKED, -1, PK_KEEP, cl=(0, 1.0))
row("packed", "block", PACKED, -1, PK + " takes f32 plans", fwd="f64", cl=(0, 1.0))
row("packed", "block", PACKED, -1, PK_KEEP, cl=(0, 1.0), fp="dc3")
row("packed", "block", PACKED, -2, COMPONENTS % 1, packed=1)
row("packed", "block", PACKED, -2, COMPONENTS % 5, packed=5)
row("packed", "block", PACKED, -1, PK + ": " + FILTER, fp="dc3", packed=5)
row("packed", "grid", PACKED, -2, PK_GRID)
row("packed", "grid", PACKED, -2, COMPONENTS % 5, packed=5)
row("packed", "grid", PACKED, -2, PK_GRID, d_in=A + 2)
row("packed", "frames", PACKED, -2, PK_PAIR)
row("packed", "temporal", PACKED, -2, PK_PAIR)
row("packed", "frames", PACKED, -2, PK_PAIR, d_in=A + 2)
row("packed", "block", PACKED, -2, PK_ALIGN, d_in=A + 2)
row("packed", "block", PACKED, -2, PK_ALIGN, d_out=A + 2)
row("packed", "block16", PACKED, -2,
    PK + ": the 4 component tiles of a 16x16x16 block (65536 bytes) and the tables do not fit a workgroup's 64 KB of LDS", packed=4)
row("packed", "block16", PACKED, -2, PK_ALIGN, packed=4, d_out=A + 2)
# calls with nothing wrong, which the product library would launch: the emulation library's -3 comes last
emul_only("a good call", "block", PACKED, NO_PACKED)
emul_only("a good call", "block", PACKED, NO_PACKED, packed=4)
emul_only("a good call", "block", DITHER, NO_DITHER)
emul_only("a good call", "grid", FLOAT + U8, NO_GRID)
emul_only("a good call", "grid", DITHER, NO_DITHER)
emul_only("a good call", "temporal", PLANAR, NO_TIME)
emul_only("a good call with a limit", "block", ("topn", "u8_topn", "limit", "u8_limit"), NO_TOPN, keep=7)
emul_only("a good call with a limit", "block", ("u8_dither_limit",), NO_DITHER, keep=7)


def check(L, which):
    P = plans(L)
    wrong, calls = [], 0
    for what, pair, entries, kw, *want in ROWS:
        if want[which] is None:
            continue
        for entry in entries:
            calls += 1
            got = call(L, P, entry, pair, **kw)
            assert got[0] in (-1, -2, -3), (what, pair, entry, kw, got)          # (anything else came from a launch: a bug in the table)
            if got != want[which]:
                wrong.append((what, pair, entry, kw, got, want[which]))
    assert not wrong, "\n".join(map(repr, wrong))
    return calls


def test_every_entry_is_in_the_table():
    seen = {e for row_ in ROWS for e in row_[2]}
    assert seen == set(ALL + SPEC)
    for e in ALL:          # null plan, null buffers, f64 and bad filter parameters reach every roundtrip entry
        for key in ("fwd", "inv", "d_in", "d_out", "fp"):
            assert any(e in r[2] and key in r[3] for r in ROWS), (e, key)


def test_refusals_of_the_product_library():
    assert check(_lib.load(), 0) > 300


def test_refusals_of_the_emulation_library():
    from emul_lib import emul
    assert check(emul(), 1) > 300
