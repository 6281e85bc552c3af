"""Shared table of NON-DENSE plan geometries at kernel-selecting lengths -- TEST INFRASTRUCTURE ONLY.

tests/test_geometry_cpu.py runs the table through the CPU emulation of the kernel phases, tests/test_geometry_gpu.py through the HIP
library.  A case is one plan (guru or many_r2r arguments, sample type, kinds, planner switches), the kernel family `Plan.describe()` must
name for it, optional fused scales and whether it runs in place.  Everything is deterministic: fixed seeds, `oracle_lib.synth_f32` inputs.

The reference of a case never relies on the port's own stride handling: the input is gathered into a dense [batch..., axes...] float64
array by numpy index arithmetic, transformed by `oracle_lib.r2r_many(impl="port")` and scattered to the output positions.  (The port's
stride handling with differing input and output layouts is pinned against the direct definition in test_geometry_cpu.py.)
"""
import os
import re

import numpy as np
from numpy.lib.stride_tricks import as_strided

import oracle_lib as ol

REDFT01, REDFT10 = ol.REDFT01, ol.REDFT10
K10, K01 = REDFT10, REDFT01

SCALE, IN0, OUT0 = 0.37, 0.5, 0.7       # set_scale / set_axis_scale0 values of the scaled cases (the f64 channel-line test's)
PAD = 48                                # elements behind the last owned one: a store beyond the plan's span lands in them
SPEC_LIST = os.path.join(ol.ROOT, "dspfun_amd", "csrc", "spec_list.h")

# tolerances of the dense tests of the same families, relative to max|ref| and rms(ref) (test_gpu_parity.py: check / TOL from
# BASELINE.json north_star; test_f64_specialised_sizes; test_bluestein_sizes_vs_oracle)
TOL_F32, TOL_F64, TOL_F64_BLUE = 1e-5, 1e-13, 2e-13


class Case:
    """dims / how: (n, in_stride, out_stride) in elements, `how` in the (shuffled) order handed to the planner.  `many`: the same plan as
    Plan.many_r2r keyword arguments (the plan is then created through that entry point).  expect: regular expressions that must all match
    describe(); reject: ones that must not.  emul: "run" (the emulation reaches the same family), "generic" (the family needs the device:
    plan-time compiled kernels -- the emulation runs the case on `emul_expect` instead) or "describe" (too big for the emulation: planned
    and described only)."""

    def __init__(self, name, family, dims, how, kinds, expect, reject=(), dtype="f32", env=None, scaled_axis=None, inplace=False,
                 emul="run", emul_expect=None, many=None, seed=0):
        self.name, self.family = name, family
        self.dims = [tuple(int(v) for v in d) for d in dims]
        self.how = [tuple(int(v) for v in d) for d in how]
        self.kinds = list(kinds)
        self.expect, self.reject = list(expect), list(reject)
        self.dtype, self.env = dtype, dict(env or {})
        self.scaled_axis, self.inplace = scaled_axis, inplace
        self.emul, self.emul_expect = emul, list(emul_expect or [])
        self.many, self.seed = many, seed
        if inplace:
            assert all(d[1] == d[2] for d in self.dims + self.how), name     # in place with differing layouts is undefined: never built

    def __repr__(self):
        return self.name

    # ---- geometry ----
    @property
    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32

    @property
    def shape(self):
        return tuple(d[0] for d in self.how) + tuple(d[0] for d in self.dims)

    @property
    def samples(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def size(self, side):
        """elements of the input (side 1) or output (side 2) buffer: the plan's span and PAD sentinels behind it"""
        return 1 + sum((d[0] - 1) * d[side] for d in self.how + self.dims) + PAD

    def view(self, buf, side):
        it = buf.dtype.itemsize
        return as_strided(buf, shape=self.shape, strides=tuple(d[side] * it for d in self.how + self.dims))

    def owned(self, side):
        m = np.zeros(self.size(side), dtype=bool)
        self.view(m, side)[...] = True
        return m

    # ---- data ----
    def make_input(self):
        n = self.size(1)
        x = ol.synth_f32(0x6E0 + self.seed, n)
        if self.dtype == "f64":
            return x.astype(np.float64) * (1 + 2.0 ** -30) + 1e-9 * (np.arange(n) % 977)
        return x

    def make_output(self):
        """the out-of-place output buffer before the run: a position-dependent sentinel pattern"""
        n = self.size(2)
        return (-4096.0 - (np.arange(n) % 509)).astype(self.np_dtype)

    def reference(self, x):
        """dense float64 [batch..., axes...] result for the input buffer x"""
        nb, rank = len(self.how), len(self.dims)
        dense = np.array(self.view(x, 1), dtype=np.float64)     # a copy, also of a dense f64 input: the input scale below must not reach x
        n = [d[0] for d in self.dims]
        if self.scaled_axis is not None:
            sl = [slice(None)] * dense.ndim
            sl[nb + self.scaled_axis] = 0
            dense[tuple(sl)] *= IN0
        lines = int(np.prod(n))
        ref = ol.r2r_many(dense.ravel(), n, self.kinds, howmany=dense.size // lines, idist=lines, odist=lines, impl="port", threads=8)
        ref = ref.reshape(dense.shape)
        if self.scaled_axis is not None:
            ref *= SCALE
            ref[tuple(sl)] *= OUT0
        assert rank == len(self.kinds)
        return ref

    @property
    def tol(self):
        if self.dtype == "f32":
            return TOL_F32
        return TOL_F64_BLUE if "BLUE" in self.family else TOL_F64

    # ---- the plan ----
    def plan(self, lib=None):
        from dspfun_amd.engine import Plan
        if self.many is not None:
            p = Plan.many_r2r(kinds=self.kinds, lib=lib, dtype=self.dtype, **self.many)
        else:
            p = Plan.guru(self.dims, self.how, self.kinds, lib=lib, dtype=self.dtype)
        if self.scaled_axis is not None:
            p.set_scale(SCALE).set_axis_scale0(self.scaled_axis, IN0, OUT0)
        return p

    def check_describe(self, text, emulation=False):
        expect = self.emul_expect if (emulation and self.emul == "generic") else self.expect
        for pat in expect:
            assert re.search(pat, text), (self.name, pat, text)
        for pat in self.reject:
            assert not re.search(pat, text), (self.name, pat, text)


def errors(got, ref):
    """(max, rms) error relative to max|ref| and rms(ref): `check` of test_gpu_parity.py"""
    got = np.asarray(got, dtype=np.float64)
    m = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    r = np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30)
    return float(m), float(r)


def verify(case, x_before, x_after, out_before, out_after):
    """the assertions both runners share.  In place: pass the one buffer as x_* and out_* = None.  Returns (max, rms) error."""
    ref = case.reference(x_before)
    if case.inplace:
        before, after = x_before, x_after
    else:
        assert np.array_equal(x_after.view(np.uint8), x_before.view(np.uint8)), f"{case.name}: out-of-place input changed"
        before, after = out_before, out_after
    own = case.owned(2)
    assert int(own.sum()) == case.samples, f"{case.name}: output positions overlap"
    stray = np.flatnonzero((after.view(np.uint32 if case.dtype == "f32" else np.uint64) != before.view(np.uint32 if case.dtype == "f32" else np.uint64)) & ~own)
    assert stray.size == 0, f"{case.name}: {stray.size} positions outside the plan's index set changed, first at {stray[:8]}"
    got = np.ascontiguousarray(case.view(after, 2))
    m, r = errors(got, ref)
    print(f"GEOMETRY {case.name} family={case.family!r} dtype={case.dtype} max={m:.3e} rms={r:.3e} tol={case.tol:g}")
    assert m <= case.tol and r <= case.tol, (case.name, m, r, case.tol)
    return m, r


# ---------------------------------------------------------------- layouts ----------------------------------------------------------------
def nest(unit, counts, gaps, align=1):
    """strides of nested batch dimensions, innermost first: dimension i steps over the whole extent of what lies inside it plus gaps[i]
    elements, rounded up to `align`.  Returns (strides, extent)."""
    out, ext = [], unit
    for n, g in zip(counts, gaps):
        st = -(-(ext + g) // align) * align
        out.append(st)
        ext = (n - 1) * st + ext
    return out, ext


def shuffled(how, seed):
    how = list(how)
    order = np.random.default_rng(seed).permutation(len(how))
    return [how[i] for i in order]


# line-count / batch-structure / layout-direction variants: (tag, counts innermost first, input gaps, output gaps or None = same, in place)
def variants(ragged):
    return [
        ("one", [], [], None, False),                                  # a single line / plane, out of place, same layout
        ("two-gap", [2], [12], None, True),                            # one batch dimension with a gap, in place
        ("prime-nb01", [7, 2], [4, 20], [8, 36], False),               # nb0 and nb1 with different gaps; other pitch and dist on the output
        ("ragged-host", ragged, [4, 8, 16, 44], None, True),           # four batch dimensions: more than a launch takes (hostloop)
        ("ragged-host-oop", ragged, [4, 8, 16, 44], [8, 4, 28, 12], False),
    ]


def row_cases(family, N, C, dtype, expect, ragged=(5, 3, 2, 2), env=None, line_pad=0, emul="run", emul_expect=None, tags=None, reject=()):
    """lines of N pixels of C interleaved samples, row pitch > N*C"""
    out = []
    for i, (tag, counts, gin, gout, inplace) in enumerate(variants(list(ragged))):
        if tags is not None and tag not in tags:
            continue
        unit = N * C + line_pad
        si, _ = nest(unit, counts, gin)
        so, _ = nest(unit, counts, gout if gout is not None else gin)
        how = [(n, a, b) for n, a, b in zip(counts, si, so)]
        if C > 1:
            how.append((C, 1, 1))
        kind = (K10, K01)[i % 2]
        name = f"{family} {dtype} N={N} C={C} {tag}"
        scaled = 0 if tag == "prime-nb01" else None
        out.append(Case(name, family, [(N, C, C)], shuffled(how, i + N), [kind], expect + (["hostloop"] if "host" in tag and "TINY" not in family else []),
                        reject=reject, dtype=dtype, env=env, scaled_axis=scaled, inplace=inplace, emul=emul, emul_expect=emul_expect, seed=i + N))
    return out


def col_cases(family, N, inner, pitch, dtype, expect, ragged=(3, 2, 2, 2), env=None, align=4, opitch=None, emul="run", emul_expect=None, tags=None,
              reject=()):
    """planes of N rows of `inner` contiguous samples, row pitch `pitch` >= inner; the transform runs down the rows.  opitch: the row pitch of
    the out-of-place outputs with their own layout (default pitch + align)"""
    out = []
    for i, (tag, counts, gin, gout, inplace) in enumerate(variants(list(ragged))):
        if tags is not None and tag not in tags:
            continue
        po = pitch if gout is None else (opitch or pitch + align)
        si, _ = nest((N - 1) * pitch + inner, counts, gin, align)
        so, _ = nest((N - 1) * po + inner, counts, gout if gout is not None else gin, align)
        how = [(n, a, b) for n, a, b in zip(counts, si, so)]
        if inner > 1:
            how.append((inner, 1, 1))
        kind = (K01, K10)[i % 2]
        name = f"{family} {dtype} N={N} inner={inner} pitch={pitch} {tag}"
        scaled = 0 if tag == "prime-nb01" else None
        out.append(Case(name, family, [(N, pitch, po)], shuffled(how, i + N), [kind], expect + (["hostloop"] if "host" in tag and "TINY" not in family else []),
                        reject=reject, dtype=dtype, env=env, scaled_axis=scaled, inplace=inplace, emul=emul, emul_expect=emul_expect, seed=i + N + inner))
    return out


def transposing_cases(family, N, dtype, expect, env=None, lines=7, C=3):
    """out of place between layouts that differ in more than a pitch: rows in -> columns out, the reverse, interleaved in -> planar out"""
    pin = N + 4
    return [
        Case(f"{family} {dtype} N={N} rows->columns", family, [(N, 1, lines + 2)], [(lines, pin, 1)], [K10], expect, dtype=dtype, env=env, seed=N + 1),
        Case(f"{family} {dtype} N={N} columns->rows", family, [(N, lines + 1, 1)], [(lines, 1, pin)], [K01], expect, dtype=dtype, env=env, seed=N + 2,
             scaled_axis=0),
        Case(f"{family} {dtype} N={N} interleaved->planar", family, [(N, C, 1)], shuffled([(C, 1, N + 8), (lines, N * C + 6, C * (N + 8) + 5)], N), [K10], expect,
             dtype=dtype, env=env, seed=N + 3),
        Case(f"{family} {dtype} N={N} planar->interleaved", family, [(N, 1, C)], shuffled([(C, N + 8, 1), (lines, C * (N + 8) + 5, N * C + 6)], N), [K01], expect,
             dtype=dtype, env=env, seed=N + 4),
    ]


# ------------------------------------------------------------- spec_list.h entries -------------------------------------------------------------
ENTRY_MACROS = ("DSPFFT_ROW_SPECS", "DSPFFT_COL_SPECS_A", "DSPFFT_COL_SPECS_B", "DSPFFT_ROW_SPECS_F64", "DSPFFT_ROW_CHAN_SPECS_F64", "DSPFFT_COL_SPECS_F64")


def parse_spec_list(path=SPEC_LIST):
    """{macro: [(N, P, threads), ...]} for the X(...) lines of ENTRY_MACROS, in the order of the file (the order the registries number them)"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for macro in ENTRY_MACROS:
        m = re.search(r"#define\s+" + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text)
        assert m, macro
        out[macro] = [tuple(int(v) for v in e.split(",")[:3]) for e in re.findall(r"X\(([^)]*)\)", m.group(1))]
        assert out[macro], macro
    return out


def entry_cases():
    """one rank-1 non-dense case per listed entry, which must select exactly that entry.  Returns (cases, unreachable): an entry the generator
    has no geometry for is named in `unreachable` (a test failure, not a skip)."""
    specs = parse_spec_list()
    cases, unreachable = [], []

    def row_entry(macro, table, i, dtype):
        N, C, _ = table[i]
        first = [j for j, e in enumerate(table) if e[:2] == (N, C)][0]
        if first != i:                      # a second entry of the same (N, C) is taken only through DSPFFT_ROW_PREF: no generator for it
            unreachable.append(f"{macro} X({N}, {C}, ...) #{i}")
            return
        tagf = " f64" if dtype == "f64" else ""
        env, expect, reject = {}, [rf"ROW\*{tagf} N={N} C={C} spec#{i} threads="], ["channel lines"]
        chan = [e for e in specs["DSPFFT_ROW_CHAN_SPECS_F64"] if e[:2] == (N, C)] if dtype == "f64" else []
        if chan and C * (N // 2 + 16) * 16 > 160 * 1024:          # no whole-line kernel: reached through its channel-line form
            expect, reject = [rf"ROW\* f64 N={N} C={C} spec#{i} as {C} channel lines"], []
        elif chan:
            env = {"DSPFFT_ROW_CHAN": "0"}                      # the whole-line kernel behind the channel lines
        c = row_cases(f"entry {macro}", N, C, dtype, expect, env=env, tags=["prime-nb01"], ragged=(3,), reject=reject)[0]
        c.name = f"entry {macro} X({N}, {C}) spec#{i}"
        cases.append(c)

    def chan_entry(i):
        N, G, _ = specs["DSPFFT_ROW_CHAN_SPECS_F64"][i]
        rows = [j for j, e in enumerate(specs["DSPFFT_ROW_SPECS_F64"]) if e[:2] == (N, G)]
        if not rows:
            unreachable.append(f"DSPFFT_ROW_CHAN_SPECS_F64 X({N}, {G}, ...): no row entry to hang on")
            return
        c = row_cases("entry DSPFFT_ROW_CHAN_SPECS_F64", N, G, "f64", [rf"ROW\* f64 N={N} C={G} spec#{rows[0]} as {G} channel lines"], tags=["prime-nb01"])[0]
        c.name = f"entry DSPFFT_ROW_CHAN_SPECS_F64 X({N}, {G}) chan#{i}"
        cases.append(c)

    def col_entry(macro, table, i, base, dtype):
        N, K, T = table[i]
        earlier = [e for e in table[:i] if e[0] == N]
        inner = next((K * m for m in (3, 1, 5, 7) if not any((K * m) % e[1] == 0 for e in earlier)), None)
        env = {}
        if inner is None and dtype == "f32" and not any(e[1] == K for e in earlier):
            inner, env = K * 3, {"DSPFFT_COL_KPREF": str(K)}     # shadowed by a narrower earlier entry: asked for by width
        if inner is None:
            unreachable.append(f"{macro} X({N}, {K}, {T}, ...) #{base + i}")
            return
        tagf = " f64" if dtype == "f64" else ""
        pitch = inner + 8
        c = col_cases(f"entry {macro}", N, inner, pitch, dtype, [rf"COL\*{tagf} N={N} K={K} spec#{base + i} threads={T} inner={inner} "], env=env,
                      tags=["prime-nb01"], ragged=(3,))[0]
        c.name = f"entry {macro} X({N}, {K}) spec#{base + i}"
        cases.append(c)

    for i in range(len(specs["DSPFFT_ROW_SPECS"])):
        row_entry("DSPFFT_ROW_SPECS", specs["DSPFFT_ROW_SPECS"], i, "f32")
    col = specs["DSPFFT_COL_SPECS_A"] + specs["DSPFFT_COL_SPECS_B"]           # one registry: DSPFFT_COL_SPECS = A then B
    na = len(specs["DSPFFT_COL_SPECS_A"])
    for i in range(len(col)):
        col_entry("DSPFFT_COL_SPECS_A" if i < na else "DSPFFT_COL_SPECS_B", col, i, 0, "f32")
    for i in range(len(specs["DSPFFT_ROW_SPECS_F64"])):
        row_entry("DSPFFT_ROW_SPECS_F64", specs["DSPFFT_ROW_SPECS_F64"], i, "f64")
    for i in range(len(specs["DSPFFT_ROW_CHAN_SPECS_F64"])):
        chan_entry(i)
    for i in range(len(specs["DSPFFT_COL_SPECS_F64"])):
        col_entry("DSPFFT_COL_SPECS_F64", specs["DSPFFT_COL_SPECS_F64"], i, 0, "f64")
    return cases, unreachable


def entry_count():
    return sum(len(v) for v in parse_spec_list().values())


# ------------------------------------------------------------------ the table ------------------------------------------------------------------
def family_cases():
    c = []
    no_blue = {"DSPFFT_NO_BLUESTEIN": "1"}
    for dt, tagf in (("f32", ""), ("f64", " f64")):
        # TINY: packed (contiguous lines back to back, several LDS chunks and a ragged tail) and not packed
        c.append(Case(f"TINY packed {dt} N=16 x 257 lines, 3 runs with a gap", "TINY packed", [(16, 1, 1)], [(3, 16 * 257 + 7, 16 * 257 + 7), (257, 16, 16)], [K10],
                      [rf"TINY{tagf} N=16 .* packed"], dtype=dt, inplace=True, seed=1))
        c.append(Case(f"TINY packed {dt} N=8 x 600 lines to other run pitch", "TINY packed", [(8, 1, 1)], [(600, 8, 8), (2, 8 * 600 + 3, 8 * 600 + 10)], [K01],
                      [rf"TINY{tagf} N=8 .* packed"], dtype=dt, scaled_axis=0, seed=2))
        c += row_cases("TINY", 32, 1, dt, [rf"TINY{tagf} N=32 "], line_pad=5, reject=["packed"])
        c += col_cases("TINY", 12, 21, 23, dt, [rf"TINY{tagf} N=12 "], align=1, reject=["packed"], tags=["two-gap", "prime-nb01", "ragged-host-oop"])
        c += transposing_cases("TINY", 17, dt, [rf"TINY{tagf} N=17 "])
        # generic ROW with several lines per workgroup: forced (ragged last group: 7, 14 and 30 lines in groups of 4) and the planner's own choice
        lpw = {"DSPFFT_ROW_LPW": "4"}
        c += row_cases("ROW generic LPW>1", 64, 3, dt, [rf"ROW{tagf}  N=64 C=3 .* x4 "], env=lpw, line_pad=6)
        c += row_cases("ROW generic LPW>1", 96, 1, dt, [rf"ROW{tagf}  N=96 C=1 .* x4 "], env=lpw, line_pad=1, tags=["one", "prime-nb01", "ragged-host"])
        c.append(Case(f"ROW generic LPW>1 {dt} N=64 C=1 4099 lines (planner's x4)", "ROW generic LPW>1", [(64, 1, 1)], [(4099, 68, 72)], [K01],
                      [rf"ROW{tagf}  N=64 C=1 .* lines=4099 x4 "], dtype=dt, seed=3))
        # COL with a tail tile: an inner run that is no multiple of any listed K, and a pitch that breaks the 4-sample rule
        c += col_cases("COL generic tail tile", 2160, 21, 24, dt, [rf"COL{tagf}  N=2160 K=\d+ inner=21 tiles=[2-9]"], reject=[r"COL\*"])
        c += col_cases("COL generic misaligned pitch", 1080, 48, 50, dt, [rf"COL{tagf}  N=1080 K=\d+ inner=48 "], align=1, opitch=53, reject=[r"COL\*"],
                       tags=["one", "two-gap", "prime-nb01"])
        c += transposing_cases("COL generic transposing", 3840, dt, [rf"COL{tagf}  N=3840 K=2 inner=1 "])
        c += transposing_cases("COL generic transposing", 2160, dt, [rf"COL{tagf}  N=2160 K=2 inner=1 "], lines=13)
        # Bluestein: a small length and LDS-filling ones
        c += col_cases("BLUE", 37, 6, 9, dt, [rf"BLUE{tagf} N=37 "], align=1)
        c += row_cases("BLUE", 1366, 1, dt, [rf"BLUE{tagf} N=1366 "], line_pad=3, ragged=(3, 3, 2, 2), tags=["one", "two-gap", "prime-nb01", "ragged-host-oop"])
        c += col_cases("BLUE", 4100, 6, 8, dt, [rf"BLUE{tagf} N=4100 "], tags=["one", "prime-nb01"])
        c += transposing_cases("BLUE", 1366, dt, [rf"BLUE{tagf} N=1366 "], lines=5)[:2]
        # the O(N^2) pass, LDS lines and lines staged in device memory
        c += row_cases("DENSE", 1009, 1, dt, [rf"DENSE{tagf} N=1009 "], env=no_blue, line_pad=2, reject=["staged"])
        c += col_cases("DENSE", 211, 5, 8, dt, [rf"DENSE{tagf} N=211 "], env=no_blue, reject=["staged"], tags=["two-gap", "prime-nb01"])
        c += transposing_cases("DENSE", 1009, dt, [rf"DENSE{tagf} N=1009 "], env=no_blue, lines=3)[:2]
        staged = {"DSPFFT_NO_BLUESTEIN": "1", "DSPFFT_DENSE_STAGED": "1"}
        c += row_cases("DENSE staged", 4099, 1, dt, [rf"DENSE{tagf} N=4099 .*staged in device memory"], env=staged, line_pad=1, ragged=(3, 2, 2, 2),
                       tags=["one", "prime-nb01", "ragged-host-oop"])
        # plan-time compiled kernels (the emulation has no compiler: it runs the same geometry on the runtime-geometry kernels)
        jit = {"DSPFFT_JIT": "1"}
        c += row_cases("ROW+ (JIT)", 1500, 3, dt, [rf"ROW\+{tagf} N=1500 C=3 compiled at plan time"], env=jit, line_pad=9, emul="generic",
                       emul_expect=[rf"ROW{tagf}  N=1500 C=3 "], tags=["one", "two-gap", "prime-nb01"])
        c += col_cases("COL+ (JIT)", 1000, 48, 64, dt, [rf"COL\+{tagf} N=1000 K=\d+ compiled at plan time"], env=jit, emul="generic",
                       emul_expect=[rf"COL{tagf}  N=1000 "], tags=["one", "two-gap", "prime-nb01"])
    # ROW*: C = 3 and C = 1 (any row pitch: pixels are moved sample by sample), doubles as whole lines and as channel lines
    c += row_cases("ROW*", 3840, 3, "f32", [r"ROW\* N=3840 C=3 spec#"], line_pad=12)
    c += row_cases("ROW*", 960, 3, "f32", [r"ROW\* N=960 C=3 spec#"], line_pad=5, tags=["two-gap", "prime-nb01"])      # an odd pitch stays on the listed kernel
    c += row_cases("ROW*", 1920, 1, "f32", [r"ROW\* N=1920 C=1 spec#"], line_pad=4)
    c += row_cases("ROW*", 1920, 3, "f64", [r"ROW\* f64 N=1920 C=3 spec#\d+ threads"], line_pad=6)
    c += row_cases("ROW*", 1280, 1, "f64", [r"ROW\* f64 N=1280 C=1 spec#\d+ threads"], line_pad=3, tags=["two-gap", "prime-nb01", "ragged-host"])
    for N in (3840, 4096, 7680):        # chan_work: groups of eight lines -- tail only (1, 2), one group + tail (14), ragged under a host loop (30)
        c += row_cases("ROW* channel lines", N, 3, "f64", [rf"ROW\* f64 N={N} C=3 spec#\d+ as 3 channel lines"], line_pad=6,
                       tags=None if N == 3840 else ["two-gap", "prime-nb01", "ragged-host-oop"])
    # COL*: inner runs of K x odd (narrower listed tiles), padded rows, planes with gaps
    c += col_cases("COL*", 2160, 24, 32, "f32", [r"COL\* N=2160 K=8 spec#"])
    c += col_cases("COL*", 1080, 48, 52, "f32", [r"COL\* N=1080 K=16 spec#"])
    c += col_cases("COL*", 256, 96, 100, "f32", [r"COL\* N=256 K=32 spec#"], tags=["two-gap", "prime-nb01", "ragged-host-oop"])
    c += col_cases("COL*", 2160, 12, 16, "f64", [r"COL\* f64 N=2160 K=4 spec#"])
    c += col_cases("COL*", 1080, 24, 28, "f64", [r"COL\* f64 N=1080 K=8 spec#"], tags=["two-gap", "prime-nb01", "ragged-host-oop"])
    # BLOCK: block-major stacks with a gap between blocks, and the blocks of a volume embedded in a larger one (side by side)
    for i, (bd, bh, bw) in enumerate([(8, 8, 8), (4, 4, 4), (16, 16, 16)]):
        vol = bd * bh * bw
        kind = (K10, K01)[i % 2]
        for tag, di, do, inplace in (("in place", vol + 16, vol + 16, True), ("other dist out", vol + 4, vol + 32, False)):
            c.append(Case(f"BLOCK block-major {bw}x{bh}x{bd} x 37 {tag}", "BLOCK block-major", [(bd, bh * bw, bh * bw), (bh, bw, bw), (bw, 1, 1)], [(37, di, do)],
                          [kind] * 3, [rf"BLOCK {bw}x{bh}x{bd} .*block-major"], inplace=inplace, scaled_axis=1 if not inplace else None, seed=40 + i))
        D, H, W = 2 * bd, 3 * bh, 5 * bw
        for tag, (hi, wi), (ho, wo), inplace in (("in place", (H + 1, W + 4), (H + 1, W + 4), True), ("other pitches out", (H + 2, W + 8), (H, W + 12), False)):
            dims = [(bd, hi * wi, ho * wo), (bh, wi, wo), (bw, 1, 1)]
            how = [(D // bd, bd * hi * wi, bd * ho * wo), (H // bh, bh * wi, bh * wo), (W // bw, bw, bw)]
            c.append(Case(f"BLOCK side by side {bw}x{bh}x{bd} in a padded volume {tag}", "BLOCK side by side", dims, shuffled(how, i), [kind] * 3,
                          [rf"BLOCK {bw}x{bh}x{bd} .*side by side"], inplace=inplace, scaled_axis=2 if inplace else None, seed=50 + i))
    return c


def frame_cases():
    """the rank-2 and rank-3 cases: the only ones near a 4K frame"""
    c = []

    def many(n, howmany, embed_in, stride, dist_in, embed_out=None, ostride=None, dist_out=None):
        embed_out = embed_in if embed_out is None else embed_out
        ostride = stride if ostride is None else ostride
        dist_out = dist_in if dist_out is None else dist_out
        kw = dict(n=list(n), howmany=howmany, inembed=list(embed_in), istride=stride, idist=dist_in, onembed=list(embed_out), ostride=ostride, odist=dist_out)
        dims, si, so = [], stride, ostride
        for a in range(len(n) - 1, -1, -1):
            dims.insert(0, (n[a], si, so))
            si *= embed_in[a]; so *= embed_out[a]
        return kw, dims, ([(howmany, dist_in, dist_out)] if howmany > 1 else [])

    # two RGB frames with padded rows and a gap between them, as interleaved frames are laid out: the forced outer-radix-2 split (row pairs +
    # half tiles).  Frames are a guru batch dimension; the reduced copy is the one the emulation can afford.
    for (h, w, emul) in ((512, 512, "run"), (2160, 3840, "describe")):
        pitch = w * 3 + 12
        frame = h * pitch + 40
        for kind, inplace in ((K10, True), (K01, False)):
            c.append(Case(f"split {w}x{h}x3 two frames, padded rows, {'in place' if inplace else 'out of place'} kind={kind}", "ROW*2 + COL*/2 (split)",
                          [(h, pitch, pitch), (w, 3, 3)], [(3, 1, 1), (2, frame, frame)], [kind, kind],
                          [rf"ROW\*2 N={w} C=3 row pairs", rf"COL\*/2 N={h} as 2 x {h // 2}"], env={"DSPFFT_FORCE_SPLIT": "1"}, inplace=inplace, emul=emul, seed=60 + h))
    # motion's plane batch: inembed = onembed = minbuf > n on both inner axes (motion.c:535-552), mixed kinds across the axes
    mh, mw = 1080 + 8, 1920 + 16
    kw, dims, how = many([1080, 1920], 3, [mh, mw], 1, mh * mw)
    c.append(Case("motion 1920x1080 planes in minbuf, in place", "ROW* + COL* (frames)", dims, how, [K10, K01], [r"ROW\* N=1920 C=1 spec#", r"COL\* N=1080 K=16 spec#"],
                  inplace=True, many=kw, scaled_axis=1, emul="describe", seed=70))
    kw, dims, how = many([270, 480], 3, [270 + 2, 480 + 4], 1, 272 * 484)
    c.append(Case("motion 480x270 planes in minbuf, in place", "ROW + COL (frames)", dims, how, [K10, K01], [r"ROW  N=480 C=1 ", r"COL  N=270 "],
                  inplace=True, many=kw, scaled_axis=1, seed=71))
    # a 256 x 54 x 96 volume embedded in a larger one: the COL 256 entries over padded planes (z), generic columns (y), rows (x)
    kw, dims, how = many([256, 54, 96], 1, [256, 54 + 2, 96 + 8], 1, 0)
    c.append(Case("volume 96x54x256 embedded, in place", "volume (COL* 256)", dims, how, [K10, K01, K10], [r"axis 0: COL\* N=256 K=\d+ spec#"], inplace=True, many=kw, seed=72))
    kw, dims, how = many([256, 54, 96], 1, [256, 56, 104], 1, 0, embed_out=[256, 54, 96 + 4])
    c.append(Case("volume 96x54x256 embedded, to another embedding", "volume (COL* 256)", dims, how, [K01, K01, K10], [r"axis 0: COL\* N=256 K=\d+ spec#"], many=kw,
                  scaled_axis=0, seed=73))
    return c


_table = None


def all_cases():
    global _table
    if _table is None:
        entries, _ = entry_cases()
        _table = family_cases() + frame_cases() + entries
        names = [c.name for c in _table]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return _table


def case_ids():
    return [c.name for c in all_cases()]


def family_counts():
    out = {}
    for c in all_cases():
        out[c.family] = out.get(c.family, 0) + 1
    return out
