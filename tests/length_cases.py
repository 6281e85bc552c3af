"""Shared table of transform LENGTHS -- TEST INFRASTRUCTURE ONLY (tests/test_lengths_cpu.py, tests/test_lengths_gpu.py).

The planner factors every length over engine.cpp's kRadices; the butterflies of radix 7, 11 and 13 (radix.h: DftOddPrime) exist for the
runtime-geometry ROW / COL passes, the Bluestein convolution, the kernels compiled at plan time and the temporal block kernel.  This
module names the lengths that reach them and restates, in Python, how the planner orders the radices, so that a test can say WHICH
stage position of WHICH radix a length exercises.  The restatements are never trusted on their own: every test that uses one first
asserts it equals what `Plan.describe()` names (`pin_fft`, `pin_conv`, `pin_spec`), so a planner change fails there instead of quietly
moving the coverage."""
import math
import re

import numpy as np

import geometry_cases as gc

RADICES = (16, 15, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2)          # engine.cpp: kRadices, in its order


def _smooth(n, primes):
    for p in primes:
        while n % p == 0:
            n //= p
    return n == 1


SMOOTH13 = [n for n in range(2, 1025) if _smooth(n, (2, 3, 5, 7, 11, 13))]          # what the README promises the temporal kernel
assert len(SMOOTH13) == 245
ROUGH = [n for n in range(17, 700) if not _smooth(n, (2, 3, 5, 7, 11, 13))]         # a prime factor above 13: Bluestein's range
TINY = list(range(1, 33))


# ------------------------------------------------------------ the planner, restated ------------------------------------------------------------
def factorize(L):
    """engine.cpp factorize / factor_search: the fewest stages, then the smallest sum of radices (the first such multiset in the search's
    order: radices tried in kRadices' order, non-increasing along a path), sorted ascending.  None: no factorisation."""
    if L == 1:
        return []
    for maxdepth in range(1, 9):
        best = []

        def search(rem, cur, minr):
            if rem == 1:
                if not best or len(cur) < len(best[0]) or (len(cur) == len(best[0]) and sum(cur) < sum(best[0])):
                    best[:] = [list(cur)]
                return
            if len(cur) == maxdepth:
                return
            for r in RADICES:
                if r > minr or rem % r:
                    continue
                cur.append(r)
                search(rem // r, cur, r)
                cur.pop()
        search(L, [], 16)
        if best:
            return sorted(best[0])
    return None


def jit_radices(radices):
    """engine.cpp jit_radices: descending, then the last odd radix of that order (the smallest odd one) moved to the end"""
    r = sorted(radices, reverse=True)
    for i in range(len(r) - 1, -1, -1):
        if r[i] % 2:
            r.append(r.pop(i))
            break
    return r


def blue_length(N):
    """engine.cpp blue_length(2 N - 1): the 7-smooth M in [lo, lo + lo / 3 + 16] with the smallest stages x M (the first such M)"""
    lo = 2 * N - 1
    best = None
    for M in range(lo, lo + lo // 3 + 16 + 1):
        if not _smooth(M, (2, 3, 5, 7)):
            continue
        f = factorize(M)
        if f is None:
            continue
        cost = len(f) * M
        if best is None or cost < best[0]:
            best = (cost, M, f)
    return (best[1], best[2]) if best else None


# ------------------------------------------------------------ what describe() prints ------------------------------------------------------------
def _rad(text):
    return [int(v) for v in text.split("x")]


def parse_fft(text):
    """[(L, [r1, r2 ...])] of every `fft=L(r1xr2...)` (ROW and COL lines)"""
    return [(int(m.group(1)), [] if m.group(1) == "1" else _rad(m.group(2))) for m in re.finditer(r"\bfft=(\d+)\(([\dx]+)\)", text)]


def parse_conv(text):
    """[(M, [r1, r2 ...])] of every `conv=M(...)` (BLUE lines)"""
    return [(int(m.group(1)), _rad(m.group(2))) for m in re.finditer(r"\bconv=(\d+)\(([\dx]+)\)", text)]


def parse_spec(text):
    """[(kind, sample type, N, C or K, threads, [radices])] of every RowSpecT<...> / ColSpecT<...> type string (ROW+ and COL+ lines)"""
    out = []
    for m in re.finditer(r"\b(Row|Col)SpecT<(float|double), ([\d, ]+)>", text):
        v = [int(x) for x in m.group(3).split(",")]
        out.append((m.group(1), m.group(2), v[0], v[1], v[2], v[3:]))
    return out


def family_of(text):
    """the kernel family an `axis 0:` line names: ROW, ROW*, ROW+, COL, COL*, COL+, BLUE, TINY, DENSE, BLOCK"""
    m = re.search(r"axis \d+: ([A-Z]+[*+]?)", text)
    assert m, text
    return m.group(1)


def pin_fft(text, L):
    """the radices describe() names for an FFT of L points, after asserting that the restatement gives the same"""
    got = parse_fft(text)
    assert len(got) == 1 and got[0][0] == L, (L, text)
    assert got[0][1] == factorize(L), (L, got[0][1], factorize(L), text)
    return got[0][1]


def pin_conv(text, N):
    got = parse_conv(text)
    assert len(got) == 1, (N, text)
    M, f = blue_length(N)
    assert got[0] == (M, f), (N, got[0], (M, f), text)
    return got[0][1]


def pin_spec(text, kind, L):
    """the radices of the one compiled kernel's type string, after asserting jit_radices(factorize(L)) gives the same"""
    got = parse_spec(text)
    assert len(got) == 1 and got[0][0] == kind, (kind, L, text)
    assert got[0][5] == jit_radices(factorize(L)), (L, got[0][5], jit_radices(factorize(L)), text)
    assert int(np.prod(got[0][5])) == L
    return got[0][5]


# ------------------------------------------------------------------ coverage ------------------------------------------------------------------
def positions(radices):
    """{(radix, "only" | "first" | "mid" | "last")} of one stage list"""
    n = len(radices)
    if n == 1:
        return {(radices[0], "only")}
    return {(r, "first" if i == 0 else "last" if i == n - 1 else "mid") for i, r in enumerate(radices)}


def coverage(stage_lists):
    out = set()
    for r in stage_lists:
        out |= positions(r)
    return out


def table(cov):
    """{radix: "only, first, ..."} in the order only, first, mid, last"""
    order = ("only", "first", "mid", "last")
    return {r: ", ".join(p for p in order if (r, p) in cov) for r in sorted({r for r, _ in cov})}


# the planner's order over SMOOTH13 as COL lengths (test_lengths_cpu.py derives it from the restatement and both sweeps
# assert it from describe()'s strings)
COL_TABLE = {**{r: "only, first" for r in (2, 3, 4)}, **{r: "only, first, mid, last" for r in range(5, 14)}, **{r: "only, first, last" for r in (15, 16)}}
# the same for the ROW pass's L = N / 2 over the even lengths of SMOOTH13 (L <= 512, at most three stages)
ROW_LENGTHS = [n for n in SMOOTH13 if n % 2 == 0]


def cover_subset(lengths, of=lambda n: n, order=factorize, need=None):
    """a small subset of `lengths` whose stage lists order(of(n)) still reach every (radix, position) the whole list reaches (or `need`):
    greedy, shortest lengths first among equals"""
    need = set(coverage(order(of(n)) for n in lengths) if need is None else need)
    out = []
    while need:
        n = max(lengths, key=lambda v: (len(positions(order(of(v))) & need), -v))
        gain = positions(order(of(n))) & need
        assert gain, need
        need -= gain
        out.append(n)
    return sorted(out)


# ------------------------------------------------------------------- shapes -------------------------------------------------------------------
NO_TINY = {"DSPFFT_NO_TINY": "1"}            # lengths <= 32 reach ROW and COL only with it
KINDS = (gc.K10, gc.K01)
COL_SHAPE = dict(inner=6, pitch=9, align=1)  # no listed or compiled kernel takes it (a pitch of 9 breaks the 4-sample rule)


def _with_kind(case, kind):
    case.kinds = [kind]
    case.name += f" kind={'REDFT10' if kind == gc.K10 else 'REDFT01'}"
    return case


def col_case(family, N, dtype, kind, expect, env=None, reject=()):
    """the prime-nb01 variant: padded lines, nb0 and nb1 with different gaps, out of place into another pitch, fused scales"""
    c = gc.col_cases(family, N, COL_SHAPE["inner"], COL_SHAPE["pitch"], dtype, expect, env=env, align=COL_SHAPE["align"], tags=["prime-nb01"], reject=reject)[0]
    return _with_kind(c, kind)


def row_case(family, N, C, dtype, kind, expect, env=None, line_pad=3, reject=()):
    c = gc.row_cases(family, N, C, dtype, expect, env=env, line_pad=line_pad, tags=["prime-nb01"], reject=reject)[0]
    return _with_kind(c, kind)


def tagf(dtype):
    return " f64" if dtype == "f64" else ""


def sweep_col(N, dtype, kind):
    return col_case("COL", N, dtype, kind, [rf"COL{tagf(dtype)}  N={N} K=\d+ inner=6 "], env=NO_TINY, reject=[r"COL[*+]"])


def sweep_row(N, C, dtype, kind):
    """generic ROW, or the listed ROW* kernel of (N, C) where there is one: the caller counts the case under the family describe() names"""
    return row_case("ROW", N, C, dtype, kind, [rf"ROW\*?{tagf(dtype)} +N={N} C={C} "], env=NO_TINY)


def sweep_blue(N, dtype, kind):
    return col_case("BLUE", N, dtype, kind, [rf"BLUE{tagf(dtype)} N={N} K=\d+ inner=6 "], env=NO_TINY)


def tiny_cases(N, dtype, kind):
    """packed (257 contiguous lines: several LDS chunks and a ragged tail; out of place with fused scales) and strided (the COL shape)"""
    packed = gc.Case(f"TINY packed {dtype} N={N} x 257 lines", "TINY packed", [(N, 1, 1)], [(257, N, N)], [kind],
                     [rf"TINY{tagf(dtype)} N={N} .* packed"], dtype=dtype, scaled_axis=0, seed=N)
    strided = col_case("TINY", N, dtype, kind, [rf"TINY{tagf(dtype)} N={N} "], reject=["packed"])
    return [_with_kind(packed, kind), strided]


def chunks(values, size=32):
    values = list(values)
    n = max(1, -(-len(values) // size))
    per = -(-len(values) // n)
    return [values[i:i + per] for i in range(0, len(values), per)]


def chunk_id(c):
    return f"{c[0]}..{c[-1]}"


ROW_TABLE = table(coverage(factorize(n // 2) for n in ROW_LENGTHS if n > 2))
ROW_C3_LENGTHS = cover_subset([n for n in ROW_LENGTHS if n > 2], of=lambda n: n // 2)


class Worst:
    """the worst (max, rms) per (family, dtype) of a sweep, and the lengths that ran under it"""

    def __init__(self):
        self.by = {}

    def add(self, family, dtype, N, m, r):
        w = self.by.setdefault((family, dtype), dict(max=0.0, rms=0.0, at=None, lengths=[]))
        if m > w["max"]:
            w["max"], w["at"] = m, N
        w["rms"] = max(w["rms"], r)
        if N not in w["lengths"]:
            w["lengths"].append(N)

    def report(self, what):
        for (family, dtype), w in sorted(self.by.items()):
            print(f"GEOMETRY sweep {what} family={family!r} dtype={dtype} worst max={w['max']:.3e} (N={w['at']}) rms={w['rms']:.3e} lengths={w['lengths']}")


# ------------------------------------------------------- kernels compiled at plan time -------------------------------------------------------
JIT_L = (98, 286, 338, 343, 686, 1001, 1331, 2197)          # 7,2,7 / 13,2,11 / 13,2,13 / 7,7,7 / 7,7,2,7 / 13,11,7 / 11,11,11 / 13,13,13
JIT_F64 = (286, 1001)
JIT_TAGS = ["one", "two-gap", "prime-nb01"]
JIT_ENV = {"DSPFFT_JIT": "1"}


def jit_params():
    """(family, N, C, dtype): COL+ at N = L (inner 48, pitch 64), ROW+ at N = 2 L with C = 1, N = 2002 also with C = 3"""
    out = []
    for L in JIT_L:
        for dt in ("f32",) + (("f64",) if L in JIT_F64 else ()):
            out.append(("COL+", L, 0, dt))
            out.append(("ROW+", 2 * L, 1, dt))
    out.append(("ROW+", 2002, 3, "f32"))
    return out


def jit_cases(family, N, C, dtype, tags=None):
    tags = JIT_TAGS if tags is None else tags
    if family == "COL+":
        return gc.col_cases("COL+ (JIT)", N, 48, 64, dtype, [rf"COL\+{tagf(dtype)} N={N} K=\d+ compiled at plan time"], env=JIT_ENV, tags=tags)
    return gc.row_cases("ROW+ (JIT)", N, C, dtype, [rf"ROW\+{tagf(dtype)} N={N} C={C} compiled at plan time"], env=JIT_ENV, line_pad=9, tags=tags)


def jit_fft_length(family, N):
    return N if family == "COL+" else N // 2


# ------------------------------------------------------------- the temporal kernel -------------------------------------------------------------
TEMPORAL_HW = (4, 37)       # P = 148: two tiles at K = 128, a short last tile at every width
TEMPORAL_NBLOCKS = 2        # the clip has 2 D + 1 frames: one frame cropped
TEMPORAL_RESCALED = [(2, 1024), (1024, 2), (1001, 1024), (1024, 1001), (14, 22), (22, 14), (26, 28), (338, 242), (169, 121), (7, 13), (13, 7), (3, 1000),
                     (130, 512), (520, 264), (66, 130)]       # the last three cross the tile widths' switches at 128, 256, 512 and the 256 / 512 threads' at m K = 8192
TEMPORAL_QUANT = cover_subset(SMOOTH13)                       # D = D' lengths that still reach every (radix, position)


def temporal_tile(D, S):
    """temporal_core.h: temporal_tile_k and temporal_threads"""
    m = max(D, S)
    K = 128
    while K > 16 and m * K * 4 > 64 * 1024:
        K >>= 1
    assert m * K * 4 <= 64 * 1024, (D, S)
    return K, (512 if m * K > 8192 else 256)


def temporal_tol(D, S, base):
    """motion_temporal_ref.TOL's own model: a transform of N points is log2 N + 3 roundings deep, 2 (log2 N + 3) + 3 for the chain; `base`
    stands for 25 roundings (N = 256) and errors grow as the root of their number -- never below `base`"""
    return base * math.sqrt(max(1.0, (2 * (math.log2(max(D, S)) + 3) + 3) / 25.0))


def temporal_impl(D, S):
    """the oracle's transforms: the direct O(N^2) sum up to 256 points, the port (pinned to it in tests/test_oracle.py) beyond"""
    return "direct" if max(D, S) <= 256 else "port"


def temporal_case(D, S, kind="band"):
    """motion_temporal_ref.case on the sweep's clip: [2 D + 1][4][37], computed once per session"""
    import motion_temporal_ref as tr
    if kind == "band" and min(D, S) < 8:
        kind = "band-pi"        # (the dyadic band leaves up to 40 % of the oracle's pixels of so few frames exactly on k + 1/2)
    return tr.case(D, S, kind, hw=TEMPORAL_HW, nblocks=TEMPORAL_NBLOCKS, impl=temporal_impl(D, S))
