"""CPU: which listed fused column kernels keep their twiddle tables in LDS (dct_spec.h ColSpecT::RT_TABLES, spec_fused.h), as
dspfft_col_roundtrip_table_bytes reports it for the product library and for the emulation build of the same sources.

The kernel stages, behind its tile, W[m TW] (m < M1) of every stage with M1 > 1 and T[k], k <= N/2: 8 bytes an entry.  It does so only
where tile + tables leave as many workgroups resident in a CU's 160 KB as the tile alone -- counted as the hardware allocates: the kernel's
32-byte static block in front, rounded up to granules of 1280 bytes --; elsewhere it keeps its global loads and the entry reports 0.
Both rules are recomputed here from spec_list.h, so a change of either in the headers shows."""
import os
import re

import pytest

from dspfun_amd import _lib
from emul_lib import emul

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
CU_LDS = 160 * 1024
STATIC, GRANULE = 32, 1280         # the fused kernel's static block (its coded count, padded to the tile's alignment); gfx950's LDS allocation granule
COL_PADC = 1                       # dct_spec.h DSP_COL_PADC: one padding row per first-stage sub-block where there are two stages or more


def listed_tiles():
    """(N, K, T, radices) of DSPFFT_COL_SPECS_A and _B"""
    text = open(os.path.join(CSRC, "spec_list.h")).read()
    body = text[text.index("#define DSPFFT_COL_SPECS_A"):text.index("#define DSPFFT_COL_SPECS(X)")]
    tiles = [tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"\bX\((\d+(?:\s*,\s*\d+)+)\)", body)]
    return [(t[0], t[1], t[2], t[3:]) for t in tiles]


def table_entries(n, radices):
    """sum of M1 over the stages with M1 > 1 (M1 = product of the LATER radices), plus N/2 + 1"""
    total = 0
    for i in range(len(radices)):
        m1 = 1
        for r in radices[i + 1:]:
            m1 *= r
        if m1 > 1:
            total += m1
    return total + n // 2 + 1


def tile_bytes(n, k, radices):
    rows = n + (radices[0] * COL_PADC if len(radices) >= 2 else 0)
    return rows * (k // 2) * 8


def resident(nbytes):
    """workgroups of that many dynamic bytes a CU holds"""
    return CU_LDS // (-(-(nbytes + STATIC) // GRANULE) * GRANULE)


def expected(n, k, radices):
    tile, tab = tile_bytes(n, k, radices), 8 * table_entries(n, radices)
    return tab if resident(tile + tab) == resident(tile) else 0


TILES = listed_tiles()


@pytest.fixture(scope="module", params=["product", "emulation"])
def lib(request):
    return _lib.load() if request.param == "product" else emul()


def test_the_list_was_read():
    assert len(TILES) >= 20 and (2160, 8, 512, (12, 12, 15)) in TILES and (1080, 16, 512, (12, 10, 9)) in TILES
    for n, k, t, radices in TILES:
        p = 1
        for r in radices:
            p *= r
        assert p == n


def test_the_benchmark_tiles_stage_their_tables(lib):
    # 2160 x 8: 180 + 15 + 1081 entries, 1080 x 16: 90 + 9 + 541
    assert lib.dspfft_col_roundtrip_table_bytes(2160, 8, 512) == 8 * (180 + 15 + 1081) == 10208
    assert lib.dspfft_col_roundtrip_table_bytes(1080, 16, 512) == 8 * (90 + 9 + 541) == 5120


@pytest.mark.parametrize("n,k,t,radices", TILES, ids=[f"{n}x{k}x{t}" for n, k, t, _ in TILES])
def test_every_listed_tile_follows_the_count_and_the_fit_rule(lib, n, k, t, radices):
    assert lib.dspfft_col_roundtrip_table_bytes(n, k, t) == expected(n, k, radices)


def test_a_tile_whose_tables_do_not_fit_reports_zero(lib):
    misfits = [(n, k, t) for n, k, t, radices in TILES if expected(n, k, radices) == 0]
    assert misfits, "the fit rule leaves every listed tile its tables: no misfit to look at"
    for n, k, t in misfits:
        assert lib.dspfft_col_roundtrip_table_bytes(n, k, t) == 0
    # ... and it is the rule, not the count, that says so
    n, k, t = misfits[0]
    radices = next(r for a, b, c, r in TILES if (a, b, c) == (n, k, t))
    tile, tab = tile_bytes(n, k, radices), 8 * table_entries(n, radices)
    assert tab > 0 and resident(tile + tab) < resident(tile)


def test_the_rule_counts_granules():
    # 1080 x 8: 34944 + 5120 + 32 bytes round up to 40960, and four of those are a CU's LDS to the byte; one granule more would cost a workgroup
    assert resident(34944 + 5120) == 4 == resident(34944) and resident(34944 + 5120 + GRANULE) == 3
    assert expected(1080, 8, (12, 10, 9)) == 5120


def test_an_unlisted_tile_reports_minus_one(lib):
    for n, k, t in [(2160, 16, 512), (2160, 8, 256), (364, 16, 128), (0, 0, 0)]:
        assert lib.dspfft_col_roundtrip_table_bytes(n, k, t) == -1
