"""The E-step's launch planner (csrc/vbhem_estep_plan.h) through its host check build
(tests/plancheck): every field of plan_split and plan_fb equals the table recorded from
the planner as it stood inside vbhem_capi.hip (tests/golden/estep_plan_table.txt), so a
changed offset or a differently chosen block size fails here, without a GPU.  The table's
rows are the grid below; SplitLayout<S, LPC> against the run-time layout functions is a
static_assert of the check build itself."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANCHECK_PATH = os.path.join(ROOT, "tests", "plancheck", "libplancheck.so")
TABLE_PATH = os.path.join(ROOT, "tests", "golden", "estep_plan_table.txt")
COV_DIAG, COV_FULL = 0, 1

SPLIT_FIELDS = ("ok nwb lpc ppb off_Y off_F off_R off_L off_T lds lds_bwd lds_list list_nwb "
                "list_off_Y list_off_F list_off_R list_off_L list_off_T lds_l").split()
FB_FIELDS = ("found PPB threads lds BI BJ njb pair_stride off_At off_amax off_lpi off_Ab off_pib "
             "off_flag off_reg off_k1m off_k1P off_k1c off_k1mu off_k1C").split()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(PLANCHECK_PATH):
        subprocess.run(["make", "-C", ROOT, "plancheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(PLANCHECK_PATH)
    ci, vp, ll = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    lib.plancheck_split.argtypes = [ci] * 7 + [vp]
    lib.plancheck_split.restype = None
    lib.plancheck_fb.argtypes = [ci] * 6 + [vp]
    lib.plancheck_fb.restype = None
    lib.plancheck_persistent_blocks.argtypes = [ll, ll, ll]
    lib.plancheck_persistent_blocks.restype = ll
    return lib


@pytest.fixture(scope="module")
def table():
    """{"split": {(SB, d, covmode, K, S, T, LPC): values}, "fb": {(SB, d, covmode, K, S, T): values}}"""
    rows = {"split": {}, "fb": {}}
    with open(TABLE_PATH) as f:
        for line in f:
            if line.startswith("#"):
                continue
            key, values = line.split(":")
            kind, *args = key.split()
            rows[kind][tuple(int(x) for x in args)] = [int(x) for x in values.split()]
    return rows


def lpcs(S):
    """Lanes per column of the two plans the scheduler makes: dense / list, backward-only."""
    return (1 if S <= 4 else 2 if S <= 8 else 4, 1 if S <= 8 else 2)


def test_plan_split_is_the_recorded_plan(lib, table):
    grid = set()
    for S in range(1, 17):
        for SB, T, K, LPC in itertools.product({1, S}, (1, 2, 10, 50, 200), (1, 16, 2400), set(lpcs(S))):
            grid.add((SB, 2, COV_FULL, K, S, T, LPC))
    refused = {(5, 2, COV_FULL, 16, 4, 10, 1), (4, 65, COV_FULL, 16, 4, 10, 1)}  # SB > S; d = 65
    assert set(table["split"]) == grid | refused
    out = np.zeros(len(SPLIT_FIELDS), dtype=np.int64)
    for key, want in table["split"].items():
        lib.plancheck_split(*key, out.ctypes.data)
        assert dict(zip(SPLIT_FIELDS, out.tolist())) == dict(zip(SPLIT_FIELDS, want)), key
    for key in refused:
        assert table["split"][key][0] == 0, key
    # the grid is not all of one kind: plans that fit, plans refused for LDS, list
    # geometries of 8 waves and of fewer
    oks = [v for v in table["split"].values() if v[0]]
    assert 0 < len(oks) < len(table["split"]) - len(refused)
    assert {v[12] for v in oks} >= {8, 1} and {v[1] for v in oks} >= {1, 2, 4}


def test_plan_fb_is_the_recorded_plan(lib, table):
    grid = set(itertools.product(
        ((1, 3), (3, 2), (5, 5), (8, 8), (12, 12), (16, 16), (16, 32), (23, 23)),  # (S, SB)
        ((2, COV_FULL), (8, COV_FULL), (16, COV_FULL), (4, COV_DIAG)), (1, 3, 32), (2, 10, 50)))
    assert set(table["fb"]) == {(SB, d, cov, K, S, T) for (S, SB), (d, cov), K, T in grid}
    out = np.zeros(len(FB_FIELDS), dtype=np.int64)
    for key, want in table["fb"].items():
        lib.plancheck_fb(*key, out.ctypes.data)
        assert dict(zip(FB_FIELDS, out.tolist())) == dict(zip(FB_FIELDS, want)), key
    # S SB = 512 is the launch bound, 529 past it
    assert any(v[0] for k, v in table["fb"].items() if (k[4], k[0]) == (16, 32))
    assert not any(v[0] for k, v in table["fb"].items() if (k[4], k[0]) == (23, 23))


def test_persistent_blocks(lib):
    """Blocks per cluster of a persistent grid: at most the tiles and the device's resident
    blocks shared among the K clusters, at least one; from 8 up a multiple of 8."""
    for tiles, resident, K in itertools.product((0, 1, 7, 8, 9, 1000), (1, 256, 2048), (1, 16, 300)):
        nb = max(1, min(tiles, resident // K))
        if nb >= 8:
            nb = nb // 8 * 8
        assert lib.plancheck_persistent_blocks(tiles, resident, K) == nb, (tiles, resident, K)
