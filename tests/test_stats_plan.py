"""The fused E-step epilogue's planner (csrc/vbhem_stats_plan.h) through its host check
build (tests/plancheck), without a GPU.

The recorded table (tests/golden/stats_plan_table.txt) is what the launch code did when
the choice lived in the launchers of vbhem_stats.hip: per key, every launch's kernel with
its template arguments, grid, block, dynamic LDS and nzero / stats_slabs.  Every plan must
reproduce its row, so a changed threshold or a different kernel fails here.  The table's
keys are the grid below; the assertions on the table keep the grid from going hollow."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANCHECK_PATH = os.path.join(ROOT, "tests", "plancheck", "libplancheck.so")
TABLE_PATH = os.path.join(ROOT, "tests", "golden", "stats_plan_table.txt")
COV_DIAG, COV_FULL = 0, 1

S_SB = [(S, SB) for S in (1, 4, 5, 8, 10, 12, 16) for SB in sorted({1, S}) if SB == S or S in (5, 10, 16)]
D_COV = [(d, COV_FULL) for d in (2, 4, 8, 9, 11, 14, 16)] + [(d, COV_DIAG) for d in (2, 12, 16)]
K_KT = [(K, KT) for K in (1, 8, 16, 200) for KT in sorted({K, K // 2}) if KT >= 1]
OPERAND = (0, 1, 2)  # none, U only, U and its statistics copy Us
# (NO_STATS_M, NO_STATS_U, NO_STATS_G, SU_BLOCKS) for K clusters
SWITCH_SETS = {
    "default": lambda K: (0, 0, 0, -1),
    "NO_STATS_M": lambda K: (1, 0, 0, -1),
    "NO_STATS_U": lambda K: (0, 1, 0, -1),
    "NO_STATS_M+NO_STATS_G": lambda K: (1, 0, 1, -1),
    "SU_BLOCKS=K": lambda K: (0, 0, 0, K),
    "SU_BLOCKS=K+1": lambda K: (0, 0, 0, K + 1),
}
RESP_KERNELS = ("vhem", "trials", "kp", "generic")  # enum RespKernel
GATED_KERNELS = ("list4_reduce", "mfma", "grouped", "operand", "gather")  # enum GatedStats


def nu_of(d, cov):
    return 1 + d + (d * (d + 1) // 2 if cov == COV_FULL else d)


def gated_key(K, S, SB, d, cov, opnd, nchunk, resident, sw, fold=0, nbases=None):
    """nbases: the bases of the group (25 per chunk); nzero_m as the scheduler sets it"""
    return ("gated", K, S, SB, d, cov, opnd, nchunk, nchunk * 25 if nbases is None else nbases, resident,
            fold, min(nchunk, 128)) + tuple(SWITCH_SETS[sw](K))


GATED_REFUSED = gated_key(16, 16, 16, 32, COV_FULL, 0, 7, 256, "default")  # a 71 KB batch record
GATED_Z32 = [gated_key(K, 8, 8, 8, COV_FULL, 2, 512, 256, "default", nbases=(1 << 32) // K + off)
             for K, off in ((16, -1), (16, 0), (200, 1))]  # the 32-bit offset of Z: below, at, past


def grid():
    """The table's keys: every axis over a base shape; products only where axes interact."""
    keys = []
    few_shapes = ((4, 4), (16, 16), (10, 1))
    few_d = ((2, COV_FULL), (11, COV_FULL), (16, COV_FULL), (12, COV_DIAG))
    every_d_at = ((16, 16),)  # takes every d
    shape_d = [(s, dc) for s, dc in itertools.product(S_SB, D_COV) if dc in few_d or s in every_d_at]
    # dense schedule: the shapes at one K; the other K (the VHEM gate at K = 8) on a few
    for (S, SB), (d, cov) in shape_d:
        keys.append(("dense", 16, S, SB, d, cov, 0))
    for K, (S, SB), (d, cov) in itertools.product((1, 8, 200), few_shapes, few_d[::2]):
        keys.append(("dense", K, S, SB, d, cov, int(K == 8)))
    # responsibilities: K / trials (and K = 4, 32, 64 for the other KP kernels, 256 and 300 at
    # and past the trials kernel's range) x VHEM x RESP_GENERIC; the fold (its LDS grows
    # with S SB) at one K
    for (K, KT), vhem, gen in itertools.product(
            K_KT + [(4, 4), (32, 32), (64, 64), (256, 128), (300, 100)], (0, 1), (0, 1)):
        if not (vhem and gen):  # (the VHEM kernel has no generic variant)
            keys.append(("resp", K, KT, 4, 4, vhem, 0, gen))
    for (K, KT), vhem, (S, SB) in itertools.product(((16, 16), (16, 8)), (0, 1), few_shapes):
        keys.append(("resp", K, KT, S, SB, vhem, 1, 0))
    # gated schedule at one K, chunk count and residency: the shapes with the statistics
    # copy, on the operand alone, and (two d) without an operand
    for (S, SB), (d, cov) in shape_d:
        for opnd in OPERAND if (d, cov) in few_d[::2] else (1, 2):
            if opnd == 1 and nu_of(d, cov) > 64 and d != 11:
                continue  # (past 64 moment columns the operand alone changes nothing: d = 11 shows it)
            keys.append(gated_key(16, S, SB, d, cov, opnd, 512, 256, "default"))
    # ... every switch set where the operand kernels compete
    for sw, (S, SB), (d, cov), opnd in itertools.product(
            [s for s in SWITCH_SETS if s != "default"], ((4, 4), (16, 16)),
            ((2, COV_FULL), (8, COV_FULL)), (1, 2)):
        keys.append(gated_key(16, S, SB, d, cov, opnd, 512, 256, sw))
    # ... K x chunks x resident blocks: the block counts (residency: the MFMA kernel's alone)
    for K, nchunk, (S, SB, d), (opnd, res) in itertools.product(
            (1, 8, 200), (1, 7, 512), ((4, 4, 2), (16, 16, 16)), ((1, 256), (2, 256), (2, 2048))):
        keys.append(gated_key(K, S, SB, d, COV_FULL, opnd, nchunk, res, "default"))
    for K, nchunk, sw, opnd in itertools.product((1, 200), (7, 512), ("SU_BLOCKS=K", "SU_BLOCKS=K+1"), (2,)):
        keys.append(gated_key(K, 8, 8, 8, COV_FULL, opnd, nchunk, 256, sw))
    # ... the fold (an fb_exact_kernel launch first, or none), the Z offset, a refused shape
    for opnd, fold in itertools.product(OPERAND, (1, 2)):
        keys.append(gated_key(16, 8, 8, 8, COV_FULL, opnd, 7, 256, "default", fold=fold))
    keys += GATED_Z32 + [GATED_REFUSED]
    # the reduction after fb_list4_kernel's accumulating variant (S = 8)
    for d, cov in D_COV:
        keys.append(("l4reduce", 16, 8, d, cov))
    keys.append(("l4reduce", 1, 8, 8, COV_FULL))
    assert len(keys) == len(set(keys))
    return keys


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(PLANCHECK_PATH):
        subprocess.run(["make", "-C", ROOT, "plancheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(PLANCHECK_PATH)
    ci, vp, ll = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    lib.plancheck_stats_dense.argtypes = [ci] * 5 + [vp]
    lib.plancheck_resp.argtypes = [ci] * 7 + [vp]
    lib.plancheck_stats_gated.argtypes = [ci] * 7 + [ll, ll, ci, ci, vp, vp]
    lib.plancheck_list4_reduce.argtypes = [ci] * 4 + [vp]
    for f in (lib.plancheck_stats_dense, lib.plancheck_resp, lib.plancheck_stats_gated,
              lib.plancheck_list4_reduce):
        f.restype = None
    lib.plancheck_stats_m_blocks.argtypes = [ll, ci, ci, ll]
    lib.plancheck_stats_m_blocks.restype = ll
    return lib


@pytest.fixture(scope="module")
def table():
    """{key: [tokens]}: the launches recorded for the key (module docstring)"""
    rows = {}
    with open(TABLE_PATH) as f:
        for line in f:
            if line.startswith("#"):
                continue
            key, values = line.split(" : ")
            kind, *args = key.split()
            rows[(kind,) + tuple(int(x) for x in args)] = values.split()
    return rows


GATED_FIELDS = "ok kernel NTW G KSM NXR LG SM PER PB lds cap nzero stats_slabs exact_first blocks".split()


def gated_plan(lib, key):
    out = np.zeros(len(GATED_FIELDS), dtype=np.int64)
    sw = np.array(key[12:16], dtype=np.int64)
    lib.plancheck_stats_gated(*key[1:12], sw.ctypes.data, out.ctypes.data)
    return dict(zip(GATED_FIELDS, out.tolist()))


def gated_tokens(p, K):
    """A plan as the launch it stands for, in the table's words."""
    if not p["ok"]:
        return ["0"]
    kernel = GATED_KERNELS[p["kernel"]]
    if kernel == "list4_reduce":
        return [str(x) for x in ("vbhem::list4_stats_reduce_kernel", p["blocks"], 1, 1024, p["lds"], p["nzero"])]
    name, gy = {
        "mfma": ("stats_list_m_kernel<%d,%d,%d,%d,3>" % (p["NTW"], p["G"], p["KSM"], p["NXR"]), 1),
        "grouped": ("stats_list_g_kernel<%d,%d>" % (p["LG"], p["SM"]), K),
        "operand": ("stats_list_u_kernel<1,%d>" % p["SM"], K),
        "gather": ("stats_list_kernel<%d>" % p["PER"], K),
    }[kernel]
    return [str(x) for x in (p["PB"], "vbhem::" + name, p["blocks"], gy, 256, p["lds"], p["nzero"],
                             p["stats_slabs"], p["exact_first"])]


def test_the_plans_are_the_recorded_launches(lib, table):
    assert set(table) == set(grid())
    dense, resp, reduce_ = (np.zeros(n, dtype=np.int64) for n in (11, 5, len(GATED_FIELDS)))
    for key, want in table.items():
        kind = key[0]
        if kind == "dense":
            K, S, SB, d, cov, vhem = key[1:]
            lib.plancheck_stats_dense(K, S, SB, d, cov, dense.ctypes.data)
            ok, ngroups, lds, SBp, UST, JG, NBB, AST, TPW, per, unr = dense.tolist()
            got = [str(x) for x in (
                1, ngroups, lds, SBp, UST, JG, NBB, AST,
                "vbhem::stats_kernel<%d,%d>" % (TPW, vhem), 7, ngroups, 512, lds,
                "vbhem::nm_kernel<%d,%d,%d>" % (per, unr, vhem), 7, 1, 256, 0)] if ok else ["0"]
        elif kind == "resp":
            lib.plancheck_resp(*key[1:], resp.ctypes.data)
            ok, kernel, KP, lds, gate_lds = resp.tolist()
            name = {"vhem": "vhem_resp_kernel", "trials": "resp_trials_kernel", "kp": "resp_kernel<%d>" % KP,
                    "generic": "resp_kernel<0>"}[RESP_KERNELS[kernel]]
            got = (["vbhem::" + name, "512", str(lds)] if ok else ["refused"]) + [str(gate_lds)]
        elif kind == "gated":
            got = gated_tokens(gated_plan(lib, key), key[1])
        else:
            lib.plancheck_list4_reduce(*key[1:], reduce_.ctypes.data)
            got = gated_tokens(dict(zip(GATED_FIELDS, reduce_.tolist())), key[1])
        assert got == want, key


def test_the_table_reaches_every_kernel_and_bucket(table):
    def targs(prefix):
        """the template arguments of every recorded launch of a kernel"""
        out = set()
        for want in table.values():
            for tok in want:
                if tok.startswith("vbhem::" + prefix + "<"):
                    out.add(tuple(int(x) for x in tok[tok.index("<") + 1:-1].split(",")))
        return out

    names = {tok.split("<")[0] for want in table.values() for tok in want if tok.startswith("vbhem::")}
    assert names >= {"vbhem::" + n for n in (
        "list4_stats_reduce_kernel", "stats_list_m_kernel", "stats_list_g_kernel", "stats_list_u_kernel",
        "stats_list_kernel", "vhem_resp_kernel", "resp_trials_kernel", "resp_kernel", "stats_kernel",
        "nm_kernel")}
    assert {a[0] for a in targs("stats_list_g_kernel")} == {8, 16, 32}  # LG
    m = targs("stats_list_m_kernel")
    # the feature-tile ladder: 1, 2, 3, 4 tiles, 5-6, 7-8, more than 8 -> (NTW, G)
    assert {a[:2] for a in m} == {(1, 4), (2, 4), (3, 4), (4, 4), (3, 2), (4, 2), (3, 1)}
    assert {a[2] for a in m} == {1, 2, 3, 4}  # KSM
    assert {a[3] for a in m} == {1, 2, 3, 5}  # NXR
    assert targs("stats_list_kernel") == {(4,), (8,)}  # PER
    assert {a[:2] for a in targs("nm_kernel")} == {(6, 4), (24, 1)}
    assert {a[0] for a in targs("stats_kernel")} == {4, 8, 16}  # TPW
    assert {a[1] for a in targs("stats_kernel")} == {0, 1} == {a[2] for a in targs("nm_kernel")}  # the gate
    assert {a[0] for a in targs("resp_kernel")} == {0, 4, 8, 16, 32, 64}
    assert {a[1] for a in targs("stats_list_u_kernel")} == {4, 8, 12, 16}  # SM
    # (a lane group holds S^2 <= 128 entries: the grouped kernel stops at S = 11)
    assert {a[1] for a in targs("stats_list_g_kernel")} == {4, 8, 12}
    # refused plans of either schedule, of the responsibilities and of the reduction
    for kind in ("dense", "gated", "l4reduce"):
        assert any(k[0] == kind and v == ["0"] for k, v in table.items()), kind
    assert table[GATED_REFUSED] == ["0"]
    assert any(k[0] == "resp" and v[0] == "refused" for k, v in table.items())
    # the fb_exact_kernel launch first (fold = 1) and not (fold = 0, 2)
    assert {(k[10], v[-1]) for k, v in table.items() if k[0] == "gated" and v != ["0"]} == \
        {(0, "0"), (1, "1"), (2, "0")}
    # the MFMA kernel only while Z's offset fits 32 bits
    assert ["stats_list_m_kernel" in table[k][1] for k in GATED_Z32] == [True, False, False]


# tests/test_emission_u.py::test_stats_on_prepared_operand: its shapes (K, S, SB, d, cov), and
# what its comments say each switch set reaches.  Its groups are 64 bases (GROUP_BASES).
PREPARED_OPERAND_SHAPES = [
    pytest.param(16, 8, 8, 8, COV_FULL, id="full_d8"), pytest.param(8, 12, 12, 16, COV_FULL, id="full_d16"),
    pytest.param(6, 5, 4, 12, COV_DIAG, id="diag_d12"), pytest.param(4, 3, 3, 2, COV_FULL, id="full_d2_face"),
    pytest.param(3, 4, 4, 4, COV_FULL, id="full_d4_long")]


@pytest.mark.parametrize("prepare", [False, True])
@pytest.mark.parametrize("K,S,SB,d,cov", PREPARED_OPERAND_SHAPES)
def test_switch_sets_of_the_prepared_operand_test_reach_their_kernels(lib, K, S, SB, d, cov, prepare):
    def kernel(no_m=0, no_u=0, no_g=0, su_blocks=-1):
        key = ("gated", K, S, SB, d, cov, 2 if prepare else 1, 2, 64, 256, 0, 2, no_m, no_u, no_g, su_blocks)
        p = gated_plan(lib, key)
        assert p["ok"]
        return GATED_KERNELS[p["kernel"]], p

    NU = nu_of(d, cov)
    assert kernel(no_u=1)[0] == "gather"
    assert kernel()[0] == ("mfma" if prepare else kernel(no_m=1)[0])
    assert kernel(su_blocks=K + 1)[0] == kernel()[0]
    # without the MFMA kernel: the operand kernels up to 64 moment columns, one per lane;
    # the grouped one where a lane group fits the shape (its bounds written out)
    kdp = (d * (d + 1) // 2 + d if cov == COV_FULL else 2 * d) + 3 & ~3
    lanes = [LG for LG in (8, 16, 32)
             if NU <= LG and S * SB <= 4 * LG and S * S <= 4 * LG and kdp * SB <= 8 * LG]
    want = "gather" if NU > 64 else "grouped" if lanes else "operand"
    got, p = kernel(no_m=1)
    assert got == want and (not lanes or p["LG"] == lanes[0])
    assert kernel(no_m=1, su_blocks=K)[0] == want
    assert kernel(no_m=1, no_g=1)[0] == ("gather" if NU > 64 else "operand")


def test_stats_m_blocks(lib):
    """At least K + 1 blocks, at most the cap; SU_BLOCKS replaces the resident count."""
    for resident, K, cap in itertools.product((1, 256, 2048), (1, 16, 300), (1, 128, 8192)):
        assert lib.plancheck_stats_m_blocks(resident, K, cap, -1) == min(max(resident, K + 1), cap)
        for su in (0, K, K + 1, 5000):
            assert lib.plancheck_stats_m_blocks(resident, K, cap, su) == min(max(su, K + 1), cap)
