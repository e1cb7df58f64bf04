"""The preconditions of tests/test_fused_dimensions_gpu.py, on the oracle and the planner alone
(no GPU): every row of cases.DIMENSION_SHAPES sits where its comment says, so that no GPU test
there can pass vacuously.

* the gate regimes of tests/test_cluster_count_cases.py: at tscale = 100 some pair passes the gate
  Z > 1e-8, at 0.03 every pair does, at 1e-9 none, and no oracle Z lies within a relative 1e-3
  of the gate in any of them;
* through tests/plancheck, per row: the emission GEMM's k-steps kq, its register bucket (4, 12,
  40), W' rows and chunks; the gated plan's kernel and (NTW, G) from the feature tiles nt; the
  dense plan; whether fb_list4_kernel accumulates the statistics (S = 8 rows);
* coverage, so that a deleted row is noticed: with cases.SHAPES every full-covariance kq of
  d = 1 .. 16 and every nt = 1 .. 10 occurs; DIMENSION_SHAPES alone holds every (nt, G, NTW)
  that no other shape reaches;
* the switch sets of the GPU module's statistics test reach the kernels it names.

The references are computed once per row (functools.lru_cache) and never modified: the GPU
module imports them from here.
"""
import ctypes
import functools

import numpy as np
import pytest

import vbhem_oracle as vo
from cases import DIMENSION_SHAPES, SHAPES, make_case
from test_cluster_count_cases import (GATE, GATE_MARGIN, TS_ALLPASS, TS_GATED, TS_NONE, frozen, gate_margin,
                                      reference)
from test_gpu_parity import seed_of
from test_stats_plan import COV_FULL, GATED_KERNELS, gated_plan, lib, nu_of  # noqa: F401  (lib: a fixture)

ROWS = {s[0]: s for s in DIMENSION_SHAPES}
assert len(ROWS) == len(DIMENSION_SHAPES)

# d: (kq, bucket) of a full covariance, KD = d (d + 1) / 2 + d; the buckets' first and last kq
# are d = 1 / 4, 5 / 8 and 9 / 16
FULL_KQ = {1: (1, 4), 2: (2, 4), 3: (3, 4), 4: (4, 4), 5: (5, 12), 6: (7, 12), 7: (9, 12), 8: (11, 12),
           9: (14, 40), 10: (17, 40), 11: (20, 40), 12: (23, 40), 13: (26, 40), 14: (30, 40), 15: (34, 40),
           16: (38, 40)}
# what each row's comment claims: (kq, bucket, NU, (nt, G, NTW))
CLAIMS = {
    "d1_full": (1, 4, 3, (1, 4, 1)), "d6_full": (7, 12, 28, (2, 4, 2)), "d7_full": (9, 12, 36, (3, 4, 3)),
    "d9_full": (14, 40, 55, (4, 4, 4)), "d10_full": (17, 40, 66, (5, 2, 3)), "d11_full": (20, 40, 78, (5, 2, 3)),
    "d12_full": (23, 40, 91, (6, 2, 3)), "d13_full": (26, 40, 105, (7, 2, 4)),
    "d14_full": (30, 40, 120, (8, 2, 4)), "d15_full": (34, 40, 136, (9, 1, 3)),
    "d6_diag": (3, 4, 13, (1, 4, 1)), "d7_diag": (4, 4, 15, (1, 4, 1)), "d8_diag": (4, 4, 17, (2, 4, 2)),
    "d9_diag": (5, 12, 19, (2, 4, 2)), "d15_diag": (8, 12, 31, (2, 4, 2)),
    "d11_rows": (20, 40, 78, (5, 2, 3)), "d6_S8": (7, 12, 28, (2, 4, 2)), "d9_S8_ragged": (14, 40, 55, (4, 4, 4)),
    "d10_S12": (17, 40, 66, (5, 2, 3)),
}
# the (nt, G, NTW) of stats_list_m_kernel that only these rows reach
UNTESTED_TILES = {(4, 4, 4), (5, 2, 3), (6, 2, 3), (7, 2, 4), (8, 2, 4), (9, 1, 3)}
# (row, switches) of test_fused_dimensions_gpu.test_other_gated_statistics_kernels -> the kernel
STATS_SWITCH_ROWS = [
    ("d6_full", dict(NO_STATS_M=1), "grouped"),      # NU = 28: 32 lanes per pair
    ("d15_diag", dict(NO_STATS_M=1), "grouped"),     # NU = 31
    ("d6_full", dict(NO_STATS_M=1, NO_STATS_G=1), "operand"),
    ("d7_full", dict(NO_STATS_M=1), "operand"),      # NU = 36: past the grouped kernel's 32 lanes
    ("d9_full", dict(NO_STATS_M=1), "operand"),      # NU = 55
    ("d10_full", dict(NO_STATS_M=1), "gather"),      # NU = 66: just past the operand kernel's 64
    ("d13_full", dict(NO_STATS_U=1), "gather"),
]


@functools.lru_cache(maxsize=None)
def row_case(name):
    """(case, the oracle's per-pair outputs with sum_t_nu) of a DIMENSION_SHAPES row."""
    _, N, K, S, Sb, d, cov, T, ragged = ROWS[name]
    cs = make_case(N, K, S, Sb, d, cov, seed=seed_of(name) + 1, ragged=ragged, tau=T)
    pairs = vo.c_estep_pairs(cs["base"], cs["consts"], T, nthreads=4, want_tnu=True)
    frozen(pairs)
    return cs, pairs


@functools.lru_cache(maxsize=None)
def row_reference(name, tscale):
    """(tilde N, logOmega, hat_Z, Z, statistics) of the oracle at tilde N = tscale N omega."""
    return reference(*row_case(name), tscale, ROWS[name][6])


# ---- the planner (tests/plancheck) ------------------------------------------------------
EMISSION_FIELDS = "kq ksp ok bucket urc chunks nwave lds".split()


def emission_plan(lib, K, S, d, cov):  # noqa: F811
    """emission_kdp / 4, emission_ksp(K S) and plan_emission_u's fields."""
    lib.plancheck_emission.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.plancheck_emission.restype = None
    out = np.zeros(len(EMISSION_FIELDS), dtype=np.int64)
    lib.plancheck_emission(K, S, d, cov, out.ctypes.data)
    return dict(zip(EMISSION_FIELDS, out.tolist()))


def list4_accumulates(lib, K, S, Sb, T, d, cov):  # noqa: F811
    lib.plancheck_list4_acc.argtypes = [ctypes.c_int] * 6
    lib.plancheck_list4_acc.restype = ctypes.c_int
    return bool(lib.plancheck_list4_acc(K, S, Sb, T, d, cov))


def stats_plan(lib, shape, no_m=0, no_u=0, no_g=0):  # noqa: F811
    """The gated plan of a row's fused call on a prepared base set (one chunk of N bases)."""
    _, N, K, S, Sb, d, cov, T, ragged = shape
    nchunk = -(-N // 64)
    p = gated_plan(lib, ("gated", K, S, Sb, d, cov, 2, nchunk, N, 256, 1, nchunk, no_m, no_u, no_g, -1))
    assert p["ok"]
    return dict(p, name=GATED_KERNELS[p["kernel"]])


def tiles_of(d, cov):
    return -(-nu_of(d, cov) // 16)


# ---- the gate regimes ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROWS))
def test_gate_regimes(name):
    _, N, K = ROWS[name][:3]
    Z100, Zall, Znone = (row_reference(name, ts)[3] for ts in (TS_GATED, TS_ALLPASS, TS_NONE))
    margins = [gate_margin(Z) for Z in (Z100, Zall, Znone)]
    print("CASE", name, "gated pairs", int((Z100 > GATE).sum()), "of", N * K, "gate margins",
          ["%.1e" % m for m in margins])
    assert Z100.shape == (N, K) and np.isfinite(row_case(name)[1]["LL_elbo"]).all()
    assert (Z100 > GATE).any()            # short lists
    assert not (Z100 > GATE).all()
    assert (Zall > GATE).all()            # every list full
    assert not (Znone > GATE).any()       # every list empty
    assert min(margins) > GATE_MARGIN


# ---- the planner's buckets ----------------------------------------------------------------
def test_claims_name_every_row():
    assert set(CLAIMS) == set(ROWS)


@pytest.mark.parametrize("name", list(ROWS))
def test_row_sits_where_its_comment_says(lib, name):  # noqa: F811
    _, N, K, S, Sb, d, cov, T, ragged = ROWS[name]
    kq, bucket, NU, (nt, G, NTW) = CLAIMS[name]
    KD = d * (d + 1) // 2 + d if cov == COV_FULL else 2 * d
    em = emission_plan(lib, K, S, d, cov)
    p = stats_plan(lib, ROWS[name])
    dense = np.zeros(11, dtype=np.int64)
    lib.plancheck_stats_dense(K, S, Sb, d, cov, dense.ctypes.data)
    print("CASE", name, "emission", em, "gated", p["name"], (nt, p["G"], p["NTW"]), "dense ok/TPW",
          int(dense[0]), int(dense[8]), "list4", list4_accumulates(lib, K, S, Sb, T, d, cov))
    # the emission GEMM: k-steps, bucket, W' rows in chunks of urc row tiles
    assert kq == -(-KD // 4) and (cov != COV_FULL or FULL_KQ[d] == (kq, bucket))
    assert em["ok"] and (em["kq"], em["bucket"]) == (kq, bucket)
    assert em["ksp"] == -(-K * S // 128) * 128
    assert em["urc"] == (8 if bucket <= 12 else 4) and em["chunks"] * em["urc"] * 16 == em["ksp"]
    # the statistics: NU feature columns in nt tiles of 16
    assert NU == nu_of(d, cov) == 1 + KD and nt == tiles_of(d, cov)
    assert (p["name"], p["G"], p["NTW"]) == ("mfma", G, NTW)
    # the dense schedule fits every row (TPW = 4: at most 4 MFMA tiles per wave) -- the GPU
    # module keeps the refusal branch of test_fused_cluster_counts_gpu for a row that would not
    assert dense[0] == 1 and dense[8] == 4
    # fb_list4_kernel sums the gated statistics itself only at S = 8, T = 10, NU <= 48
    assert list4_accumulates(lib, K, S, Sb, T, d, cov) == (name == "d6_S8")


def test_rows_with_a_path_of_their_own(lib):  # noqa: F811
    # K S > 128 in the 40-step bucket: four W' chunks of 4 row tiles
    _, N, K, S, Sb, d, cov, T, ragged = ROWS["d11_rows"]
    em = emission_plan(lib, K, S, d, cov)
    assert K * S > 128 and (em["bucket"], em["ksp"], em["urc"], em["chunks"]) == (40, 256, 4, 4)
    assert em["chunks"] > 2
    # every other row: one chunk in the 4- and 12-step buckets, two in the 40-step one
    for name, (_, N, K, S, Sb, d, cov, T, ragged) in ROWS.items():
        if name != "d11_rows":
            em = emission_plan(lib, K, S, d, cov)
            assert em["chunks"] == (2 if em["bucket"] == 40 else 1), name
    # S = 8, T = 10: the accumulation at two feature tiles, its reduction planned; past three
    # tiles (NU = 55 > 48) fb_list4_kernel leaves the sums to stats_list_m_kernel
    reduce_ = np.zeros(16, dtype=np.int64)
    for name, acc in (("d6_S8", True), ("d9_S8_ragged", False)):
        _, N, K, S, Sb, d, cov, T, ragged = ROWS[name]
        assert (S, T) == (8, 10)
        assert list4_accumulates(lib, K, S, Sb, T, d, cov) == acc
        assert stats_plan(lib, ROWS[name])["name"] == "mfma"
    lib.plancheck_list4_reduce(4, 8, 6, 1, reduce_.ctypes.data)
    assert reduce_[0] == 1 and GATED_KERNELS[reduce_[1]] == "list4_reduce"
    assert tiles_of(6, 1) == 2 and ROWS["d9_S8_ragged"][4] < 8 and ROWS["d9_S8_ragged"][8]
    # ... not at T = 5 (the d6_full row), nor at S = 12
    assert not list4_accumulates(lib, 4, 8, 8, 5, 6, 1)
    _, N, K, S, Sb, d, cov, T, ragged = ROWS["d10_S12"]
    assert (S, T) == (12, 10) and Sb < S and emission_plan(lib, K, S, d, cov)["bucket"] == 40
    # past the emission GEMM's 40 k-steps (d = 17 full: 43) the plan is refused
    assert not emission_plan(lib, 4, 3, 17, 1)["ok"] and emission_plan(lib, 4, 3, 17, 1)["kq"] == 43


def test_every_dimension_bucket_is_reached(lib):  # noqa: F811
    """Over SHAPES and DIMENSION_SHAPES: every k-step count of a full covariance of d = 1 .. 16,
    every feature-tile count 1 .. 10; over DIMENSION_SHAPES alone the tile plans no other shape
    reaches."""
    both = SHAPES + DIMENSION_SHAPES
    full_kq = {emission_plan(lib, s[2], s[3], s[5], 1)["kq"] for s in both if s[6] == COV_FULL}
    assert full_kq >= {kq for kq, _ in FULL_KQ.values()}
    assert {emission_plan(lib, 4, 3, d, 1)["kq"] for d in FULL_KQ} == {kq for kq, _ in FULL_KQ.values()}
    assert {tiles_of(s[5], s[6]) for s in both} >= set(range(1, 11))
    tiles = set()
    for s in DIMENSION_SHAPES:
        p = stats_plan(lib, s)
        tiles.add((tiles_of(s[5], s[6]), p["G"], p["NTW"]))
    assert tiles >= UNTESTED_TILES
    # the diagonal rows' k-steps: 3, 4 (twice: NU = 15 and 17), 5, 8
    assert sorted(emission_plan(lib, s[2], s[3], s[5], 0)["kq"] for s in DIMENSION_SHAPES if s[6] == 0) == \
        [3, 4, 4, 5, 8]


@pytest.mark.parametrize("name,sw,want", STATS_SWITCH_ROWS,
                         ids=["%s-%s" % (n, "+".join(sw)) for n, sw, _ in STATS_SWITCH_ROWS])
def test_switch_sets_reach_the_other_gated_statistics_kernels(lib, name, sw, want):  # noqa: F811
    p = stats_plan(lib, ROWS[name], no_m=sw.get("NO_STATS_M", 0), no_u=sw.get("NO_STATS_U", 0),
                   no_g=sw.get("NO_STATS_G", 0))
    assert p["name"] == want
    if want == "grouped":
        assert p["LG"] == 32
    assert stats_plan(lib, ROWS[name])["name"] == "mfma"
