"""The preconditions of tests/test_fused_cluster_counts_gpu.py, on the oracle and the planner
alone (no GPU): the shapes of cases.CLUSTER_COUNT_SHAPES and cases.TRIAL_COUNT_SHAPES put the
fused epilogue where their comments say, so that no GPU test there can pass vacuously.

* tscale = 100 (tilde N = 100 N omega, the configs' virtual samples): some pair of every shape
  passes the gate Z > 1e-8, and at least one cluster of every single-call shape has no gated
  pair at all -- the empty list the gated kernels must handle;
* tscale = 0.03: every pair of every cluster (of every trial) passes; tscale = 1e-9: none does;
* no oracle Z lies within a relative 1e-3 of the gate in any of these regimes (a pair the
  reference gates and the kernel drops would otherwise hide inside the 1e-9 bound's noise);
* the kernel the planner names for every row: resp_kernel<K> at K = 4, 32, 64, resp_kernel<0>
  elsewhere (masked lanes, or the K > 64 loop), resp_trials_kernel with 1, 2, 3 and 4 clusters
  per lane, a refusal at R K = 260; with cases.SHAPES every resp_kernel instance is reached;
* the adversarial cluster of the exact-fallback cases is gated for every base;
* the largest K the responsibilities kernel's LDS admits, and that all its pairs pass at 0.03.

The references are computed once per shape (functools.lru_cache) and never modified: the GPU
module imports them from here.
"""
import ctypes
import functools

import numpy as np
import pytest

import vbhem_oracle as vo
from cases import CLUSTER_COUNT_SHAPES, SHAPES, STATE_COUNT_SHAPES, TRIAL_COUNT_SHAPES, make_case, post_dict
from test_gpu_parity import adversarial_case, seed_of
from test_stats_plan import GATED_KERNELS, RESP_KERNELS, gated_plan, lib  # noqa: F401  (lib: a fixture)
from test_trials import _trial_posts

GATE = 1e-8
GATE_MARGIN = 1e-3
TS_GATED, TS_ALLPASS, TS_NONE = 100.0, 0.03, 1e-9
SINGLE = {s[0]: s for s in CLUSTER_COUNT_SHAPES}
TRIALS = {s[0]: s for s in TRIAL_COUNT_SHAPES}
assert len(SINGLE) == len(CLUSTER_COUNT_SHAPES) and len(TRIALS) == len(TRIAL_COUNT_SHAPES)
KP_ROWS = {"K4_chunks": 4, "K32_chunks": 32, "K64": 64, "K64_one": 64}
# (N, K) of the exact-fallback cases: adversarial_case(1, N=N, K=K), clusters 1.. pushed away
ADVERSARIAL = [(131, 7), (131, 33), (131, 64), (131, 65), (70, 129)]
KMAX_SHAPE = dict(N=5, S=2, Sb=2, d=2, cov=0, T=4)   # the largest accepted K, name "Kmax"


def frozen(*arrays):
    for a in arrays:
        for v in (a.values() if isinstance(a, dict) else [a]):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def single_case(name):
    """(case, the oracle's per-pair outputs) of a CLUSTER_COUNT_SHAPES row."""
    _, N, K, S, Sb, d, cov, T, ragged = SINGLE[name]
    cs = make_case(N, K, S, Sb, d, cov, seed=seed_of(name) + 1, ragged=ragged, tau=T)
    pairs = vo.c_estep_pairs(cs["base"], cs["consts"], T, nthreads=4)
    frozen(pairs)
    return cs, pairs


def reference(cs, pairs, tscale, cov):
    N = cs["base"]["prior"].shape[0]
    tN = tscale * N * cs["base"]["omega"]
    logOmega, hz, Z, _ = vo.responsibilities(pairs["LL_elbo"], tN, cs["post"]["alpha"])
    st = vo.c_statistics(Z, pairs, cov)
    frozen(hz, Z, st)   # (tilde N and logOmega go to the engine, which copies them)
    return tN, logOmega, hz, Z, st


@functools.lru_cache(maxsize=None)
def single_reference(name, tscale):
    """(tilde N, logOmega, hat_Z, Z, statistics) of the oracle at tilde N = tscale N omega."""
    return reference(*single_case(name), tscale, SINGLE[name][6])


@functools.lru_cache(maxsize=None)
def trial_case(name):
    """(case, per trial r: (posterior dict, oracle constants, oracle per-pair outputs))."""
    _, N, K, S, Sb, d, cov, T, ragged, R = TRIALS[name]
    cs = make_case(N, K, S, Sb, d, cov, seed=seed_of(name), ragged=ragged, tau=T)
    trials = []
    for P in _trial_posts(cs, R, seed_of(name)):
        post = post_dict(P)
        consts = vo.prelude(post, cov)
        pairs = vo.c_estep_pairs(cs["base"], consts, T, nthreads=4)
        frozen(pairs)
        trials.append((post, consts, pairs))
    return cs, trials


@functools.lru_cache(maxsize=None)
def trial_reference(name, tscale):
    """Per trial r: (tilde N, logOmega, hat_Z, Z, statistics), the oracle on that trial alone."""
    cs, trials = trial_case(name)
    return [reference(dict(cs, post=post), pairs, tscale, TRIALS[name][6]) for post, _, pairs in trials]


@functools.lru_cache(maxsize=None)
def adversarial_reference(N, K):
    """test_gpu_parity.adversarial_case with every other cluster's emissions pushed far away:
    (case, constants, oracle pairs, (tilde N, logOmega, hat_Z, Z, statistics) at tscale 100)."""
    cs, consts = adversarial_case(1, N=N, K=K)
    consts["c"][1:] = 1.0e4
    pairs = vo.c_estep_pairs(cs["base"], consts, cs["T"], nthreads=4)
    frozen(pairs)
    return cs, consts, pairs, reference(cs, pairs, TS_GATED, 1)


@functools.lru_cache(maxsize=None)
def kmax_reference(K):
    """The KMAX_SHAPE case of K clusters at tscale = 0.03 (seed as a shape named "Kmax")."""
    s = KMAX_SHAPE
    cs = make_case(s["N"], K, s["S"], s["Sb"], s["d"], s["cov"], seed=seed_of("Kmax") + 1, tau=s["T"])
    pairs = vo.c_estep_pairs(cs["base"], cs["consts"], s["T"], nthreads=4)
    frozen(pairs)
    return cs, pairs, reference(cs, pairs, TS_ALLPASS, s["cov"])


def gate_margin(Z):
    """the closest any Z comes to the gate, relative to it"""
    return float(np.abs(np.asarray(Z) / GATE - 1.0).min())


# ---- the planner (tests/plancheck) ------------------------------------------------------
def resp_plan(lib, K, KT, S=4, SB=4, fold=0, generic=0):  # noqa: F811
    """(ok, kernel name, KP, lds, gate_list_lds) of plan_resp for a VBHEM call."""
    out = np.zeros(5, dtype=np.int64)
    lib.plancheck_resp(K, KT, S, SB, 0, fold, generic, out.ctypes.data)
    ok, kernel, KP, lds, gate_lds = out.tolist()
    name = {"vhem": "vhem_resp_kernel", "trials": "resp_trials_kernel", "kp": "resp_kernel<%d>" % KP,
            "generic": "resp_kernel<0>"}[RESP_KERNELS[kernel]]
    return bool(ok), name, KP, lds, gate_lds


def lds_limit(lib):  # noqa: F811
    lib.plancheck_lds_limit.restype = ctypes.c_longlong
    lib.plancheck_lds_limit.argtypes = []
    return int(lib.plancheck_lds_limit())


def largest_k(lib):  # noqa: F811
    """The largest K whose resp_lds(K, K) fits the LDS limit (estep_fused_checked's check)."""
    limit = lds_limit(lib)
    fits = lambda K: resp_plan(lib, K, K)[3] <= limit  # noqa: E731
    lo, hi = 64, 1 << 16   # resp_lds grows with K from 64 on (one base per wave step)
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def group_lanes(K):
    G = 1
    while G < K and G < 64:
        G <<= 1
    return G


# ---- the gate regimes ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SINGLE))
def test_single_call_gate_regimes(name):
    _, N, K = SINGLE[name][:3]
    Z100, Zall, Znone = (single_reference(name, ts)[3] for ts in (TS_GATED, TS_ALLPASS, TS_NONE))
    gated = (Z100 > GATE).sum(0)
    margins = [gate_margin(Z) for Z in (Z100, Zall, Znone)]
    print("CASE", name, "gated pairs", int(gated.sum()), "empty clusters", int((gated == 0).sum()),
          "gate margins", ["%.1e" % m for m in margins])
    assert Z100.shape == (N, K) and np.isfinite(single_case(name)[1]["LL_elbo"]).all()
    assert gated.sum() >= 1
    assert (gated == 0).sum() >= 1        # an empty list
    assert (Zall > GATE).all()            # every list full
    assert not (Znone > GATE).any()       # every list empty
    assert min(margins) > GATE_MARGIN


@pytest.mark.parametrize("name", list(TRIALS))
def test_trial_gate_regimes(name):
    _, N, K, S, Sb, d, cov, T, ragged, R = TRIALS[name]
    refs100, refsall = trial_reference(name, TS_GATED), trial_reference(name, TS_ALLPASS)
    assert len(refs100) == R
    gated = sum(int((r[3] > GATE).sum()) for r in refs100)
    margins = [gate_margin(r[3]) for r in refs100 + refsall]
    print("CASE", name, "gated pairs", gated, "gate margin %.1e" % min(margins))
    assert gated >= 1
    for r in refsall:
        assert r[3].shape == (N, K) and (r[3] > GATE).all()
    assert min(margins) > GATE_MARGIN
    # the trials differ: no two share their responsibilities (R K_trial distinct clusters)
    if K > 1:
        hz = [r[2] for r in refsall]
        assert all(not np.array_equal(hz[0], h) for h in hz[1:])


@pytest.mark.parametrize("N,K", ADVERSARIAL)
def test_adversarial_cluster_is_gated_for_every_base(N, K):
    cs, consts, pairs, (tN, logOmega, hz, Z, st) = adversarial_reference(N, K)
    assert Z.shape == (N, K) and np.isfinite(pairs["LL_elbo"]).all()
    assert (Z[:, 0] > GATE).all()
    assert gate_margin(Z) > GATE_MARGIN


# ---- the planner's buckets ----------------------------------------------------------------
def test_single_call_rows_reach_their_resp_kernels(lib):  # noqa: F811
    limit = lds_limit(lib)
    instances = set()
    for name, (_, N, K, S, Sb, *_rest) in SINGLE.items():
        for fold in (0, 1):
            ok, kernel, KP, lds, gate_lds = resp_plan(lib, K, K, S, Sb, fold=fold)
            assert ok and lds <= limit and gate_lds <= limit, name
            assert kernel == "resp_kernel<%d>" % KP_ROWS.get(name, 0), (name, kernel)
        instances.add(KP)
        # the generic kernel is what VBHEM_RESP_GENERIC puts the K = 4, 32, 64 rows on
        assert resp_plan(lib, K, K, S, Sb, generic=1)[1] == "resp_kernel<0>"
    assert instances == {0, 4, 32, 64}
    # every instance runs under the oracle somewhere: 8 and 16 on cases.SHAPES
    for _, N, K, S, Sb, *_rest in SHAPES + STATE_COUNT_SHAPES:
        instances.add(resp_plan(lib, K, K, S, Sb)[2])
    assert instances == {0, 4, 8, 16, 32, 64}
    # resp_kernel<0>'s branches: G = 8, 16, 32, 64 lanes per base with masked lanes (K < G),
    # and the loop with 2 to 5 clusters in a lane (K > 64); under VBHEM_RESP_GENERIC K = G too
    generic = [s[2] for n, s in SINGLE.items() if n not in KP_ROWS]
    assert {group_lanes(K) for K in generic if K < group_lanes(K)} == {8, 16, 32, 64}
    assert {-(-K // 64) for K in generic if K > 64} == {2, 3, 5}
    assert {65, 129, 257} <= set(generic)
    # more than one chunk (64 bases at least each), and one short chunk at K = 64
    assert all(SINGLE[n][1] > 64 for n in KP_ROWS if n != "K64_one") and SINGLE["K64_one"][1] < 64
    # the dense schedule's row groups: several at the larger K
    dense = np.zeros(11, dtype=np.int64)
    ngroups = {}
    for name, (_, N, K, S, Sb, d, cov, *_rest) in SINGLE.items():
        lib.plancheck_stats_dense(K, S, Sb, d, cov, dense.ctypes.data)
        ngroups[name] = int(dense[1]) if dense[0] else 0
    assert ngroups["K257"] > 1 and ngroups["K65_S5"] > 1 and ngroups["K33_S8"] > 1
    assert all(ngroups.values())   # (no row whose dense plan is refused)


@pytest.mark.parametrize("name", ["K33", "K65_S5"])
def test_switch_sets_reach_the_other_gated_statistics_kernels(lib, name):  # noqa: F811
    """On a prepared base set the MFMA kernel sums the gated statistics; the switch sets of the
    GPU module's test put these two shapes on each of the other three kernels."""
    _, N, K, S, Sb, d, cov, T, ragged = SINGLE[name]
    nchunk = -(-N // 64)

    def kernel(no_m=0, no_u=0, no_g=0):
        p = gated_plan(lib, ("gated", K, S, Sb, d, cov, 2, nchunk, N, 256, 1, nchunk, no_m, no_u, no_g, -1))
        assert p["ok"]
        return GATED_KERNELS[p["kernel"]]

    assert [kernel(), kernel(no_m=1), kernel(no_m=1, no_g=1), kernel(no_u=1)] == \
        ["mfma", "grouped", "operand", "gather"]


def test_trial_rows_reach_the_trials_kernel(lib):  # noqa: F811
    limit = lds_limit(lib)
    slots = set()
    for name, (_, N, K, S, Sb, d, cov, T, ragged, R) in TRIALS.items():
        ok, kernel, KP, lds, gate_lds = resp_plan(lib, R * K, K, S, Sb)
        assert ok and kernel == "resp_trials_kernel" and lds <= limit and gate_lds <= limit, name
        assert R * K <= 256 and R > 1
        slots.add(-(-R * K // 64))
    assert slots == {1, 2, 3, 4}   # clusters per lane (kRespSlots = 4)
    totals = {s[2] * s[9] for s in TRIAL_COUNT_SHAPES}
    assert {15, 27, 65, 66, 130, 195, 255, 256} <= totals
    ok, kernel, *_ = resp_plan(lib, 260, 65)
    assert not ok and kernel == "resp_trials_kernel"   # refused: past 4 slots of 64 lanes


def test_largest_cluster_count(lib):  # noqa: F811
    """The largest K of estep_fused_checked's LDS check, the gated schedule still planned for
    it, and every pair of the KMAX_SHAPE case passing the gate at tscale = 0.03."""
    limit, K = lds_limit(lib), largest_k(lib)
    print("CASE Kmax", K, "resp_lds", resp_plan(lib, K, K)[3], "limit", limit)
    assert resp_plan(lib, K, K)[3] <= limit < resp_plan(lib, K + 1, K + 1)[3]
    s = KMAX_SHAPE
    ok, kernel, KP, lds, gate_lds = resp_plan(lib, K + 1, K + 1, s["S"], s["Sb"])
    assert kernel == "resp_kernel<0>" and gate_lds <= limit
    # the recursion kernels' plan (plan_split: one lane per column at S = 2) and its list mode
    lib.plancheck_split.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p]
    lib.plancheck_split.restype = None
    split = np.zeros(19, dtype=np.int64)
    for k in (K, K + 1):
        lib.plancheck_split(s["Sb"], s["d"], s["cov"], k, s["S"], s["T"], 1, split.ctypes.data)
        assert split[0] == 1 and split[11] > 0, split
    cs, pairs, (tN, logOmega, hz, Z, st) = kmax_reference(K)
    assert Z.shape == (s["N"], K) and (Z > GATE).all() and gate_margin(Z) > GATE_MARGIN
