"""The fused VBHEM E-step across the cluster-count buckets of its epilogue, against the oracle
(cases.CLUSTER_COUNT_SHAPES, cases.TRIAL_COUNT_SHAPES; their preconditions are asserted on the
oracle and the planner alone by tests/test_cluster_count_cases.py, which also computes the
references used here, once per shape).

The other single-call parity tests use K in {1..6, 8, 16, 32}.  Here:
a. every row of CLUSTER_COUNT_SHAPES in four regimes -- the gated schedule at tscale = 100
   (short lists, some empty), 1e-9 (every list empty) and 0.03 (every list full), the dense
   schedule at 100 -- with a second call on the same engine bit-identical to the first;
b. resp_kernel<K> (K = 4, 32, 64) against resp_kernel<0> (VBHEM_RESP_GENERIC): bit-identical;
c. the gated statistics kernels behind VBHEM_NO_STATS_M / _G / _U at K = 33 and 65;
d. the exact fallback (folded into resp_kernel: `mine = pair / K`, or launched) at K = 7 .. 129;
e. batched trials, each trial against the oracle run on that trial's own posterior;
f. the largest K the library accepts, and the refusal one past it.

Bounds: test_gpu_parity.test_fused_matches_oracle's -- stat_err < 1e-9 for Nj, N1, M, Nr, Y, SC,
Lt1 within 1e-10 relative, Lt7 within 1e-9 relative + 1e-9, hatz_err < RTOL_NORTH_STAR,
elem_err(L_elbo) < RTOL_PAIRS (1e-9 for a trial's columns: the emission GEMM shifts the means
by the average over all R K clusters).  Every test prints its figures before it asserts
(DESIGN.md section 4.14c records them).
"""
import numpy as np
import pytest
import torch

from cases import lib_switches  # noqa: F401  (a fixture)
from conftest import RTOL_NORTH_STAR, RTOL_PAIRS, elem_err, hatz_err, stat_err
from test_cluster_count_cases import (ADVERSARIAL, GATE, KMAX_SHAPE, KP_ROWS, SINGLE, TRIALS, TS_ALLPASS,
                                      TS_GATED, TS_NONE, adversarial_reference, kmax_reference,
                                      largest_k, single_case, single_reference, trial_case,
                                      trial_reference)
from test_gpu_parity import DEV, engine
from test_stats_plan import lib  # noqa: F401  (a fixture: tests/plancheck)

pytestmark = pytest.mark.gpu

STAT_KEYS = ("Nj", "N1", "M", "Nr", "Y", "SC")
# (id, schedule, tscale)
REGIMES = [("gated-Nv100", "gated", TS_GATED), ("dense-Nv100", "dense", TS_GATED),
           ("gated-allgated", "gated", TS_NONE), ("gated-allpass", "gated", TS_ALLPASS)]
DENSE_REFUSAL = "statistics tile does not fit"


@pytest.fixture
def schedule(lib_switches):  # noqa: F811
    """``schedule("dense")`` / ``schedule("gated")``: the fused schedule for the rest of the test."""
    return lambda which: lib_switches(FUSED_DENSE=int(which == "dense"))


def figures(vb, vec, hatZ, LL, dims, ref, LL_ref):
    """The parity figures of one statistics vector (section), hat_Z and L_elbo block against
    the oracle's (tilde N, logOmega, hat_Z, Z, statistics)."""
    K, S, d, cov = dims
    tN, logOmega, hz, Z, st = ref
    got = vb.host.unpack_stats(vec, K, S, d, cov)
    figs = {k: stat_err(got[k], st[k]) for k in STAT_KEYS}
    Lt1 = float((Z * LL_ref).sum())
    Lt7 = float((hz * np.log(hz)).sum())
    figs["Lt1"] = abs(got["Lt1"] - Lt1) / abs(Lt1)
    figs["Lt7"] = abs(got["Lt7"] - Lt7) / (1e-9 * abs(Lt7) + 1e-9)   # in units of its bound
    figs["hatZ"] = hatz_err(hatZ, hz)
    figs["LL"] = elem_err(LL, LL_ref)
    figs["finite"] = float(np.isfinite(vec).all())
    return figs


def assert_bounds(figs, what, ll_bound=RTOL_PAIRS):
    assert figs["finite"] == 1.0, what
    for k in STAT_KEYS:
        assert figs[k] < 1e-9, (what, k, figs[k])
    assert figs["Lt1"] <= 1e-10, (what, figs["Lt1"])
    assert figs["Lt7"] <= 1.0, (what, figs["Lt7"])
    assert figs["hatZ"] < RTOL_NORTH_STAR, (what, figs["hatZ"])
    assert figs["LL"] < ll_bound, (what, figs["LL"])


def show(*head, figs):
    print("FIGS", *head, {k: "%.2e" % v for k, v in figs.items() if k != "finite"})


def run_fused(vb, base, consts, T, logOmega, tN):
    """One engine, one fused call: (engine, tilde N on the device, statistics, hat_Z, L_elbo)."""
    eng = engine(vb, base, consts, T)
    eng.set_log_omega(logOmega)
    tN_dev = torch.as_tensor(tN, device=DEV)
    vec = eng.fused(tN_dev).clone()
    return eng, tN_dev, vec, eng.hatZ.clone(), eng.LL.clone()


def dims_of(shape):
    return shape[2], shape[3], shape[5], shape[6]


# ---- a. single calls ------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES, ids=[r[0] for r in REGIMES])
@pytest.mark.parametrize("name", list(SINGLE))
def test_fused_matches_oracle(vb, vo, lib, schedule, name, regime):  # noqa: F811
    from vbhem_amd import _capi
    regime_id, which, tscale = regime
    _, N, K, S, Sb, d, cov, T, ragged = SINGLE[name]
    cs, pairs = single_case(name)
    ref = single_reference(name, tscale)
    tN, logOmega, hz, Z, st = ref
    gated = (Z > GATE).sum(0)
    if tscale == TS_ALLPASS:   # (asserted on the oracle here as in test_gpu_parity)
        assert (Z > GATE).all() and (Z > GATE).sum() > (single_reference(name, TS_GATED)[3] > GATE).sum()
    elif tscale == TS_NONE:
        assert not gated.any()
    schedule(which)
    if which == "dense":
        plan = np.zeros(11, dtype=np.int64)
        lib.plancheck_stats_dense(K, S, Sb, d, cov, plan.ctypes.data)
        if not plan[0]:   # the dense plan does not fit this shape: the library must say so
            eng = engine(vb, cs["base"], cs["consts"], T)
            eng.set_log_omega(logOmega)
            with pytest.raises(_capi.VbhemError, match=r"status -2.*" + DENSE_REFUSAL):
                eng.fused(torch.as_tensor(tN, device=DEV))
            return
    eng, tN_dev, vec, hatZ, LL = run_fused(vb, cs["base"], cs["consts"], T, logOmega, tN)
    kernels, nfb = (_capi.last_kernel(0), _capi.last_kernel(1)), eng.fallback_count()
    again = eng.fused(tN_dev)
    same = torch.equal(again, vec) and torch.equal(eng.hatZ, hatZ) and torch.equal(eng.LL, LL)
    figs = figures(vb, vec.cpu().numpy(), hatZ.cpu().numpy(), LL.cpu().numpy(), (K, S, d, cov), ref,
                   pairs["LL_elbo"])
    show(name, regime_id, kernels, "fallback", nfb, "gated", int(gated.sum()), "empty",
         int((gated == 0).sum()), "repeat", same, figs=figs)
    assert nfb == 0
    assert_bounds(figs, (name, regime_id))
    assert same, (name, regime_id)


# ---- b. the K-templated path against the generic one -------------------------------------------
@pytest.mark.parametrize("tscale", [TS_GATED, TS_ALLPASS], ids=["Nv100", "allpass"])
@pytest.mark.parametrize("name", list(KP_ROWS))
def test_templated_path_bit_identical_to_generic(vb, vo, schedule, name, tscale):
    """resp_kernel<K> (buffer stores, unrolled group reductions, two pipelined steps) and
    resp_kernel<0> at K = G add the same terms in the same order: statistics, hat_Z and L_elbo
    are torch.equal with VBHEM_RESP_GENERIC on and off -- over three chunks, and at K64_one
    over one chunk of 9 bases, whose second pipelined step lies wholly past the end.  The
    generic run is held to the oracle as well (resp_kernel<0> with every lane of a group in
    use)."""
    from vbhem_amd import _capi
    _, N, K, S, Sb, d, cov, T, ragged = SINGLE[name]
    cs, pairs = single_case(name)
    ref = single_reference(name, tscale)
    schedule("gated")
    outs = []
    for generic in (0, 1):
        with _capi.switches(RESP_GENERIC=generic):
            eng, _, vec, hatZ, LL = run_fused(vb, cs["base"], cs["consts"], T, ref[1], ref[0])
        outs.append((vec, hatZ, LL))
        del eng
    same = [torch.equal(a, b) for a, b in zip(*outs)]
    vec, hatZ, LL = outs[1]
    figs = figures(vb, vec.cpu().numpy(), hatZ.cpu().numpy(), LL.cpu().numpy(), (K, S, d, cov), ref,
                   pairs["LL_elbo"])
    show(name, "generic", "tscale", tscale, "bit-identical (stats, hatZ, LL)", same, figs=figs)
    assert_bounds(figs, (name, "generic"))
    assert all(same), (name, same)


# ---- c. the other gated statistics kernels -------------------------------------------------------
@pytest.mark.parametrize("sw", [dict(NO_STATS_M=1), dict(NO_STATS_M=1, NO_STATS_G=1), dict(NO_STATS_U=1)],
                         ids=["NO_STATS_M", "NO_STATS_M+NO_STATS_G", "NO_STATS_U"])
@pytest.mark.parametrize("name", ["K33", "K65_S5"])
def test_other_gated_statistics_kernels(vb, vo, schedule, lib_switches, name, sw):  # noqa: F811
    """stats_list_g_kernel, stats_list_u_kernel and stats_list_kernel (grid y = cluster) at an
    odd K past 32 and past 64, tscale = 100: lists of 0 to a few dozen pairs."""
    _, N, K, S, Sb, d, cov, T, ragged = SINGLE[name]
    cs, pairs = single_case(name)
    ref = single_reference(name, TS_GATED)
    schedule("gated")
    lib_switches(**sw)
    eng, _, vec, hatZ, LL = run_fused(vb, cs["base"], cs["consts"], T, ref[1], ref[0])
    figs = figures(vb, vec.cpu().numpy(), hatZ.cpu().numpy(), LL.cpu().numpy(), (K, S, d, cov), ref,
                   pairs["LL_elbo"])
    show(name, "+".join(sw), "fallback", eng.fallback_count(), figs=figs)
    assert eng.fallback_count() == 0
    assert_bounds(figs, (name, sw))


# ---- d. the exact fallback ----------------------------------------------------------------------
@pytest.mark.parametrize("sw", [{}, dict(NO_FOLD_EXACT=1)], ids=["fold", "NO_FOLD_EXACT"])
@pytest.mark.parametrize("N,K", ADVERSARIAL)
def test_exact_fallback_at_larger_k(vb, vo, schedule, lib_switches, N, K, sw):  # noqa: F811
    """test_gpu_parity.test_exact_fallback_gated_pairs past K = 2: cluster 0 underflows for every
    base and wins it, so both passes flag its N pairs.  Folded into resp_kernel, a chunk block
    takes the flagged pairs whose base pair / K is its own -- masked lanes at K = 7, 33, one
    cluster per lane at 64, the K > 64 loop at 65, 129; VBHEM_NO_FOLD_EXACT: fb_exact_kernel
    launches instead."""
    cs, consts, pairs, ref = adversarial_reference(N, K)
    tN, logOmega, hz, Z, st = ref
    S, d = consts["logPi"].shape[1], cs["base"]["centres"].shape[2]
    assert (Z[:, 0] > GATE).all()   # the flagged cluster is gated for every base
    schedule("gated")
    lib_switches(**sw)
    eng, _, vec, hatZ, LL = run_fused(vb, cs["base"], consts, cs["T"], logOmega, tN)
    nfb = eng.fallback_count()
    figs = figures(vb, vec.cpu().numpy(), hatZ.cpu().numpy(), LL.cpu().numpy(), (K, S, d, 1), ref,
                   pairs["LL_elbo"])
    show("adversarial", N, K, "+".join(sw) or "fold", "fallback", nfb, figs=figs)
    assert nfb >= 2 * N
    assert figs["finite"] == 1.0
    for k in STAT_KEYS:
        assert figs[k] < 1e-9, (K, k, figs[k])
    assert figs["LL"] < RTOL_PAIRS
    assert figs["hatZ"] < RTOL_NORTH_STAR


# ---- e. batched trials ----------------------------------------------------------------------------
@pytest.mark.parametrize("tscale", [TS_GATED, TS_ALLPASS], ids=["Nv100", "allpass"])
@pytest.mark.parametrize("name", list(TRIALS))
def test_trials_match_oracle(vb, vo, schedule, name, tscale):
    """One vbhem_estep_fused_trials call over R K_trial clusters; trial r's section of the
    statistics, its columns of hat_Z and of L_elbo against the oracle run on trial r's own
    posterior (never against a single GPU call).  L_elbo elementwise within 1e-9: the emission
    GEMM's mean shift is the average over all R K_trial cluster means."""
    from vbhem_amd import host
    from vbhem_amd.em import _stack_constants
    from vbhem_amd.estep import EStepEngine
    _, N, K, S, Sb, d, cov, T, ragged, R = TRIALS[name]
    cs, trials = trial_case(name)
    refs = trial_reference(name, tscale)
    tN = refs[0][0]
    schedule("gated")
    eng = EStepEngine(vb.BaseSet.from_numpy(cs["base"]), R * K, S, T, device=DEV, trials=R)
    eng.set_clusters(_stack_constants([consts for _, consts, _ in trials]))
    eng.set_log_omega(np.concatenate([r[1] for r in refs]))
    vec = eng.fused(torch.as_tensor(tN, device=DEV)).cpu().numpy()
    hatZ, LL, nfb = eng.hatZ.cpu().numpy(), eng.LL.cpu().numpy(), eng.fallback_count()
    SL = host.stats_len(K, S, d, cov)
    assert vec.size == R * SL
    worst = {}
    for r in range(R):
        cols = slice(r * K, (r + 1) * K)
        f = figures(vb, vec[r * SL:(r + 1) * SL], hatZ[:, cols], LL[:, cols], (K, S, d, cov), refs[r],
                    trials[r][2]["LL_elbo"])
        worst = {k: max(v, worst.get(k, 0.0)) if k != "finite" else min(v, worst.get(k, 1.0))
                 for k, v in f.items()}
    show(name, "tscale", tscale, "trials", R, "fallback", nfb, "gated",
         sum(int((r[3] > GATE).sum()) for r in refs), figs=worst)
    assert nfb == 0
    assert_bounds(worst, name, ll_bound=1e-9)
    if K == 1:   # a trial of one cluster: hat_Z = 1 + 1e-50 = 1 exactly, Nj = sum tilde N
        assert (hatZ == 1.0).all()
        Nj = np.array([host.unpack_stats(vec[r * SL:(r + 1) * SL], K, S, d, cov)["Nj"][0] for r in range(R)])
        print("FIGS", name, "Nj vs sum tilde N", float(np.abs(Nj / tN.sum() - 1.0).max()))
        assert np.abs(Nj - tN.sum()).max() <= 1e-12 * tN.sum()


# ---- f. the largest accepted K ---------------------------------------------------------------------
def test_largest_cluster_count(vb, vo, lib, schedule):  # noqa: F811
    """K = the largest whose resp_lds(K, K) fits the LDS limit (found through tests/plancheck;
    2,407 by the formula): N = 5 bases, every one of the 5 K pairs gated (tscale = 0.03), so
    gate_list_kernel runs ten rounds of its j0 loop and every cluster's list holds 5 pairs.  The
    binding limit is that of estep_fused_checked: resp_kernel's per-wave Nj accumulators of all
    K clusters in LDS; the gate lists' ballot masks and the recursion kernels still fit there
    (asserted by test_cluster_count_cases.test_largest_cluster_count).  K + 1 is refused with
    VBHEM_ERR_UNSUPPORTED, the error is consumed, and the next call on the first engine gives
    the bits it gave before."""
    from vbhem_amd import _capi
    K = largest_k(lib)
    s = KMAX_SHAPE
    cs, pairs, ref = kmax_reference(K)
    tN, logOmega, hz, Z, st = ref
    assert (Z > GATE).all() and Z.size == s["N"] * K
    schedule("gated")
    eng, tN_dev, vec, hatZ, LL = run_fused(vb, cs["base"], cs["consts"], s["T"], logOmega, tN)
    kernels, nfb = (_capi.last_kernel(0), _capi.last_kernel(1)), eng.fallback_count()
    figs = figures(vb, vec.cpu().numpy(), hatZ.cpu().numpy(), LL.cpu().numpy(),
                   (K, s["S"], s["d"], s["cov"]), ref, pairs["LL_elbo"])
    show("Kmax", K, kernels, "fallback", nfb, figs=figs)
    assert nfb == 0
    assert_bounds(figs, ("Kmax", K))
    # one cluster more: refused before any launch
    one_more = {k: np.concatenate([v, v[:1]], axis=0) for k, v in cs["consts"].items()
                if k in ("logA", "logPi", "m", "P", "c")}
    big = engine(vb, cs["base"], one_more, s["T"])
    big.set_log_omega(np.concatenate([logOmega, logOmega[:1]]))
    with pytest.raises(_capi.VbhemError, match=r"status -2.*too many clusters"):
        big.fused(tN_dev)
    again = eng.fused(tN_dev)
    torch.cuda.synchronize()
    assert torch.equal(again, vec) and torch.equal(eng.hatZ, hatZ) and torch.equal(eng.LL, LL)
