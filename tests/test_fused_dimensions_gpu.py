"""The fused E-step at the observation dimensions d <= 16 no other test runs on the device,
against the oracle (cases.DIMENSION_SHAPES; its preconditions are asserted on the oracle and
the planner alone by tests/test_dimension_cases.py, which also computes the references used
here, once per row).

The other parity tests run full covariances at d in {2, 3, 4, 5, 8, 16, 20} and diagonal ones at
{1, 2, 3, 12, 16}.  Here:
a. every row of DIMENSION_SHAPES in the four regimes of test_fused_cluster_counts_gpu (the gated
   schedule at tscale = 100, 1e-9 and 0.03, the dense schedule at 100), a second call on the
   same engine bit-identical to the first: the emission GEMM's k-step counts 7, 9 (12-step
   bucket), 14 .. 34 (the general 40-step instance), 3, 4, 5, 8 (diagonal), and
   stats_list_m_kernel's tile plans (4, 4, 4), (5, 2, 3), (6, 2, 3), (7, 2, 4), (8, 2, 4), (9, 1, 3);
b. the per-pair outputs on the prepared operand, the per-call operand and the raw / generic
   kernels (VBHEM_NO_UGEMM: launch_raw_kq<7> at d = 6 full, <3> at d = 6 diagonal), each against
   the oracle;
c. the gated statistics kernels behind VBHEM_NO_STATS_M / _G / _U where NU crosses their limits
   (32 lanes per pair, 64 moment columns);
d. the VHEM fused E-step (E /= smooth in emission_u_kernel) at full d = 6, 9, 11, 15, 16 and
   diagonal d = 9, smooth = 1 and 2.5, both schedules, against tests/vhem_ref.py.

Bounds: those of test_fused_cluster_counts_gpu.assert_bounds, test_emission_u's per-pair
RTOL_PAIRS and test_vhem_gpu.check_fused, unchanged.  Every test prints its figures before it
asserts (DESIGN.md section 4.14d records them).
"""
import functools

import numpy as np
import pytest
import torch

from cases import lib_switches  # noqa: F401  (a fixture)
from conftest import RTOL_PAIRS, elem_err, stat_err
from test_cluster_count_cases import GATE, TS_ALLPASS, TS_GATED, TS_NONE
from test_dimension_cases import ROWS, STATS_SWITCH_ROWS, row_case, row_reference, stats_plan
from test_emission_u import KEYS, _pairs
from test_fused_cluster_counts_gpu import (DENSE_REFUSAL, REGIMES, assert_bounds, figures, run_fused,
                                           schedule, show)  # noqa: F401  (schedule: a fixture)
from test_gpu_parity import DEV, engine
from test_stats_plan import lib  # noqa: F401  (a fixture: tests/plancheck)
from test_vhem_gpu import build_fused, check_fused_shape, gpu_engine
from test_vhem_gpu import run_fused as run_fused_vhem

pytestmark = pytest.mark.gpu


# ---- a. every row, four regimes -----------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES, ids=[r[0] for r in REGIMES])
@pytest.mark.parametrize("name", list(ROWS))
def test_fused_matches_oracle(vb, vo, lib, schedule, name, regime):  # noqa: F811
    from vbhem_amd import _capi
    regime_id, which, tscale = regime
    _, N, K, S, Sb, d, cov, T, ragged = ROWS[name]
    cs, pairs = row_case(name)
    ref = row_reference(name, tscale)
    tN, logOmega, hz, Z, st = ref
    gated = (Z > GATE).sum(0)
    if tscale == TS_ALLPASS:
        assert (Z > GATE).all() and (Z > GATE).sum() > (row_reference(name, TS_GATED)[3] > GATE).sum()
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
    show(name, regime_id, kernels, "fallback", nfb, "gated", int(gated.sum()), "repeat", same, figs=figs)
    assert nfb == 0
    assert_bounds(figs, (name, regime_id))
    assert same, (name, regime_id)


# ---- b. per-pair outputs of the three emission paths ---------------------------------------------
PAIR_ROWS = ["d6_full", "d6_diag", "d7_full", "d9_full", "d13_full", "d15_full", "d9_diag", "d11_rows"]


@pytest.mark.parametrize("name", PAIR_ROWS)
def test_pairs_of_every_emission_path(vb, vo, name):
    """emission_u_kernel on the prepared operand (shift = the base means' average) and on the
    per-call operand (shift = the cluster means' average), and with VBHEM_NO_UGEMM the kernels
    that build the operand per column tile from the covariances: emission_raw_kernel<KQ> for an
    even d <= 8 (KQ = 7 at d = 6 full, 3 at d = 6 diagonal -- instances nothing else reaches),
    emission_gen_kernel elsewhere.  Every variant against the oracle: L_elbo entry by entry, the
    sums and moments with stat_err, at RTOL_PAIRS."""
    cs, ref = row_case(name)
    variants = [("prepared", dict(prepare=True)), ("per-call", dict(prepare=False)),
                ("NO_UGEMM", dict(prepare=True, old=True))]
    worst = {}
    for label, kw in variants:
        got, eng = _pairs(vb, cs, **kw)
        if label == "prepared":
            assert eng._U is not None  # the prepared path ran
        for k in KEYS + ("sum_t_nu",):
            err = elem_err if k == "LL_elbo" else stat_err
            worst[label, k] = err(got[k], ref[k])
    print("FIGS", name, {label: "%.2e" % max(v for (lb, _), v in worst.items() if lb == label)
                         for label, _ in variants},
          "LL_elbo", {label: "%.2e" % worst[label, "LL_elbo"] for label, _ in variants})
    for (label, k), e in worst.items():
        assert e < RTOL_PAIRS, (name, label, k, e)


# ---- c. the other gated statistics kernels -------------------------------------------------------
@pytest.mark.parametrize("tscale", [TS_GATED, TS_ALLPASS], ids=["Nv100", "allpass"])
@pytest.mark.parametrize("name,sw,want", STATS_SWITCH_ROWS,
                         ids=["%s-%s" % (n, "+".join(sw)) for n, sw, _ in STATS_SWITCH_ROWS])
def test_other_gated_statistics_kernels(vb, vo, lib, schedule, lib_switches, name, sw, want, tscale):  # noqa: F811
    """stats_list_g_kernel with 32 lanes per pair (NU = 28, 31), stats_list_u_kernel at NU = 28,
    36 and 55 (one moment column per lane, the last lanes idle), stats_list_kernel's covariance
    gather just past 64 columns (NU = 66) and at NU = 105: short lists and full ones."""
    _, N, K, S, Sb, d, cov, T, ragged = ROWS[name]
    p = stats_plan(lib, ROWS[name], no_m=sw.get("NO_STATS_M", 0), no_u=sw.get("NO_STATS_U", 0),
                   no_g=sw.get("NO_STATS_G", 0))
    assert p["name"] == want   # the switch set reaches the kernel named
    cs, pairs = row_case(name)
    ref = row_reference(name, tscale)
    schedule("gated")
    lib_switches(**sw)
    eng, _, vec, hatZ, LL = run_fused(vb, cs["base"], cs["consts"], T, ref[1], ref[0])
    figs = figures(vb, vec.cpu().numpy(), hatZ.cpu().numpy(), LL.cpu().numpy(), (K, S, d, cov), ref,
                   pairs["LL_elbo"])
    show(name, "+".join(sw), want, "tscale", tscale, "fallback", eng.fallback_count(), figs=figs)
    assert eng.fallback_count() == 0
    assert_bounds(figs, (name, sw, tscale))


# ---- d. the VHEM fused E-step -----------------------------------------------------------------------
VHEM_N = 131   # chunks of 44 / 44 / 43 bases
# (d, cov) -> the emission GEMM: kq 7 and 5 (12-step bucket), 14 / 20 / 34 (the general 40-step
# instance), 38 (the exact instance; its SM variant at smooth = 2.5)
VHEM_DIMS = [(6, 1), (9, 1), (11, 1), (15, 1), (16, 1), (9, 0)]
VHEM_CASES = {"vhem_d%d_%s_sm%s" % (d, "full" if cov else "diag", smooth): (3, 3, d, cov, True, 5, 4, smooth, "nt")
              for d, cov in VHEM_DIMS for smooth in (1.0, 2.5)}


@functools.lru_cache(maxsize=None)
def vhem_case(name):
    """test_vhem_gpu.fused_case's recipe on VHEM_N bases; the seed from the sorted names."""
    return build_fused(VHEM_CASES[name], 7100 + sorted(VHEM_CASES).index(name), N=VHEM_N)


@pytest.fixture(params=["gated", "dense"])
def vhem_schedule(request, capi_lib):
    from vbhem_amd import _capi
    prev = _capi.set_fused_mode(_capi.FUSED_GATED if request.param == "gated" else _capi.FUSED_DENSE)
    yield request.param
    _capi.set_fused_mode(prev)


@pytest.mark.parametrize("name", sorted(VHEM_CASES))
def test_fused_vhem_matches_restatement(vb, vo, vhem_schedule, name):
    """K = 4, S = Sb = 3 ragged, T = 5, inf_norm 'nt': test_vhem_gpu.check_fused's bars."""
    case = vhem_case(name)
    base, h, opt, es, want = case
    S, Sb, d, cov, ragged, T, K, smooth, norm = VHEM_CASES[name]
    assert opt["smooth"] == smooth and base["prior"].shape[0] == VHEM_N
    vec, Z = run_fused_vhem(vb, gpu_engine(vb, base, K, S, T), base, h, opt)
    check_fused_shape(vb, name + "-" + vhem_schedule, VHEM_CASES[name], case, vec, Z)
