"""The run routines of the batched VB-HMM EM (csrc/vbhmm_em_run.h) on the host: the
serial walker of tests/vbhmmemcheck against oracle/vbhmm_em_oracle.em(fb_fn='c'), which
restates vbhmm_em.m + vbhmm_em_lb.m loop for loop.  Inputs (a) .. (e) and the
iteration-count condition are described in tests/vbhmm_em_batch_ref.py; the cases of (d)
and (e), the corners of the kernels' buckets, are compared with no run left out.  Tolerances are
the project's: rtol 1e-9 on bound trajectories and post_err < 1e-8 on posteriors
(tests/test_vbhmm_em.py), stat_err < 1e-10 on statistics (RTOL_PAIRS).
"""
import numpy as np
import pytest

import vbhmm_em_batch_ref as R
import vbhmm_em_oracle as vho
from conftest import RTOL_PAIRS, post_err, stat_err


def _input(name):
    if name == "a":
        return R.runs_a() + (R.options(),)
    if name == "b":
        return R.runs_b() + (R.options(),)
    if name == "c3":
        return R.runs_c(3) + (R.options(3),)
    return R.corner_input(name)


CORNERS = R.NAMES_D + R.NAMES_E


@pytest.mark.parametrize("name", ["a", "b", "c3"] + CORNERS)
def test_host_walker_matches_oracle(vb, vo, name):
    subj, runs, opt = _input(name)
    ref = R.oracle_runs(name, subj, runs, opt)
    got = R.run_check(subj, runs, opt, "host")
    excluded = R.compare_with_oracle(got, ref, opt, post_err, name)
    if name in CORNERS:
        assert not any(R.near_threshold(r["LLs"], opt["minDiff"]) for r in ref), name
        assert excluded == 0, name
    # the posterior at the last E-step: the oracle stopped one M-step earlier
    # (a): every ninth run (each (K, trial) pattern once); (b): one run per K; (c): all
    step = {"a": 9, "b": 3}.get(name, 1)
    for i in range(0, len(runs), step):
        if got[i]["iters"] != ref[i]["iters"]:
            continue
        s, K, g = runs[i]
        est = R.oracle_estep_posterior(subj[s], K, opt, g, ref[i]["iters"])
        for k in R.POST_KEYS:
            assert post_err(got[i]["varpar_estep"][k], est[k]) < 1e-8, (name, i, k)


@pytest.mark.parametrize("name", ["a", "b", "c3"] + CORNERS)
def test_first_iteration_statistics(vb, vo, name):
    subj, runs, opt = _input(name)
    pick = list(range(0, len(runs), 9)) if name == "a" else list(range(len(runs)))
    sel = [runs[i] for i in pick]
    got = R.run_check(subj, sel, opt, "host", max_iter=1)
    for g, (s, K, gmm) in zip(got, sel):
        ref = R.oracle_first_iteration(subj[s], K, opt, gmm)
        assert g["iters"] == 1 and g["status"] == 1
        for k in ("Nk1", "Nk", "M", "xbar", "t1_S"):
            assert stat_err(g[k], ref[k]) < RTOL_PAIRS, (name, s, K, k)
        assert abs(g["LLs"][0] - ref["L"]) <= RTOL_PAIRS * abs(ref["L"]), (name, s, K)
    if name == "d8x1":       # the run with a far component: its state is empty
        assert 1e-50 <= got[3]["Nk1"][0] <= got[3]["Nk"][0] < 1e-40


def test_empty_sequences_change_no_bit(vb):
    """A subject with empty sequences (first, last, two adjacent) gives the bits of the
    same subject without them."""
    subj, runs, opt = R.corner_input("e0")
    assert [n for n, a in enumerate(subj[0]) if a.shape[0] == 0] == list(R.EMPTY_AT)
    dense = R.without_empty(subj)
    assert len(dense[0]) == len(subj[0]) - len(R.EMPTY_AT)
    a = R.run_check(subj, runs, opt, "host")
    b = R.run_check(dense, runs, opt, "host")
    for i, (x, y) in enumerate(zip(a, b)):
        assert R.same_bits(x, y), i


def test_unstable_run_is_contained(vb):
    R.check_unstable("host")


def _loop_state(subj_data, K, opt, varpar):
    """The E-step state of the loop engine (vbhmm_em.vbhmm_em's statistics, statement by
    statement) at a posterior, with the C forward-backward instead of the GPU's."""
    import vbhem_oracle as vo
    dim = len(opt["mu0"])
    data = [np.asarray(a, dtype=np.float64).reshape(-1, dim) for a in subj_data]
    lens = np.array([a.shape[0] for a in data])
    pre = vo.vbhmm_prelude(varpar)
    f = vo.c_vbhmm_fb(data, varpar, pre)
    fb = dict(gamma_all=f["gamma"].transpose(2, 1, 0), logrho_Saved=f["logrho"].transpose(2, 1, 0),
              xi_sum=f["xi_sum"].transpose(1, 2, 0), phi_norm=f["phi_norm"],
              logLambdaTilde=pre["logLambdaTilde"], logPiTilde=pre["logPiTilde"], logATilde=pre["logATilde"])
    g_all = fb["gamma_all"]
    X = np.concatenate(data, axis=0)
    n_idx = np.repeat(np.arange(len(data)), lens)
    t_idx = np.concatenate([np.arange(n) for n in lens])
    Nk = g_all.sum(axis=(1, 2)) + 1e-50
    G = g_all[:, n_idx, t_idx]
    xbar = (G @ X) / Nk[:, None]
    t1_S = np.zeros((K, dim, dim))
    for k in range(K):
        d1 = X - xbar[k]
        t1_S[k] = (d1 * G[k][:, None]).T @ d1 / Nk[k]
    W0 = np.asarray(opt["W0"], dtype=np.float64)
    W0inv = np.linalg.inv(float(W0) * np.eye(dim) if W0.size == 1 else np.diag(W0.reshape(-1)))
    st = dict(dim=dim, K=K, N=len(data), W0inv=W0inv, W0mode="iid" if W0.size == 1 else "diag", t1_S=t1_S,
              xbar=xbar, Nk=Nk, M=fb["xi_sum"].sum(2))
    return st, fb


@pytest.mark.parametrize("W0", [0.001, [0.001, 0.002]])
def test_derivative_helper_is_the_bounds_derivative_block(vb, vo, W0):
    from vbhem_amd.vbhmm_em import vbhmm_clip_hyps, vbhmm_em_lb, vbhmm_em_lb_derivs
    subj, runs = R.runs_a()
    opt, clipped = vbhmm_clip_hyps(R.options(W0=W0))
    s, K, gmm = [r for r in runs if r[1] == 3][2]
    ref = vho.em(subj[s], K, opt, gmm, fb_fn="c")
    vp = R.oracle_estep_posterior(subj[s], K, opt, gmm, ref["iters"])
    st, fb = _loop_state(subj[s], K, opt, vp)
    LB, dLB = vbhmm_em_lb(st, opt, vp, fb, do_deriv=True, clipped=clipped)
    pre = {k: fb[k] for k in ("logLambdaTilde", "logPiTilde", "logATilde")}
    got = vbhmm_em_lb_derivs(dict(dim=st["dim"], K=K, W0inv=st["W0inv"], W0mode=st["W0mode"]), opt, vp, pre, clipped)
    assert set(got) == set(dLB)
    for k in dLB:
        assert np.array_equal(np.asarray(got[k]), np.asarray(dLB[k])), k
    # the bound itself: the same bits with and without the derivatives, and the oracle's value
    assert vbhmm_em_lb(st, opt, vp, fb) == LB
    assert abs(LB - ref["LLs"][-1]) <= 1e-9 * abs(LB)


def test_bound_value_unchanged_by_the_refactor(vb, vo):
    """vbhmm_em_lb on a fixed state: the statement-by-statement bound of the oracle to
    1e-12 (it was 1e-12 before the derivative block moved out), and a clipped
    hyperparameter still zeroes its derivative where moving on would raise the bound."""
    from vbhem_amd.vbhmm_em import vbhmm_clip_hyps, vbhmm_em_lb
    subj, runs = R.runs_a()
    base = R.options()
    s, K, gmm = [r for r in runs if r[1] == 2][1]
    mix = vho.init_from_gmm(subj[s], K, base, gmm)
    vp = dict(alpha=mix["alpha"], epsilon=mix["epsilon"], beta=mix["beta"], v=mix["v"], m=mix["m"].T.copy(),
              W=mix["W"].transpose(2, 0, 1).copy())
    st, fb = _loop_state(subj[s], K, base, vp)
    first = vho.em(subj[s], K, dict(base, maxIter=1), gmm, fb_fn="c")["LLs"][0]
    LB = vbhmm_em_lb(st, base, vp, fb)
    assert abs(LB - first) <= 1e-12 * abs(first)
    hi = dict(base, alpha0=base["hyps_max"]["alpha0"] * 2)
    opt, clipped = vbhmm_clip_hyps(hi)
    assert clipped["alpha0"][0] == 1
    _, d = vbhmm_em_lb(st, opt, vp, fb, do_deriv=True, clipped=clipped)
    _, d_free = vbhmm_em_lb(st, opt, vp, fb, do_deriv=True)
    assert d["d_logalpha0"][0] == (0.0 if d_free["d_logalpha0"][0] > 0 else d_free["d_logalpha0"][0])
    for k in d:
        if k != "d_logalpha0":
            assert np.array_equal(np.asarray(d[k]), np.asarray(d_free[k])), k


def test_walker_result_does_not_depend_on_padding(vb):
    """A K <= 4 run gives the same bits under KM = 4 and KM = 8."""
    subj, runs = R.runs_a()
    opt = R.options()
    sel = [runs[1], runs[7]]
    a = R.run_check(subj, sel, opt, "host", KM=4)
    b = R.run_check(subj, sel, opt, "host", KM=8)
    for x, y in zip(a, b):
        assert x["LL"] == y["LL"] and x["iters"] == y["iters"]
        assert np.array_equal(x["LLs"], y["LLs"])
        for k in R.POST_KEYS:
            assert np.array_equal(x["varpar"][k], y["varpar"][k]), k
