"""The batched VB-HMM EM on the GPU (csrc/vbhmm_em.hip): vbhmm_em_batch against the
oracle and against the host walker of the same routines, bitwise independence of a run
from its position and from the launch chunking, NaN containment, vbhmm_em_gamma against
vbhmm_fb, and the engine="fused" path of vbhmm_learn_batch / learn_hyps_batch against
engine="loop".  Inputs and conditions: tests/vbhmm_em_batch_ref.py.
"""
import numpy as np
import pytest

import vbhmm_em_batch_ref as R
from conftest import RTOL_PAIRS, post_err, stat_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _vs_host(subj, runs, opt, tag):
    dev = R.run_check(subj, runs, opt, "device")
    host = R.run_check(subj, runs, opt, "host")
    for i, (d, h) in enumerate(zip(dev, host)):
        assert d["iters"] == h["iters"] and d["status"] == h["status"], (tag, i)
        np.testing.assert_allclose(d["LLs"], h["LLs"], rtol=1e-9, err_msg=f"{tag} run {i}")
        for k in R.POST_KEYS:
            assert post_err(d["varpar"][k], h["varpar"][k]) < 1e-8, (tag, i, k)
            assert post_err(d["varpar_estep"][k], h["varpar_estep"][k]) < 1e-8, (tag, i, k)
    d1 = R.run_check(subj, runs, opt, "device", max_iter=1)
    h1 = R.run_check(subj, runs, opt, "host", max_iter=1)
    for i, (d, h) in enumerate(zip(d1, h1)):
        for k in ("Nk1", "Nk", "M", "xbar", "t1_S"):
            assert stat_err(d[k], h[k]) < RTOL_PAIRS, (tag, i, k)
        assert abs(d["LL"] - h["LL"]) <= RTOL_PAIRS * abs(h["LL"]), (tag, i)
    return dev


@pytest.mark.parametrize("name", ["a", "b"])
def test_batch_matches_oracle_and_host_walker(vb, vo, name):
    subj, runs = R.runs_a() if name == "a" else R.runs_b()
    opt = R.options()
    dev = _vs_host(subj, runs, opt, name)
    R.compare_with_oracle(dev, R.oracle_runs(name, subj, runs, opt), opt, post_err, name)


@pytest.mark.parametrize("dim", [2, 3, 8])
def test_edge_subjects_match_host_walker(vb, dim):
    subj, runs = R.runs_c(dim)
    _vs_host(subj, runs, R.options(dim), f"c{dim}")


def test_position_independence_bitwise(vb):
    subj, runs = R.runs_a()
    opt = R.options()
    base = R.run_check(subj, runs, opt, "device")
    again = R.run_check(subj, runs, opt, "device")
    perm = np.random.default_rng(3).permutation(len(runs))
    shuffled = R.run_check(subj, [runs[i] for i in perm], opt, "device")
    rev = R.run_check(subj, runs[::-1], opt, "device")
    one = R.run_check(subj, runs, opt, "device", chunk_runs=1)
    seven = R.run_check(subj, runs, opt, "device", chunk_runs=7)
    for i in range(len(runs)):
        assert R.same_bits(base[i], again[i]), i
        assert R.same_bits(base[i], one[i]), i
        assert R.same_bits(base[i], seven[i]), i
        assert R.same_bits(base[i], rev[len(runs) - 1 - i]), i
    for j, i in enumerate(perm):
        assert R.same_bits(base[i], shuffled[j]), i


def test_unstable_run_is_contained_on_the_device(vb):
    R.check_unstable("device")


def test_gamma_matches_vbhmm_fb(vb):
    from vbhem_amd import vbhmm
    from vbhem_amd.vbhmm_em import vbhmm_em_gamma
    subj, runs = R.runs_b()
    csub, cruns = R.runs_c(2)
    datas = [subj[0]] + csub
    opt = R.options()
    sb = vbhmm.SubjectBatch(datas, 2, DEV)
    items = []
    for s, K, g in [runs[4], runs[7], runs[10]]:         # K = 2, 3, 5 on the 70-sequence subject
        items.append((0, R.initial_posteriors(datas, [(0, K, g)], opt)[0]))
    for s, K, g in cruns[:3]:                              # 64 / 65 / 1 sequences
        items.append((s + 1, R.initial_posteriors(datas, [(s + 1, K, g)], opt)[0]))
    got = vbhmm_em_gamma(sb, items)
    for (s, vp), gam in zip(items, got):
        ref = vbhmm.vbhmm_fb(datas[s], vp, device=DEV)["gamma_all"]          # [K, N, maxT]
        assert len(gam) == len(datas[s])
        for n, g in enumerate(gam):
            T = datas[s][n].shape[0]
            assert g.shape == (ref.shape[0], T)
            assert np.max(np.abs(g - ref[:, n, :T])) <= 1e-12 * np.max(np.abs(ref[:, n, :T]))


@pytest.fixture(scope="module")
def engines(vb):
    from vbhem_amd.vbhmm_em import vbhmm_learn_batch
    subj = R.demo_subjects()
    opt = R.options(numtrials=4)
    loop = vbhmm_learn_batch(subj, [1, 2, 3], opt, device=DEV)
    fused = vbhmm_learn_batch(subj, [1, 2, 3], opt, device=DEV, engine="fused")
    return subj, loop, fused


def test_learn_batch_engines_agree(vb, engines):
    from vbhem_amd.vbhmm_em import vbhmm_remove_empty
    subj, (hl, Ll), (hf, Lf) = engines
    np.testing.assert_allclose(Lf, Ll, rtol=1e-9)
    for s, (a, b) in enumerate(zip(hl, hf)):
        assert a["model_bestK"] == b["model_bestK"], s
        np.testing.assert_allclose(b["model_LL"], a["model_LL"], rtol=1e-9)
        for ka, kb in zip(a["model_all"], b["model_all"]):
            np.testing.assert_allclose(kb["trials_LL"], ka["trials_LL"], rtol=1e-9)
            # the trial the fused engine picked: its loop-engine bound is within 1e-9 of the loop's best
            pick = int(np.nanargmax(kb["trials_LL"]))
            best = np.nanmax(ka["trials_LL"])
            assert abs(ka["trials_LL"][pick] - best) <= 1e-9 * abs(best), s
        assert len(b["gamma"]) == len(subj[s])
        for g, seq in zip(b["gamma"], subj[s]):
            assert g.shape == (len(b["pdf"]), seq.shape[0])
            np.testing.assert_allclose(g.sum(0), 1.0, rtol=1e-12)
    base = vb.hmms_to_h3m_hem([vbhmm_remove_empty(h, 1e-3) for h in hf], vb.COV_FULL, True)
    ref = vb.hmms_to_h3m_hem([vbhmm_remove_empty(h, 1e-3) for h in hl], vb.COV_FULL, True)
    assert base.N == ref.N == 10


def _lhb_setup(engine):
    from vbhem_amd.vbhmm_em import hyps_batch_objective
    subj = R.demo_subjects()[:3]
    opt = R.options(numtrials=2, learn_hyps_batch=["alpha0", "epsilon0", "v0", "beta0", "W0", "mu0"])
    return hyps_batch_objective(subj, [2], opt, device=DEV, engine=engine)


def test_hyps_batch_objective_engines_agree(vb):
    gl, X0, _, _ = _lhb_setup("loop")
    gf, X0f, _, _ = _lhb_setup("fused")
    assert np.array_equal(X0, X0f)
    step = 0.05 * np.cos(np.arange(X0.size))
    for X in (X0, X0 + step):
        fl, dl = gl(X)
        ff, df = gf(X)
        assert abs(ff - fl) <= 1e-9 * abs(fl)
        assert stat_err(df, dl) < 1e-8


def test_learn_hyps_batch_runs_under_the_fused_engine(vb):
    from vbhem_amd.vbhmm_em import hyps_batch_objective, vbhmm_learn_batch
    subj = R.demo_subjects()[:3]
    opt = R.options(numtrials=2, learn_hyps_batch=["alpha0", "epsilon0", "beta0"])
    g, X0, _, _ = hyps_batch_objective(subj, [2], opt, device=DEV, engine="fused")
    first = -g(X0)[0]
    hmms, Ls = vbhmm_learn_batch(subj, [2], opt, device=DEV, engine="fused")
    assert len(hmms) == 3 and np.isfinite(Ls).all()
    for s, h in enumerate(hmms):
        opt_L = h["learn_hyps_batch"]["opt_L"]
        assert np.isfinite(opt_L) and opt_L >= first
        assert set(h["vbopt"]) == {"alpha0", "epsilon0", "beta0"}
        assert len(h["gamma"]) == len(subj[s])


def test_learn_hyps_runs_under_the_fused_engine(vb):
    """Per-subject hyperparameter learning: every evaluation a fused call of one run.  The
    first evaluation starts from a converged trial, so the optimum is not below that
    trial's bound; the two engines' optima are printed, not compared (BFGS amplifies
    last-bit differences)."""
    from vbhem_amd.vbhmm_em import vbhmm_learn
    data = R.demo_subjects()[5]
    opt = R.options(numtrials=2, learn_hyps=1, hyp_length=5)
    h = vbhmm_learn(data, [2], opt, device=DEV, engine="fused")
    ref = vbhmm_learn(data, [2], opt, device=DEV)
    print("learn_hyps opt_L fused", h["learn_hyps"]["opt_L"], "loop", ref["learn_hyps"]["opt_L"])
    assert np.isfinite(h["LL"]) and np.isfinite(h["learn_hyps"]["opt_L"])
    assert set(h["learn_hyps"]["vbopt"]) == set(ref["learn_hyps"]["vbopt"])
    low = np.min(h["trials_LL_random"])
    assert h["learn_hyps"]["opt_L"] >= low - 1e-9 * abs(low)
    np.testing.assert_allclose(h["trials_LL_random"], ref["trials_LL_random"], rtol=1e-9)
    assert len(h["gamma"]) == len(data) and len(h["pdf"]) == 2


def test_more_than_eight_states_falls_back_to_the_loop(vb, capi_lib):
    from vbhem_amd.vbhmm_em import vbhmm_learn
    subj, _ = R.runs_b()
    opt = R.options(maxIter=5)
    g = R.gmm_trials(subj[0], 9, 1, seed=5)
    a = vbhmm_learn(subj[0], [9], opt, device=DEV, gmms={9: g})
    b = vbhmm_learn(subj[0], [9], opt, device=DEV, gmms={9: g}, engine="fused")
    assert a["LL"] == b["LL"]
    for k in R.POST_KEYS:
        assert np.array_equal(a["varpar"][k], b["varpar"][k]), k
    # the C call itself refuses K = 9 (a KM of 16)
    R.run_check(subj, [(0, 9, g[0])], opt, "device", expect=-2)
    assert b"K <= 8" in capi_lib.vbhem_last_error()
