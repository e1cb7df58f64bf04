"""The batched VB-HMM EM on the GPU (csrc/vbhmm_em.hip): vbhmm_em_batch against the
oracle and against the host walker of the same routines, bitwise independence of a run
from its position, from the launch chunking and from KM, NaN containment, vbhmm_em_gamma
against vbhmm_fb and the C forward-backward, and the engine="fused" path of
vbhmm_learn_batch / learn_hyps_batch against engine="loop".  The cases of inputs (d) and
(e) sit at the corners of the kernel's buckets (K = KM, K * dim = 64 lanes, 8 rounds of
the covariance loop, a third round of sequences, empty sequences) and are compared with
the oracle directly, with no run left out.  Inputs and conditions:
tests/vbhmm_em_batch_ref.py.
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


CORNERS = R.NAMES_D + R.NAMES_E


@pytest.mark.parametrize("name", CORNERS)
def test_bucket_corners_match_oracle_and_host_walker(vb, vo, name):
    """The device against the walker AND against the oracle itself: what walker and
    kernel share cannot hide behind their agreement."""
    subj, runs, opt = R.corner_input(name)
    dev = _vs_host(subj, runs, opt, name)
    ref = R.oracle_runs(name, subj, runs, opt)
    assert not any(R.near_threshold(r["LLs"], opt["minDiff"]) for r in ref), name
    assert R.compare_with_oracle(dev, ref, opt, post_err, name) == 0, name
    for i, (s, K, g) in enumerate(runs):      # the posterior at the last E-step
        est = R.oracle_estep_posterior(subj[s], K, opt, g, ref[i]["iters"])
        for k in R.POST_KEYS:
            assert post_err(dev[i]["varpar_estep"][k], est[k]) < 1e-8, (name, i, k)
    d1 = R.run_check(subj, runs, opt, "device", max_iter=1)
    for i, (d, (s, K, g)) in enumerate(zip(d1, runs)):
        first = R.oracle_first_iteration(subj[s], K, opt, g)
        assert d["iters"] == 1 and d["status"] == 1, (name, i)
        for k in ("Nk1", "Nk", "M", "xbar", "t1_S"):
            assert stat_err(d[k], first[k]) < RTOL_PAIRS, (name, i, k)
        assert abs(d["LLs"][0] - first["L"]) <= RTOL_PAIRS * abs(first["L"]), (name, i)


def test_empty_sequences_change_no_bit_on_the_device(vb):
    subj, runs, opt = R.corner_input("e0")
    a = R.run_check(subj, runs, opt, "device")
    b = R.run_check(R.without_empty(subj), runs, opt, "device")
    for i, (x, y) in enumerate(zip(a, b)):
        assert R.same_bits(x, y), i


@pytest.mark.parametrize("name", ["d4x2", "d4x8", "d3x2w", "c8", "e0"])
def test_result_does_not_depend_on_KM_on_the_device(vb, name):
    """The contract of csrc/vbhmm_em.hip: a K <= 4 run gives the same bits under KM = 4 and
    KM = 8 (Python takes KM from the largest K of the whole list)."""
    subj, runs, opt = R.runs_c(8) + (R.options(8),) if name == "c8" else R.corner_input(name)
    assert max(r[1] for r in runs) <= 4
    four = R.run_check(subj, runs, opt, "device", KM=4)
    eight = R.run_check(subj, runs, opt, "device", KM=8)
    for i, (x, y) in enumerate(zip(four, eight)):
        assert R.same_bits(x, y, KM_differs=True), (name, i)


def test_position_independence_bitwise_at_the_full_bucket(vb):
    """K = 8 and K = 5 runs at dim = 8 of a larger and a smaller subject, mixed: with one
    run per launch every launch reuses slot 0, a larger run before a smaller one."""
    subj, runs, opt = R.runs_mixed()
    base = R.run_check(subj, runs, opt, "device")
    one = R.run_check(subj, runs, opt, "device", chunk_runs=1)
    two = R.run_check(subj, runs, opt, "device", chunk_runs=2)
    rev = R.run_check(subj, runs[::-1], opt, "device", chunk_runs=1)
    for i in range(len(runs)):
        assert R.same_bits(base[i], one[i]), i
        assert R.same_bits(base[i], two[i]), i
        assert R.same_bits(base[i], rev[len(runs) - 1 - i]), i
    host = R.run_check(subj, runs, opt, "host")
    for i, (d, h) in enumerate(zip(base, host)):
        assert d["iters"] == h["iters"] and d["status"] == h["status"], i
        np.testing.assert_allclose(d["LLs"], h["LLs"], rtol=1e-9, err_msg=f"mixed run {i}")


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


@pytest.mark.parametrize("name", ["d8x8", "d4x8", "e0"])
def test_gamma_matches_the_c_forward_backward(vb, vo, name):
    """Gamma-only mode at the full buckets and on the subject with empty sequences,
    against the C restatement of vbhmm_fb_mex.c on the CPU."""
    from vbhem_amd import vbhmm
    from vbhem_amd.vbhmm_em import vbhmm_em_gamma
    subj, runs, opt = R.corner_input(name)
    dim = len(opt["mu0"])
    sb = vbhmm.SubjectBatch(subj, dim, DEV)
    items = [(0, vp) for vp in R.initial_posteriors(subj, runs, opt)]
    got = vbhmm_em_gamma(sb, items)
    assert len(got) == len(items)
    for (s, vp), gam in zip(items, got):
        ref = vo.c_vbhmm_fb(subj[s], vp)["gamma"].transpose(2, 1, 0)         # [K, N, maxT]
        assert len(gam) == len(subj[s])
        for n, g in enumerate(gam):
            T = subj[s][n].shape[0]
            assert g.shape == (ref.shape[0], T), (name, n)
            if T:
                assert np.max(np.abs(g - ref[:, n, :T])) <= 1e-12 * np.max(np.abs(ref[:, n, :T])), (name, n)
    if name == "e0":
        assert [n for n, g in enumerate(got[0]) if g.shape[1] == 0] == list(R.EMPTY_AT)


@pytest.fixture(scope="module")
def engines(vb):
    from vbhem_amd.vbhmm_em import vbhmm_learn_batch
    subj = R.demo_subjects()
    opt = R.options(numtrials=4)
    loop = vbhmm_learn_batch(subj, [1, 2, 3], opt, device=DEV)
    fused = vbhmm_learn_batch(subj, [1, 2, 3], opt, device=DEV, engine="fused")
    return subj, loop, fused


def test_learn_batch_engines_agree(vb, engines):
    _engines_agree(vb, *engines)


def test_learn_batch_engines_agree_in_the_larger_bucket(vb):
    """dim = 3, K = 4 and 5 in one call (KM = 8), injected GMMs, 2 trials, 3 subjects."""
    from vbhem_amd.vbhmm_em import vbhmm_learn_batch
    rng = np.random.default_rng(81)
    subj = [R.states_subject(82 + s, 5, 3, rng.integers(3, 10, 14 + 3 * s)) for s in range(3)]
    gmms = [{K: R.gmm_trials(d, K, 2, seed=90 + K) for K in (4, 5)} for d in subj]
    opt = R.options(3, numtrials=2)
    loop = vbhmm_learn_batch(subj, [4, 5], opt, device=DEV, gmms=gmms)
    fused = vbhmm_learn_batch(subj, [4, 5], opt, device=DEV, gmms=gmms, engine="fused")
    _engines_agree(vb, subj, loop, fused)


def _engines_agree(vb, subj, loop, fused):
    from vbhem_amd.vbhmm_em import vbhmm_remove_empty
    (hl, Ll), (hf, Lf) = loop, fused
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
    assert base.N == ref.N == len(subj)


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
