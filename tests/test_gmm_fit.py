"""The batched GMM fit on the CPU: the serial walker of csrc/vbhmm_gmm_run.h (through
tests/gmmcheck) against vbhmm_em.py gmm_fit_randsample, and random_gmm_batch's draws and
failure replay on a stand-in engine with the walker behind it.  Inputs, tolerances and the
condition under which a fit may be left out: tests/gmm_ref.py.
"""
import numpy as np
import pytest

import gmm_ref as G
import vbhmm_em_batch_ref as R
from conftest import post_err


def test_walker_matches_reference_on_the_demo_subset(vb):
    subj, fits, _ = G.demo_fits()
    got = G.run_fits(subj, fits, 2)
    assert len(fits) >= 72
    excluded = G.compare_with_reference(got, subj, fits, post_err, "demo")
    ill = [i for i, g in enumerate(got) if g["status"] == G.ILL]
    print("demo subset: fits", len(fits), "ill-conditioned", ill, "left out", excluded)
    # the draws the host driver had to repeat are the ill-conditioned ones, and only they
    assert ill == list(range(72, len(fits))) and len(ill) == 2
    assert all(f[3] == 1e-10 for f in fits[:72] if f[3]) and sum(1 for f in fits if f[3]) == 2


@pytest.mark.parametrize("dim", [3, 8])
def test_walker_matches_reference_in_higher_dimensions(vb, dim):
    subj, fits = G.dim_fits(dim)
    got = G.run_fits(subj, fits, dim)
    G.compare_with_reference(got, subj, fits, post_err, f"dim{dim}")
    assert all(g["status"] == G.CONVERGED for g in got)


@pytest.mark.parametrize("K,dim", G.CORNERS)
def test_walker_matches_reference_at_the_bucket_corners(vb, K, dim):
    subj, fits = G.corner_fits(K, dim)
    got = G.run_fits(subj, fits, dim)
    assert all(g["status"] < G.ILL for g in got)
    assert G.compare_with_reference(got, subj, fits, post_err, f"K{K}d{dim}") == 0
    if K <= 4:      # the fit does not depend on the padding
        for a, b in zip(got, G.run_fits(subj, fits, dim, KM=8)):
            assert G.same_bits(a, b, KM_differs=True)


def test_walker_edge_sizes(vb):
    subj, fits = G.edge_fits()
    got = G.run_fits(subj, fits, 2)
    G.compare_with_reference(got, subj, fits, post_err, "edge")
    print("edge sizes: status", [g["status"] for g in got], "iters", [g["iters"] for g in got])
    # KM = 4 against KM = 8 where K <= 4: a fit does not depend on the padding
    small = [(i, f) for i, f in enumerate(fits) if f[1] <= 4]
    four = G.run_fits(subj, [f for _, f in small], 2, KM=4)
    for (i, _), g4 in zip(small, four):
        assert G.same_bits(got[i], g4, KM_differs=True), i


def test_max_iter_is_reported(vb):
    subj, fits, _ = G.demo_fits()
    g = G.run_fits(subj, fits[:1], 2, max_iter=5)[0]
    ref = G.ref_fit(np.concatenate(subj[fits[0][0]]), fits[0][1], fits[0][2], max_iter=5)
    assert ref["status"] == G.MAX_ITER and ref["iters"] == 5
    assert g["status"] == G.MAX_ITER and g["iters"] == 5
    np.testing.assert_allclose(g["lls"], ref["lls"], rtol=1e-9)
    for k in ("prior", "mean", "cov"):
        assert post_err(g[k], ref[k]) < 1e-8, k


def test_planted_ill_conditioned_fit(vb):
    subj = G.planted_subject()
    X = subj[0][0]
    ref = G.ref_fit(X, 2, G.PLANTED_ROWS)
    # the covariance the reference's second iteration leaves is singular: two
    # log-likelihoods, then LinAlgError from the factorisation that opens the third
    assert ref["status"] == G.ILL and len(ref["lls"]) == 2
    bad, reg = G.run_fits(subj, [(0, 2, G.PLANTED_ROWS, 0.0), (0, 2, G.PLANTED_ROWS, 1e-10)], 2)
    assert bad["status"] == G.ILL
    assert (bad["raw"][0] == G.SENTINEL).all() and (bad["raw"][2] == G.SENTINEL).all()
    ref2 = G.ref_fit(X, 2, G.PLANTED_ROWS, reg=1e-10)
    print("planted: ill at iteration", bad["iters"], "regularised iters", reg["iters"], ref2["iters"])
    assert ref2["status"] == G.CONVERGED and reg["status"] == G.CONVERGED and reg["iters"] == ref2["iters"]
    np.testing.assert_allclose(reg["lls"], ref2["lls"], rtol=1e-9)
    for k in ("prior", "mean", "cov"):
        assert post_err(reg[k], ref2[k]) < 1e-8, k


def test_bad_fits_write_nothing(vb):
    subj = [R.gaussian_subject(41, [30]), R.gaussian_subject(42, [2])]
    fits = [(0, 2, np.array([0, 29]), 0.0),
            (0, 1, np.array([3]), 0.0),            # K = 1
            (1, 2, np.array([0, 1]), 0.0),         # N <= K
            (0, 2, np.array([4, 30]), 0.0),        # a row >= N
            (0, 2, np.array([5, 20]), 0.0)]
    got = G.run_fits(subj, fits, 2)
    assert [g["status"] for g in got[:4]] == [G.CONVERGED, G.BAD, G.BAD, G.BAD]
    assert got[4]["status"] in (G.CONVERGED, G.MAX_ITER)
    for i in (1, 2, 3):
        assert G.untouched(got[i]), i
    alone = G.run_fits(subj, [fits[0], fits[4]], 2)
    assert G.same_bits(got[0], alone[0]) and G.same_bits(got[4], alone[1])


def test_random_gmm_batch_replays_the_host_draws(vb):
    em = G.em_mod()
    subj = [R.demo_subjects()[2]]
    opt = R.options(numtrials=12)
    hs = G.HostSubjects(subj, 2)
    info = {}
    got = em.random_gmm_batch(hs, [2, 3], opt, fit_batch=G.standin_fit_batch, info=info)
    for K in (2, 3):
        want = em._draw_inits(subj[0], K, opt, None)
        assert len(got[(0, K)]) == len(want) == 12
        for t, (a, b) in enumerate(zip(got[(0, K)], want)):
            for k in ("prior", "mean", "cov"):
                assert post_err(a[k], b[k]) < 1e-8, (K, t, k)
    # round 1 fits everything, round 2 the two streams from their failed trial on; that
    # round brings no new failure
    assert info["rounds"] == 2
    assert info["regularised"] == {(0, 2): [3], (0, 3): [10]}
    assert info["draws"] == {(0, 2): 13, (0, 3): 13}


def test_random_gmm_batch_closed_forms_consume_no_draws(vb):
    em = G.em_mod()
    subj = [R.gaussian_subject(43, [2]), R.demo_subjects()[0]]
    opt = R.options(numtrials=3)
    info = {}
    got = em.random_gmm_batch(G.HostSubjects(subj, 2), [1, 2], opt, fit_batch=G.standin_fit_batch, info=info)
    for s in (0, 1):
        for K in (1, 2):
            want = em._draw_inits(subj[s], K, opt, None)
            assert len(got[(s, K)]) == len(want)
            for a, b in zip(got[(s, K)], want):
                for k in ("prior", "mean", "cov"):
                    assert post_err(a[k], b[k]) < 1e-8, (s, K, k)
    assert set(info["draws"]) == {(1, 2)} and info["rounds"] == 1


def test_double_failure_raises_as_the_host_path(vb):
    em = G.em_mod()
    subj = G.planted_subject()
    opt = R.options(numtrials=12, seed=1)
    with pytest.raises(np.linalg.LinAlgError):
        em._draw_inits(subj[0], 2, opt, None)
    with pytest.raises(np.linalg.LinAlgError):
        em.random_gmm_batch(G.HostSubjects(subj, 2), [2], opt, fit_batch=G.standin_fit_batch)


@pytest.mark.parametrize("W0", [0.001, [0.001, 0.004]])
def test_initial_posterior_matches_vbhmm_init(vb, W0):
    subj, fits, _ = G.demo_fits()
    fits = fits[:24] + fits[72:]
    opt = R.options(W0=W0)
    hv, _ = G.hyper_vector(opt)
    for KM in (4, 8):
        got = G.run_fits(subj, fits, 2, hyper=hv, KM=KM)
        G.check_initial_posterior(got, subj, fits, opt, post_err, KM, f"KM{KM}")


def test_init_option_is_checked(vb):
    em = G.em_mod()
    with pytest.raises(ValueError):
        em.vbhmm_learn_batch([], [2], R.options(), init="gpu")
