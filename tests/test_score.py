"""Scoring sequences under HMMs (src/hmm/vbhmm_ll.m, vbhmm_map_state.m,
vbhmm_prob_state.m, vbhmm_random_sample.m): CPU tests.

The numpy restatement (tests/score_ref.py) is pinned on its own against closed
forms and brute force; the host build of the kernels' pair routines
(tests/scorecheck/libscorecheck.so, csrc/vbhmm_score_pair.h) is then held to
it: log-likelihoods at RTOL_PAIRS under conftest.stat_err, Viterbi paths
exactly (every max of the restatement is first shown to be decided by more
than 1e-6 relative).  The host functions of score.py are tested directly.
"""
import itertools

import numpy as np
import pytest
from scipy.stats import multivariate_normal

import score_ref as sr
from conftest import RTOL_PAIRS, stat_err

MARGIN = 1e-6


@pytest.fixture(scope="module")
def score(vb):
    from vbhem_amd import score as mod
    return mod


@pytest.fixture(scope="module")
def sc():
    return sr.load_scorecheck()


# ----------------------------------------------------------------------------
# the restatement, pinned independently of the product
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("d,diag", [(1, False), (2, False), (3, True), (8, False)])
def test_ref_single_state_is_sum_of_logpdf(d, diag):
    rng = np.random.default_rng(d)
    hmm = sr.make_hmm(rng, 1, d, diag)
    data = sr.sample_data(rng, [hmm], [1, 4, 9], d)
    ll, err = sr.vbhmm_ll(hmm, data, "")
    cov = hmm["pdf"][0]["cov"]
    mvn = multivariate_normal(hmm["pdf"][0]["mean"], np.diag(cov) if diag else cov)
    want = np.array([np.sum(mvn.logpdf(x)) for x in data])
    assert np.max(np.abs(ll - want) / np.abs(want)) < 1e-12 and not err.any()
    lln, _ = sr.vbhmm_ll(hmm, data, "n")
    assert np.allclose(lln, want / np.array([1, 4, 9]), rtol=1e-12)


def test_ref_length_one_is_log_mixture():
    rng = np.random.default_rng(5)
    hmm = sr.make_hmm(rng, 4, 2, False)
    data = sr.sample_data(rng, [hmm], [1] * 6, 2)
    ll, _ = sr.vbhmm_ll(hmm, data)
    for n, x in enumerate(data):
        rho = [multivariate_normal(p["mean"], p["cov"]).pdf(x[0]) for p in hmm["pdf"]]
        assert abs(ll[n] - np.log(np.dot(hmm["prior"], rho))) < 1e-12 * abs(ll[n])


@pytest.mark.parametrize("K,T", [(2, 1), (2, 5), (3, 2), (3, 5)])
def test_ref_brute_force_paths(K, T):
    """loglik = log of the sum over all K^T paths; the Viterbi path is their argmax."""
    rng = np.random.default_rng(10 * K + T)
    hmm = sr.make_hmm(rng, K, 2, False)
    data = sr.sample_data(rng, [hmm], [T] * 3, 2)
    for x in data:
        rho = sr.emissions(hmm, x)[0]
        paths = list(itertools.product(range(K), repeat=T))
        pr = np.array([sr.vbhmm_prob_state(hmm, [p])[0] * np.prod(rho[np.arange(T), list(p)])
                       for p in paths])
        ll = sr.forward_ll(hmm["prior"], hmm["trans"], rho)
        assert abs(ll - np.log(pr.sum())) < 1e-12 * abs(ll)
        path, vll, margin = sr.viterbi_path(hmm["prior"], hmm["trans"], rho)
        assert margin > MARGIN
        assert tuple(path) == paths[int(np.argmax(pr))]
        assert np.sort(pr)[-1] > np.sort(pr)[-2] * (1 + 1e-9)


def test_ref_floor_constant():
    assert sr.RHO_FLOOR.tobytes() == (10).to_bytes(8, "little")
    assert float(sr.RHO_FLOOR) == 4.9407e-323


# ----------------------------------------------------------------------------
# the host build of the pair routines against the restatement
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_host_pairs_match_restatement(score, sc, shape):
    K, d, diag = shape
    hmms, data = sr.make_case(K, d, diag)
    ref = sr.reference(K, d, diag)
    assert [len(x) for x in data][:4] == list(sr.RAGGED)
    assert len({len(h["prior"]) for h in hmms}) == (3 if K > 2 else 1)
    assert sr.outside_denormal_zone(ref["logrho"])
    assert ref["margin"] > MARGIN
    rc, ll, vll, paths = sr.run_scorecheck(sc, score.pack_hmms(hmms), data, d)
    assert rc == 0
    print("ll err", stat_err(ll, ref["ll"]), "viterbi ll err", stat_err(vll, ref["vll"]))
    assert stat_err(ll, ref["ll"]) < RTOL_PAIRS
    assert stat_err(vll, ref["vll"]) < RTOL_PAIRS
    for h in range(len(hmms)):
        for n in range(len(data)):
            assert np.array_equal(paths[h][n], ref["paths"][h][n]), (h, n)
    # the normalisation is by the row count: 0/0 for the empty sequence
    lens = np.array([len(x) for x in data], dtype=np.float64)
    with np.errstate(all="ignore"):
        assert stat_err(ll / lens, ref["lln"]) < RTOL_PAIRS
    assert np.isnan(ref["lln"][:, 0]).all() and (ll[:, 0] == 0).all()


@pytest.mark.parametrize("single", [False, True], ids=["all-floored", "one-floored"])
def test_host_zero_floor(score, sc, single):
    hmm, data = sr.floor_case(single)
    rho, lr = sr.emissions(hmm, data[0])
    assert sr.outside_denormal_zone(lr)
    assert (rho[2] == 0).all() if not single else (rho[:, 1] == 0).all() and (rho[:, 0] > 0).all()
    ref, _ = sr.vbhmm_ll(hmm, data, "")
    if not single:
        # the floored step contributes about log(4.94e-323)
        other = sr.forward_ll(hmm["prior"], hmm["trans"], rho[:2]) + \
            sr.forward_ll(hmm["prior"], hmm["trans"], rho[3:])
        assert abs((ref[0] - other) - np.log(4.94e-323)) < 3.0
        assert abs(ref[2] - np.log(4.94e-323)) < 1.0
    rc, ll, _, _ = sr.run_scorecheck(sc, score.pack_hmms([hmm]), data, 2)
    assert rc == 0 and np.isfinite(ll).all()
    print("floor", ll[0], ref)
    assert stat_err(ll[0], ref) < RTOL_PAIRS


def test_host_tie_break_lowest_index(score, sc):
    """States 0 and 1 are identical: every max ties, and the lowest index wins."""
    a = dict(mean=np.array([1.0, 2.0]), cov=np.array([[1.0, 0.3], [0.3, 2.0]]))
    hmm = dict(prior=np.array([0.35, 0.35, 0.3]),
               trans=np.array([[0.3, 0.3, 0.4], [0.3, 0.3, 0.4], [0.25, 0.25, 0.5]]),
               pdf=[a, dict(a), dict(mean=np.array([4.0, 0.0]), cov=np.array([0.7, 1.1]))])
    rng = np.random.default_rng(3)
    data = sr.sample_data(rng, [hmm], [1, 2, 9, 17, 30], 2)
    rc, _, _, paths = sr.run_scorecheck(sc, score.pack_hmms([hmm]), data, 2)
    assert rc == 0
    ref, _, _ = sr.vbhmm_map_state(hmm, data)
    seen = np.concatenate(paths[0])
    assert 1 not in seen and 0 in seen and 2 in seen
    for n in range(len(data)):
        assert np.array_equal(paths[0][n], ref[n])


def test_host_ieee_cases(score, sc):
    hmm = dict(prior=np.zeros(2), trans=np.array([[0.5, 0.5], [0.2, 0.8]]),
               pdf=[dict(mean=np.zeros(2), cov=np.eye(2)), dict(mean=np.ones(2), cov=np.eye(2))])
    data = [np.array([[0.1, 0.2]]), np.zeros((0, 2)), np.array([[0.1, 0.2], [0.3, 0.1]])]
    rc, ll, _, _ = sr.run_scorecheck(sc, score.pack_hmms([hmm]), data, 2)
    assert rc == 0
    assert ll[0, 0] == -np.inf and ll[0, 1] == 0.0 and np.isnan(ll[0, 2])
    ref, err = sr.vbhmm_ll(hmm, data, "n")
    assert ref[0] == -np.inf and err[0] and np.isnan(ref[1]) and not err[1] and np.isnan(ref[2])
    ref0, _ = sr.vbhmm_ll(hmm, data, "")
    assert ref0[1] == 0.0


def test_host_not_positive_definite_names_state(score, sc):
    rng = np.random.default_rng(8)
    hmms = [sr.make_hmm(rng, 3, 2, False) for _ in range(3)]
    hmms[1]["pdf"][2]["cov"] = np.array([[1.0, 2.0], [2.0, 1.0]])
    hmms[2]["pdf"][0]["cov"] = np.array([[-1.0, 0.0], [0.0, 1.0]])
    data = sr.sample_data(rng, hmms, [3], 2)
    rc, _, _, _ = sr.run_scorecheck(sc, score.pack_hmms(hmms), data, 2)
    assert rc == 1 + 1 * 3 + 2          # the first: HMM 1, state 2
    with pytest.raises(np.linalg.LinAlgError):
        sr.vbhmm_ll(hmms[1], data)


def test_padded_states_contribute_nothing(score, sc):
    hmms, data = sr.make_case(5, 3, False)
    ref = sr.reference(5, 3, False)
    packed = score.pack_hmms(hmms)
    for h, K in enumerate(packed["nstates"]):
        packed["prior"][h, K:] = 0.5
        packed["trans"][h, K:, :] = 0.25
        packed["trans"][h, :, K:] = 0.25
        packed["mean"][h, K:] = np.nan
        packed["cov"][h, K:] = np.nan
    rc, ll, _, paths = sr.run_scorecheck(sc, packed, data, 3)
    assert rc == 0 and stat_err(ll, ref["ll"]) < RTOL_PAIRS
    assert all(np.array_equal(paths[h][n], ref["paths"][h][n]) for h in range(3) for n in range(6))


# ----------------------------------------------------------------------------
# host functions of score.py
# ----------------------------------------------------------------------------
def test_prob_state(score):
    rng = np.random.default_rng(2)
    hmm = sr.make_hmm(rng, 4, 2, True)
    seqs = [rng.integers(0, 4, T) for T in (1, 2, 7)]
    got = score.vbhmm_prob_state(hmm, seqs)
    assert np.array_equal(got, sr.vbhmm_prob_state(hmm, seqs))
    assert score.vbhmm_prob_state(hmm, seqs[2]) == got[2]
    assert got[0] == hmm["prior"][seqs[0][0]]


def test_multirnd_fixed_uniforms(score):
    cum = np.cumsum([0.25, 0.25, 0.5])
    # a uniform exactly on a cumulative boundary stays in the lower bin (f > cum is false)
    for f, want in ((0.0, 0), (0.1, 0), (0.25, 0), (0.2500001, 1), (0.5, 1), (0.75, 2), (0.999, 2)):
        assert score.multirnd(cum, f) == want == sr.multirnd(cum, f)


def test_random_sample_shapes_and_seed(score):
    rng = np.random.default_rng(4)
    hmm = sr.make_hmm(rng, 3, 2, False)
    h, data = score.vbhmm_random_sample(hmm, 7, 5, seed=11)
    assert len(h) == len(data) == 5
    assert all(len(a) == 7 and b.shape == (7, 2) for a, b in zip(h, data))
    h2, data2 = score.vbhmm_random_sample(hmm, 7, 5, seed=11)
    assert all(np.array_equal(a, b) for a, b in zip(h, h2))
    assert all(np.array_equal(a, b) for a, b in zip(data, data2))
    h3, _ = score.vbhmm_random_sample(hmm, 7, 5, seed=12)
    assert any(not np.array_equal(a, b) for a, b in zip(h, h3))
    # a length distribution: P(length = 2) = 0.5, P(length = 4) = 0.5
    hl, dl = score.vbhmm_random_sample(hmm, [0, 0.5, 0, 0.5], 40, seed=1)
    assert {len(a) for a in hl} == {2, 4} and all(len(a) == len(b) for a, b in zip(hl, dl))


def test_random_sample_state_frequencies(score):
    rng = np.random.default_rng(6)
    hmm = sr.make_hmm(rng, 3, 2, True)
    h, data = score.vbhmm_random_sample(hmm, 10, 2000, seed=5)       # 2e4 state draws
    first = np.bincount([a[0] for a in h], minlength=3) / 2000.0
    sd = np.sqrt(hmm["prior"] * (1 - hmm["prior"]) / 2000.0)
    assert (np.abs(first - hmm["prior"]) < 4 * sd).all()
    cnt = np.zeros((3, 3))
    for a in h:
        np.add.at(cnt, (a[:-1], a[1:]), 1)
    n = cnt.sum(1, keepdims=True)
    sd = np.sqrt(hmm["trans"] * (1 - hmm["trans"]) / n)
    assert (np.abs(cnt / n - hmm["trans"]) < 4 * sd).all()
    # emissions: per state, the sample mean within 4 standard errors of the state's mean
    X, Z = np.concatenate(data), np.concatenate(h)
    for k, p in enumerate(hmm["pdf"]):
        xs = X[Z == k]
        assert (np.abs(xs.mean(0) - p["mean"]) < 4 * np.sqrt(p["cov"] / len(xs))).all()


def test_hmmset_needs_gpu(score):
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="no CPU path"):
        score.HmmSet([sr.make_hmm(rng, 2, 2, False)], device="cpu")


def test_pack_hmms_layout(score):
    rng = np.random.default_rng(9)
    hmms = [sr.make_hmm(rng, 3, 2, True), sr.make_hmm(rng, 1, 2, False)]
    p = score.pack_hmms(hmms)
    assert p["covmode"] == 1 and p["cov"].shape == (2, 3, 2, 2) and list(p["nstates"]) == [3, 1]
    assert np.array_equal(p["cov"][0, 1], np.diag(hmms[0]["pdf"][1]["cov"]))
    assert score.pack_hmms(hmms[:1])["covmode"] == 0
    with pytest.raises(ValueError):
        score.pack_hmms([hmms[0], sr.make_hmm(rng, 2, 3, True)])


def test_group_hmms_from_posterior(vb, score):
    """convert_h3mrtoh3mb.m:9-72: normalised eta / epsilon rows, cov = sym(inv(W)) / (v - d - 1)."""
    _, post, _ = vb.synth_workload("C2", N=8)
    hm = score.group_hmms(post)
    assert len(hm) == post.K and all(len(h["pdf"]) == post.S for h in hm)
    d = post.m.shape[2]
    for j, h in enumerate(hm):
        assert abs(h["prior"].sum() - 1) < 1e-14 and np.allclose(h["trans"].sum(1), 1, atol=1e-14)
        assert np.allclose(h["prior"], post.eta[j] / post.eta[j].sum(), rtol=1e-15)
        for k, p in enumerate(h["pdf"]):
            den = post.v[j, k] - d - 1 if post.v[j, k] > d + 1 else post.v[j, k]
            assert np.allclose(p["cov"] @ post.W[j, k] * den, np.eye(d), atol=1e-10)
            assert np.array_equal(p["cov"], p["cov"].T) and np.array_equal(p["mean"], post.m[j, k])
    packed = score.pack_hmms(hm)          # scorable: every covariance positive definite
    assert all(np.linalg.eigvalsh(c).min() > 0 for c in packed["cov"].reshape(-1, d, d))
