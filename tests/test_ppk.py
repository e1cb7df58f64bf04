"""PPK spectral clustering (src/compare_mtds/ppk: elkernel.m, bhatt.m, ppk_sc.m,
SpectralClustering.m): CPU tests.

The numpy restatement (tests/ppk_ref.py) is pinned on its own against a closed
form, quadrature and brute force over state paths; the host build of the kernels'
pair routines (tests/ppkcheck/libppkcheck.so, csrc/vbhmm_ppk_pair.h) is then held
to it at RTOL_PAIRS under conftest.stat_err.  spectral_clustering and the
bookkeeping of ppk_sc are tested on Grams from the restatement.
"""
import itertools

import numpy as np
import pytest
from scipy.integrate import quad

import ppk_ref as pr
import score_ref as sr
from conftest import RTOL_PAIRS, stat_err


@pytest.fixture(scope="module")
def ppk(vb):
    from vbhem_amd import ppk as mod
    return mod


@pytest.fixture(scope="module")
def score(vb):
    from vbhem_amd import score as mod
    return mod


@pytest.fixture(scope="module")
def pc():
    return pr.load_ppkcheck()


# ----------------------------------------------------------------------------
# the restatement, pinned independently of the product
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("bhatt", [pr.bhatt_literal, pr.bhatt_diff])
def test_ref_bhatt_is_the_integral_of_sqrt_densities(bhatt):
    """d = 1: the Bhattacharyya coefficient, by quadrature of sqrt(N1 N2)."""
    for m1, m2, v1, v2 in [(0.0, 1.0, 1.0, 2.0), (-1.5, 0.5, 0.3, 0.7), (2.0, 2.0, 1.0, 4.0)]:
        pdf = lambda x, m, v: np.exp(-0.5 * (x - m) ** 2 / v) / np.sqrt(2 * np.pi * v)
        want, _ = quad(lambda x: np.sqrt(pdf(x, m1, v1) * pdf(x, m2, v2)), -40, 40, epsabs=1e-13, epsrel=1e-13)
        got = bhatt(np.array([m1]), np.array([m2]), np.array([[v1]]), np.array([[v2]]))
        assert abs(got - want) < 1e-10 * want


@pytest.mark.parametrize("d,diag", [(1, False), (2, True), (3, False), (8, False)])
def test_ref_self_affinity_is_one(d, diag):
    h = sr.make_hmm(np.random.default_rng(d), 3, d, diag)
    for bhatt in (pr.bhatt_literal, pr.bhatt_diff):
        pot = pr.pot_matrix(h, h, bhatt=bhatt)
        assert np.max(np.abs(np.diag(pot) - 1.0)) < 1e-12
        assert np.all(pot <= 1.0 + 1e-12) and np.allclose(pot, pot.T, rtol=1e-12)


def test_ref_single_state_is_power_of_pot():
    rng = np.random.default_rng(11)
    h1, h2 = sr.make_hmm(rng, 1, 3, False), sr.make_hmm(rng, 1, 3, False)
    pot = pr.pot_matrix(h1, h2)[0, 0]
    assert 0 < pot < 1
    assert abs(pr.elkernel(h1, h2, T=1) - pot) < 1e-15
    for T in (2, 3, 10):
        assert abs(pr.elkernel(h1, h2, T=T) - pot ** (T + 1)) < 1e-13 * pot ** (T + 1)


def test_ref_recursion_is_the_sum_over_state_paths():
    """2 x 3 states, T = 3: sum over all path pairs of sqrt(P1(q) P2(r)) prod_{t=1..T+1} pot(q_t, r_t)."""
    rng = np.random.default_rng(12)
    h1, h2 = sr.make_hmm(rng, 2, 2, False), sr.make_hmm(rng, 3, 2, True)
    T, pot = 3, pr.pot_matrix(h1, h2)
    total = 0.0
    for q in itertools.product(range(2), repeat=T + 1):
        P1 = h1["prior"][q[0]] * np.prod([h1["trans"][q[t - 1], q[t]] for t in range(1, T + 1)])
        for r in itertools.product(range(3), repeat=T + 1):
            P2 = h2["prior"][r[0]] * np.prod([h2["trans"][r[t - 1], r[t]] for t in range(1, T + 1)])
            total += np.sqrt(P1 * P2) * np.prod([pot[q[t], r[t]] for t in range(T + 1)])
    got = pr.elkernel(h1, h2, T=T)
    assert abs(got - total) < 1e-13 * total


@pytest.mark.parametrize("shape", [(3, 2, False), (5, 3, True), (4, 8, False)], ids=sr.shape_id)
def test_ref_literal_and_difference_forms_agree_near_the_origin(shape):
    hmms = pr.make_set(*shape)
    a, b = pr.gram(hmms, bhatt=pr.bhatt_literal), pr.gram(hmms, bhatt=pr.bhatt_diff)
    assert np.max(np.abs(a - b) / np.abs(b)) < 1e-12


def test_ref_zero_probabilities_stay_zero():
    h = dict(prior=np.array([1.0, 0.0]), trans=np.array([[0.0, 1.0], [0.5, 0.5]]),
             pdf=[dict(mean=np.zeros(2), cov=np.ones(2)), dict(mean=np.ones(2), cov=np.ones(2))])
    for rho in (0.5, 0.3):
        assert np.isfinite(pr.elkernel(h, h, T=4, rho=rho)) and pr.elkernel(h, h, T=4, rho=rho) > 0


# ----------------------------------------------------------------------------
# the host build of the pair routines against the restatement
# ----------------------------------------------------------------------------
def host_gram(pc, score, ha, hb=None, **kw):
    rc, out = pr.run_ppkcheck(pc, score.pack_hmms(ha), None if hb is None else score.pack_hmms(hb), **kw)
    assert rc == 0
    return out


@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_host_matches_restatement(pc, score, shape):
    hmms = pr.make_set(*shape)
    assert len({len(h["prior"]) for h in hmms}) > 1 or shape[0] == 1
    got = host_gram(pc, score, hmms)
    assert stat_err(got, pr.reference(*shape)) < RTOL_PAIRS
    assert np.array_equal(got, got.T)


@pytest.mark.parametrize("T", [1, 2, 10])
@pytest.mark.parametrize("rho", [0.5, 0.3, 1.0])
@pytest.mark.parametrize("shape", [(3, 2, True), (9, 3, False)], ids=sr.shape_id)
def test_host_T_and_rho(pc, score, shape, rho, T):
    hmms = pr.make_set(*shape)
    got = host_gram(pc, score, hmms, T=T, rho=rho)
    assert stat_err(got, pr.gram(hmms, None, T, rho)) < RTOL_PAIRS


def test_host_modes_and_rectangular(pc, score):
    ha, hb = pr.make_set(5, 3, False, H=4), pr.make_set(8, 3, False, H=3, seed=1)
    rect = host_gram(pc, score, ha, hb)
    assert rect.shape == (4, 3) and stat_err(rect, pr.gram(ha, hb)) < RTOL_PAIRS
    assert stat_err(host_gram(pc, score, hb, ha), pr.gram(hb, ha)) < RTOL_PAIRS
    full = host_gram(pc, score, ha, ha)
    sym = host_gram(pc, score, ha)
    assert np.array_equal(np.triu(sym), np.triu(full)) and stat_err(sym, full) < RTOL_PAIRS
    rc, dg = pr.run_ppkcheck(pc, score.pack_hmms(ha), mode=pr.MODE_DIAG)
    assert rc == 0 and np.array_equal(dg, np.diag(full))


def test_host_translation_invariance(pc, score):
    """Means on a 2^-16 grid shifted by 2^12 (exact): the difference form gives the same
    Gram; the reference's cancelling form would lose seven digits."""
    hmms = pr.grid_set()
    moved = pr.shifted(hmms, 4096.0)
    for h, g in zip(hmms, moved):
        for p, q in zip(h["pdf"], g["pdf"]):
            assert np.array_equal(q["mean"] - 4096.0, p["mean"])
    base, got = host_gram(pc, score, hmms), host_gram(pc, score, moved)
    print("translated vs unshifted:", stat_err(got, base))
    assert stat_err(got, base) < RTOL_PAIRS
    assert stat_err(base, pr.gram(hmms)) < RTOL_PAIRS
    lit = pr.gram(moved, bhatt=pr.bhatt_literal)
    assert stat_err(lit, base) > RTOL_PAIRS  # the case does tell the two forms apart


def test_host_not_positive_definite_is_reported(pc, score):
    hmms = [dict(h) for h in pr.make_set(3, 2, False)]
    bad = dict(hmms[1])
    bad["pdf"] = [dict(p) for p in bad["pdf"]]
    bad["pdf"][0]["cov"] = np.array([[1.0, 0.0], [0.0, -3.0]])
    hmms[1] = bad
    rc, _ = pr.run_ppkcheck(pc, score.pack_hmms(hmms))
    assert rc == 1 + 1 * 3 + 0


# ----------------------------------------------------------------------------
# spectral clustering and the bookkeeping of ppk_sc
# ----------------------------------------------------------------------------
FAMILY_CASES = [(3, 2, 3, 8), (2, 2, 2, 5), (4, 3, 4, 6)]


@pytest.mark.parametrize("case", FAMILY_CASES, ids=lambda c: "K%d-d%d-F%d-n%d" % c)
def test_families_are_recovered(ppk, case):
    K, d, F, n = case
    hmms, fam = pr.families(K, d, F, n)
    A = pr.families_gram(K, d, F, n)
    for seed in range(20):
        res = ppk.ppk_sc_from_gram(hmms, A, F, seed)
        assert pr.one_label_per_family(res["label"], fam), seed


def test_ppk_sc_bookkeeping(ppk):
    hmms, fam = pr.families(3, 2, 3, 8)
    A = pr.families_gram(3, 2, 3, 8)
    res = ppk.ppk_sc_from_gram(hmms, A, 3, seed=4)
    again = ppk.ppk_sc_from_gram(hmms, A, 3, seed=4)
    assert np.array_equal(res["label"], again["label"]) and np.array_equal(res["U"], again["U"])
    N = len(hmms)
    assert res["label"].shape == (N,) and set(res["label"].tolist()) == {0, 1, 2}
    assert res["Z"].shape == (N, 3) and np.array_equal(res["Z"].sum(1), np.ones(N))
    assert np.array_equal(np.argmax(res["Z"], 1), res["label"])
    assert abs(res["weight"].sum() - 1.0) < 1e-15 and np.array_equal(res["group_size"], [8, 8, 8])
    labels, centres, U = ppk.spectral_clustering(A, 3, 3, 4)
    assert np.array_equal(labels, res["label"]) and centres.shape == (3, 3) and U.shape == (N, 3)
    assert np.allclose((U ** 2).sum(1), 1.0, atol=1e-12)
    for k in range(3):
        g = res["group"][k]
        assert np.array_equal(g, np.nonzero(res["label"] == k)[0])
        i = res["ind_center"][k]
        assert i in g and res["hmms"][k] is hmms[i]
        dist = np.sqrt(((U[g] - centres[k]) ** 2).sum(1))
        assert i == g[np.nonzero(dist == dist.min())[0][0]]
    assert res["A"] is not None and np.array_equal(res["A"], A)


def test_spectral_clustering_edge_cases(ppk):
    A = pr.families_gram(2, 2, 2, 5).copy()
    # one cluster
    labels, centres, U = ppk.spectral_clustering(A, 1, 3, 0)
    assert np.array_equal(labels, np.zeros(10, dtype=np.int64)) and centres.shape == (1, 1)
    res = ppk.ppk_sc_from_gram(pr.families(2, 2, 2, 5)[0], A, 1, 0)
    assert res["group_size"].tolist() == [10] and res["weight"].tolist() == [1.0]
    # an isolated HMM: an all-zero row and column
    A[3, :] = 0.0
    A[:, 3] = 0.0
    for type_ in (1, 2, 3):
        labels, centres, U = ppk.spectral_clustering(A, 2, type_, 0)
        assert np.isfinite(U).all() and np.isfinite(centres).all() and not np.iscomplexobj(U)
        assert labels.shape == (10,) and labels.min() >= 0 and labels.max() <= 1
    # types 1 and 2 separate two well-separated blocks too
    B = pr.families_gram(2, 2, 2, 5)
    fam = pr.families(2, 2, 2, 5)[1]
    for type_ in (1, 2):
        labels, _, _ = ppk.spectral_clustering(B, 2, type_, 1)
        assert labels.shape == (10,) and set(labels.tolist()) <= {0, 1}
    assert pr.one_label_per_family(ppk.spectral_clustering(B, 2, 2, 1)[0], fam)


def test_argument_errors(ppk):
    A = np.eye(4)
    with pytest.raises(ValueError):
        ppk.spectral_clustering(np.ones((3, 4)), 2)
    with pytest.raises(ValueError):
        ppk.spectral_clustering(A, 0)
    with pytest.raises(ValueError):
        ppk.spectral_clustering(A, 5)
    with pytest.raises(ValueError):
        ppk.spectral_clustering(A, 2, type=4)
    with pytest.raises(ValueError):
        ppk.ppk_sc_from_gram(pr.families(2, 2, 2, 5)[0], A, 2)
    with pytest.raises(ValueError):
        ppk.PpkSet(pr.families(2, 2, 2, 5)[0], device="cpu")
