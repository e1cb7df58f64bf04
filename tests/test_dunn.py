"""The evaluation of a clustering run on the CPU (vbhem_amd/evaluate.py): evaluate_run and
summarize on hand-made results of every method against values worked out by hand from
the formulas of Synthetic_experiment/evaluate_vbhem_jounarl.m, the PPK criteria against
the restatement (tests/dunn_ref.py), and the cases of the Dunn index that need no
kernel (a single remaining centre)."""
import math

import numpy as np
import pytest

import dunn_ref as dr

TRUE = np.array([0, 1, 1, 0, 0, 1])
PRED = np.array([0, 1, 1, 0, 1, 1])      # against TRUE: RI = 10 / 15, purity = 5 / 6
# 15 pairs.  Together in both: (0,3), (1,2), (1,5), (2,5): 4.  Apart in both: 0 and 3
# against 1, 2, 5: 6.  Subject 4 is with 1, 2, 5 in PRED but with 0, 3 in TRUE: 5 misses.
RI, PURITY = 10 / 15, 5 / 6


@pytest.fixture(scope="module")
def ev(vb):
    from vbhem_amd import evaluate
    return evaluate


def hmm_of(S):
    return dict(prior=np.full(S, 1.0 / S), trans=np.full((S, S), 1.0 / S),
                pdf=[dict(mean=np.array([float(s), 0.0]), cov=np.eye(2)) for s in range(S)])


def vhem_cell(label, K, counts):
    """A vhem_cluster output: ``counts[j]`` the emit_vcounts of group HMM j."""
    label = np.asarray(label)
    groups = [np.flatnonzero(label == j) for j in range(K)]
    hmms = [dict(hmm_of(len(c)), stats=dict(emit_vcounts=np.asarray(c, dtype=np.float64))) for c in counts]
    return dict(label=label, groups=groups, group_size=np.array([len(g) for g in groups]), hmms=hmms)


def test_vb(ev):
    model = dict(omega=np.array([0.4, 0.6]), hmm=[hmm_of(2), hmm_of(3)], label=PRED,
                 groups=[np.flatnonzero(PRED == j) for j in range(2)])
    for result in (model, (model, np.zeros(0, dtype=np.int64))):      # vbh3m_remove_empty returns the pair
        out = ev.evaluate_run("vb", result, TRUE, num_hmm=2, num_sta=2)
        assert out["RI"] == pytest.approx(RI, rel=1e-15) and out["purity"] == pytest.approx(PURITY, rel=1e-15)
        assert out["K_select"] == 2 and out["S_select"].tolist() == [2, 3]
        assert (out["is_K_right"], out["is_K_big"], out["is_K_less"]) == (1.0, 0.0, 0.0)
        assert (out["is_S_right"], out["is_S_big"], out["is_S_less"]) == (0.5, 0.5, 0.0)
        assert "DI" not in out
    out = ev.evaluate_run("vb", model, TRUE, num_hmm=3, num_sta=4)
    assert (out["is_K_right"], out["is_K_big"], out["is_K_less"]) == (0.0, 0.0, 1.0) and out["is_S_less"] == 1.0


def test_ccfd_labels_come_from_cl_not_from_the_halo(ev):
    res = dict(ccfd_result=dict(icl=np.array([3, 5, 4]), halo=np.array([0, -1, 1, 0, -1, 1])), label=PRED,
               groups=[np.flatnonzero(PRED == j) for j in range(2)], hmms=[hmm_of(2)] * 3)
    out = ev.evaluate_run("ccfd", res, TRUE, num_hmm=2, num_sta=2)
    assert out["RI"] == pytest.approx(RI, rel=1e-15) and out["purity"] == pytest.approx(PURITY, rel=1e-15)
    assert out["K_select"] == 3 and (out["is_K_right"], out["is_K_big"], out["is_K_less"]) == (0.0, 1.0, 0.0)
    assert not any(k.startswith("is_S") or k == "S_select" for k in out)


def test_single_centre_gives_di_zero_without_a_kernel(ev):
    """evaluate_vbhem_jounarl.m:324-325: one centre, DI = 0; nothing is scored."""
    hmms, data = [hmm_of(2)] * 6, [[np.zeros((2, 2))]] * 6
    one = np.zeros(6, dtype=np.int64)
    res = dict(ccfd_result=dict(icl=np.array([2])), label=one, groups=[np.arange(6)], hmms=[hmm_of(2)])
    out = ev.evaluate_run("ccfd", res, TRUE, 2, 2, hmms=hmms, data=data, cpt_dist=True, device="cpu")
    assert out["DI"] == 0.0 and out["K_select"] == 1 and out["is_K_less"] == 1.0
    got = ev.dunn_index([hmm_of(2), None, hmm_of(3)], hmms, data, [np.arange(6), np.arange(0), np.arange(0)],
                        device="cpu")
    assert got["DI"] == 0.0 and got["kept"] == [0] and got["inter_vct"].size == 0
    with pytest.raises(ValueError, match="cpt_dist needs"):
        ev.evaluate_run("ccfd", res, TRUE, 2, 2, cpt_dist=True)
    with pytest.raises(ValueError, match="no cluster"):
        ev.dunn_index([None], hmms, data, [np.arange(6)], device="cpu")


def test_vhem_grid_means_and_the_empty_cluster(ev):
    """Cell A: the true labels, two groups, the second HMM with one state below 1e-3.
    Cell B: every subject in group 0 of three: K_select = 1, RI = 6 / 15 (the 6 pairs
    together in TRUE), purity = 3 / 6, its one HMM with three states."""
    A = vhem_cell(TRUE, 2, [[5.0, 5.0], [5.0, 1e-4]])
    B = vhem_cell(np.zeros(6, dtype=np.int64), 3, [[4.0, 4.0, 4.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    out = ev.evaluate_run("vhem", [[A, B]], TRUE, num_hmm=2, num_sta=2)
    assert out["RI"] == pytest.approx((1 + 6 / 15) / 2, rel=1e-15) and out["purity"] == pytest.approx(0.75, rel=1e-15)
    assert out["K_select"].tolist() == [[2, 1]]
    assert (out["is_K_right"], out["is_K_big"], out["is_K_less"]) == (0.5, 0.0, 0.5)
    assert [s.tolist() for s in out["S_select"][0]] == [[2, 1], [3]]
    assert (out["is_S_right"], out["is_S_big"], out["is_S_less"]) == (0.25, 0.5, 0.25)
    # one S in the grid: no S outputs (:379, :421)
    assert "is_S_right" not in ev.evaluate_run("vhem", [[A], [B]], TRUE, 2, 2)
    # the empty clusters are dropped before the index: one centre is left, DI = 0
    hmms, data = [hmm_of(2)] * 6, [[np.zeros((2, 2))]] * 6
    out = ev.evaluate_run("vhem", [[B, B]], TRUE, 2, 2, hmms=hmms, data=data, cpt_dist=True, device="cpu")
    assert out["DI"] == 0.0


def test_negative_criterion_rule(ev):
    """:437-448: exactly one negative entry becomes +inf; two stay."""
    one = ev.fix_negative_criterion([[-5.0, 3.0], [2.0, 4.0]])
    assert one[0, 0] == np.inf and one[1, 0] == 2.0
    two = ev.fix_negative_criterion([[-5.0, -3.0], [2.0, 4.0]])
    assert two.tolist() == [[-5.0, -3.0], [2.0, 4.0]]
    good = vhem_cell(PRED, 2, [[5.0, 5.0], [5.0, 5.0, 5.0]])
    bad = vhem_cell(np.zeros(6, dtype=np.int64), 2, [[4.0, 4.0], [0.0, 0.0]])
    grid = [[bad, bad], [good, bad]]
    for method in ("vhaic", "vhbic"):
        out = ev.evaluate_run(method, grid, TRUE, 2, 2, criterion=[[-5.0, 3.0], [2.0, 4.0]])
        assert out["select"] == (1, 0) and out["RI"] == pytest.approx(RI, rel=1e-15)
        assert out["K_select"] == 2 and out["S_select"].tolist() == [2, 3] and out["is_S_big"] == 0.5
        out = ev.evaluate_run(method, grid, TRUE, 2, 2, criterion=[[-5.0, -3.0], [2.0, 4.0]])
        assert out["select"] == (0, 0) and out["K_select"] == 1 and out["RI"] == pytest.approx(6 / 15, rel=1e-15)
    # the rule is for the VHEM criteria alone
    ppk = dict(label=PRED, group=[np.flatnonzero(PRED == j) for j in range(2)], group_size=np.array([2, 4]),
               hmms=[hmm_of(2), hmm_of(3)], ind_center=np.array([0, 5]))
    empty = dict(label=np.zeros(6, dtype=np.int64), group=[np.arange(6), np.arange(0)], group_size=np.array([6, 0]),
                 hmms=[hmm_of(1), None], ind_center=np.array([2, -1]))
    for method in ("scaic", "scbic"):
        out = ev.evaluate_run(method, [[empty, ppk], [ppk, ppk]], TRUE, 2, 2, criterion=[[-5.0, 3.0], [2.0, 4.0]])
        # :498: K_select = length(group_size), the empty cluster included
        assert out["select"] == (0, 0) and out["K_select"] == 2 and out["S_select"].tolist() == [1]
        out = ev.evaluate_run(method, [[empty, ppk], [ppk, ppk]], TRUE, 2, 2, criterion=[[7.0, 3.0], [2.0, 4.0]])
        assert out["select"] == (1, 0) and out["purity"] == pytest.approx(PURITY, rel=1e-15)
        assert (out["is_S_right"], out["is_S_big"], out["is_S_less"]) == (0.5, 0.5, 0.0)
    with pytest.raises(ValueError, match="criterion"):
        ev.evaluate_run("scaic", [[ppk]], TRUE, 2, 2)
    with pytest.raises(ValueError, match="method"):
        ev.evaluate_run("kmeans", [[ppk]], TRUE, 2, 2)


def scripted_h3m():
    """A fit as dic.fit_to_h3m gives it: three clusters of three states, cluster 1 with
    Nj = 0.5 (below 1), state 1 of cluster 2 with N = 1e-4 (below 1e-3); after
    vbh3m_remove_empty the labels are PRED."""
    rng = np.random.default_rng(8)
    hm = []
    for j in range(3):
        N = np.array([5.0, 1e-4 if j == 2 else 3.0, 4.0])
        eps, al = rng.uniform(0.5, 4.0, (3, 3)), rng.uniform(0.5, 4.0, 3)
        hm.append(dict(prior=al / al.sum(), trans=eps / eps.sum(1, keepdims=True),
                       pdf=[dict(mean=np.array([10.0 * j + s, 0.0]), cov=np.eye(2)) for s in range(3)],
                       N=N, N1=rng.uniform(0.1, 1, 3), M=rng.uniform(0.1, 3, (3, 3)),
                       varpar=dict(alpha=al, epsilon=eps, beta=rng.uniform(1, 2, 3), v=rng.uniform(4, 6, 3),
                                   m=rng.normal(size=(3, 2)), W=np.stack([np.eye(2)] * 3))))
    label = np.array([0, 2, 2, 0, 2, 2])
    return dict(hmm=hm, omega=np.array([0.5, 0.1, 0.4]), Z=rng.dirichlet(np.ones(3), size=6),
                L_elbo=-rng.uniform(1, 9, (6, 3)), Nj=np.array([2.5, 0.5, 3.0]), label=label,
                groups=[np.flatnonzero(label == j) for j in range(3)], group_size=np.array([2, 0, 4]), K=3)


def test_dic_prunes_the_selected_fit(ev):
    fit = scripted_h3m()
    out = ev.evaluate_run("dic", [[fit, fit], [fit, fit]], TRUE, 2, 3, criterion=[[9.0, 8.0], [7.5, -1.0]])
    assert out["select"] == (1, 1)                       # a negative DIC is a DIC like any other
    assert out["RI"] == pytest.approx(RI, rel=1e-15) and out["purity"] == pytest.approx(PURITY, rel=1e-15)
    assert out["K_select"] == 2 and out["S_select"].tolist() == [3, 2]
    assert (out["is_K_right"], out["is_S_right"], out["is_S_less"]) == (1.0, 0.5, 0.5)


def test_summarize(ev):
    runs = [dict(RI=0.5, purity=1.0, is_K_right=1.0, is_K_big=0.0, is_K_less=0.0, K_select=2, DI=2.0),
            dict(RI=1.0, purity=0.5, is_K_right=0.0, is_K_big=1.0, is_K_less=0.0, K_select=3, DI=4.0),
            dict(RI=0.75, purity=0.75, is_K_right=1.0, is_K_big=0.0, is_K_less=0.0, K_select=2, DI=6.0)]
    s = ev.summarize(runs)
    assert s["mean_RI"] == 0.75 and s["std_RI"] == pytest.approx(0.25, rel=1e-15)      # sqrt((1/16 + 1/16) / 2)
    assert s["mean_DI"] == 4.0 and s["std_DI"] == pytest.approx(2.0, rel=1e-15)
    assert s["mean_is_K_right"] == pytest.approx(2 / 3, rel=1e-15)
    assert s["std_is_K_right"] == pytest.approx(math.sqrt(1 / 3), rel=1e-15)         # N - 1 = 2 in the divisor
    assert s["K_is"] == [2, 3, 2] and s["RI"].tolist() == [0.5, 1.0, 0.75]
    assert "mean_is_S_right" not in s and "S_is" not in s
    one = ev.summarize(runs[:1])
    assert one["std_RI"] == 0.0 and one["mean_purity"] == 1.0                         # MATLAB's std of a scalar
    with pytest.raises(ValueError):
        ev.summarize([])


def test_sc_criteria_against_the_restatement(ev):
    rng = np.random.default_rng(4)
    Ks, Ss, dim = [1, 2, 4], [2, 3], 2
    LL = -rng.uniform(100, 900, (3, 2))
    for div_T in (0, 1):
        a, b = ev.sc_aic(LL, Ks, Ss, dim, 8.5, div_T), ev.sc_bic(LL, Ks, Ss, dim, 4321, 8.5, div_T)
        assert a.shape == b.shape == (3, 2)
        assert np.max(np.abs(a - dr.sc_aic(LL.tolist(), Ks, Ss, dim, 8.5, div_T)) / np.abs(a)) < 1e-15
        assert np.max(np.abs(b - dr.sc_bic(LL.tolist(), Ks, Ss, dim, 4321, 8.5, div_T)) / np.abs(b)) < 1e-15
    # by hand: K = 2, S = 3, dim = 2: (2 - 1) + 2 ((3 - 1) + 3 * 2 + 3 * 2 * 2) = 41 parameters
    assert ev.sc_num_pars(2, 3, 2) == 41
    assert ev.sc_aic([[-10.0]], 2, 3, 2, 5.0)[0, 0] == 20 + 82
    assert ev.sc_aic([[-10.0]], 2, 3, 2, 5.0, 1)[0, 0] == 4 + 82
    assert ev.sc_bic([[-10.0]], 2, 3, 2, 100, 5.0)[0, 0] == pytest.approx(20 + math.log(100) * 41, rel=1e-15)
