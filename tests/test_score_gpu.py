"""Scoring sequences under HMMs on the GPU (score.py over hmm_score_kernel):
parity with the numpy restatement (tests/score_ref.py) at the bounds of
tests/test_score.py -- log-likelihoods at RTOL_PAIRS under conftest.stat_err,
Viterbi paths exactly -- and agreement between the entry points."""
import os

import numpy as np
import pytest
import torch

import score_ref as sr
from conftest import GOLDEN_DIR, RTOL_PAIRS, stat_err

pytestmark = pytest.mark.gpu
MARGIN = 1e-6
DEV = "cuda:0"


@pytest.fixture(scope="module")
def score(vb, capi_lib):
    from vbhem_amd import score as mod
    return mod


def split_paths(path_row, data, d):
    lens = [int(np.asarray(a).reshape(-1, d).shape[0]) for a in data]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [path_row[off[n]:off[n + 1]] for n in range(len(data))]


def check_against(score, hmms, data, d, ref):
    assert sr.outside_denormal_zone(ref["logrho"]) and ref["margin"] > MARGIN
    hset = score.HmmSet(hmms, DEV)
    ll = score.ll_matrix(hset, data, normalize=False).cpu().numpy()
    lln = score.ll_matrix(hset, data).cpu().numpy()
    path, vll = score.viterbi(hset, data)
    path, vll = path.cpu().numpy(), vll.cpu().numpy()
    print("ll err", stat_err(ll, ref["ll"]), "viterbi ll err", stat_err(vll, ref["vll"]))
    assert stat_err(ll, ref["ll"]) < RTOL_PAIRS
    assert stat_err(lln, ref["lln"]) < RTOL_PAIRS
    assert stat_err(vll, ref["vll"]) < RTOL_PAIRS
    for h in range(len(hmms)):
        got = split_paths(path[h], data, d)
        for n in range(len(data)):
            assert np.array_equal(got[n], ref["paths"][h][n]), (h, n)


@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_gpu_matches_restatement(score, shape):
    K, d, diag = shape
    hmms, data = sr.make_case(K, d, diag)
    check_against(score, hmms, data, d, sr.reference(K, d, diag))


@pytest.mark.parametrize("H", [1, 3, 17])
@pytest.mark.parametrize("N", [1, 129, 300])
def test_gpu_blocks_and_sets(score, N, H):
    """A partial block, one sequence past a block boundary, several blocks; 1, 3, 17 HMMs."""
    hmms, data = sr.make_case(3, 2, False, N=N, H=H)
    check_against(score, hmms, data, 2, sr.reference(3, 2, False, N=N, H=H))


def test_scorecheck_device_entry(score):
    """The C-ABI through plain host arrays (tests/scorecheck): the kernels themselves."""
    sc = sr.load_scorecheck()
    hmms, data = sr.make_case(9, 3, False)
    ref = sr.reference(9, 3, False)
    rc, ll, vll, paths = sr.run_scorecheck(sc, score.pack_hmms(hmms), data, 3, device=True)
    assert rc == 0
    assert stat_err(ll, ref["ll"]) < RTOL_PAIRS and stat_err(vll, ref["vll"]) < RTOL_PAIRS
    assert all(np.array_equal(paths[h][n], ref["paths"][h][n]) for h in range(3) for n in range(6))


# ----------------------------------------------------------------------------
# agreement between the entry points
# ----------------------------------------------------------------------------
def base_set_hmms(b):
    """The HMM dicts of a packed BaseSet (numpy())."""
    out = []
    for i, K in enumerate(b["nstates"]):
        out.append(dict(prior=b["prior"][i, :K], trans=b["A"][i, :K, :K],
                        pdf=[dict(mean=b["centres"][i, k], cov=b["covars"][i, k]) for k in range(K)]))
    return out


def test_base_set_equals_dicts_bitwise(vb, score):
    base = vb.synth_base_set(100, 4, 2, 2, vb.COV_FULL, seed=1002, ragged=True)
    assert len(set(base.nstates.tolist())) > 1
    rng = np.random.default_rng(0)
    data = [rng.uniform(0, 5, (T, 2)) for T in rng.integers(1, 9, 40)]
    a = score.ll_matrix(score.HmmSet(base, DEV), data)
    b = score.ll_matrix(score.HmmSet(base_set_hmms(base.numpy()), DEV), data)
    assert a.shape == (100, 40) and torch.equal(a, b)
    # against the restatement too, for three of the bases
    for i in (0, 1, 57):
        ref, _ = sr.vbhmm_ll(base_set_hmms(base.numpy())[i], data)
        assert stat_err(a[i].cpu().numpy(), ref) < RTOL_PAIRS


def test_single_hmm_equals_batched_row_bitwise(score):
    hmms, data = sr.make_case(5, 3, False)
    full = score.ll_matrix(score.HmmSet(hmms, DEV), data).cpu().numpy()
    for h, hmm in enumerate(hmms):
        ll, err = score.vbhmm_ll(hmm, data)
        assert np.array_equal(ll, full[h], equal_nan=True) and not err.any()
    paths = score.vbhmm_map_state(hmms[0], data)
    ref = sr.reference(5, 3, False)
    assert all(np.array_equal(p, r) for p, r in zip(paths, ref["paths"][0]))
    assert all(p.dtype == np.int64 for p in paths)


def packed_base_set(p):
    from vbhem_amd.h3m import BaseSet
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return BaseSet(t(p["nstates"]), t(p["prior"]), t(p["trans"]), t(p["mean"]), t(p["cov"]),
                   torch.ones(len(p["nstates"]), dtype=torch.float64), p["covmode"])


def test_poisoned_padding_changes_nothing(score):
    hmms, data = sr.make_case(5, 3, False)
    packed = score.pack_hmms(hmms)
    clean = score.HmmSet(packed_base_set(packed), DEV)
    bad = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in packed.items()}
    for h, K in enumerate(bad["nstates"]):
        bad["mean"][h, K:] = np.nan
        bad["cov"][h, K:] = np.nan
        bad["prior"][h, K:] = 0.5
        bad["trans"][h, K:, :] = 0.5
        bad["trans"][h, :, K:] = 0.5
    assert np.isnan(bad["mean"]).any() and np.isnan(bad["cov"]).any()
    poisoned = score.HmmSet(packed_base_set(bad), DEV)
    assert torch.equal(score.ll_matrix(clean, data, False), score.ll_matrix(poisoned, data, False))
    pa, va = score.viterbi(clean, data)
    pb, vb_ = score.viterbi(poisoned, data)
    assert torch.equal(pa, pb) and torch.equal(va, vb_)
    ref = sr.reference(5, 3, False)
    assert stat_err(score.ll_matrix(poisoned, data, False).cpu().numpy(), ref["ll"]) < RTOL_PAIRS


def test_not_positive_definite_is_rejected_and_consumed(score):
    from vbhem_amd import _capi
    rng = np.random.default_rng(8)
    hmms = [sr.make_hmm(rng, 3, 2, False) for _ in range(3)]
    data = sr.sample_data(rng, hmms, [3, 5], 2)
    good = score.ll_matrix(score.HmmSet(hmms, DEV), data).cpu().numpy()
    broken = [dict(h, pdf=[dict(p) for p in h["pdf"]]) for h in hmms]
    broken[1]["pdf"][2]["cov"] = np.array([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(_capi.VbhemError, match="HMM 1 state 2 is not positive definite"):
        score.HmmSet(broken, DEV)
    # the error was consumed: a torch launch and a correct call still succeed
    s = torch.arange(8, device=DEV, dtype=torch.float64).sum()
    torch.cuda.synchronize()
    assert float(s) == 28.0
    again = score.ll_matrix(score.HmmSet(hmms, DEV), data).cpu().numpy()
    assert np.array_equal(good, again)


# ----------------------------------------------------------------------------
# demo fixations under hand-written face-scale HMMs
# ----------------------------------------------------------------------------
FACE_HMMS = [
    dict(prior=[0.6, 0.3, 0.1], trans=[[0.5, 0.3, 0.2], [0.2, 0.6, 0.2], [0.3, 0.3, 0.4]],
         pdf=[dict(mean=[256.0, 192.0], cov=[[900.0, 100.0], [100.0, 1600.0]]),
              dict(mean=[230.0, 160.0], cov=[[400.0, -50.0], [-50.0, 400.0]]),
              dict(mean=[280.0, 230.0], cov=[[2500.0, 0.0], [0.0, 900.0]])]),
    dict(prior=[0.2, 0.5, 0.3], trans=[[0.7, 0.2, 0.1], [0.1, 0.7, 0.2], [0.25, 0.15, 0.6]],
         pdf=[dict(mean=[250.0, 170.0], cov=[[1600.0, 300.0], [300.0, 900.0]]),
              dict(mean=[262.0, 215.0], cov=[[900.0, 0.0], [0.0, 2500.0]]),
              dict(mean=[240.0, 250.0], cov=[[3600.0, -400.0], [-400.0, 1600.0]])]),
    dict(prior=[0.34, 0.33, 0.33], trans=[[0.4, 0.35, 0.25], [0.3, 0.45, 0.25], [0.2, 0.3, 0.5]],
         pdf=[dict(mean=[256.0, 192.0], cov=[2500.0, 2500.0]),
              dict(mean=[220.0, 200.0], cov=[900.0, 1600.0]),
              dict(mean=[290.0, 185.0], cov=[1600.0, 400.0])]),
]


def test_demo_fixations(score):
    z = np.load(os.path.join(GOLDEN_DIR, "demo_fixations.npz"))
    off, x, subject = z["offsets"], z["x"], z["subject"]
    data = [x[off[n]:off[n + 1]] for n in range(len(off) - 1)]
    ref_ll = np.array([sr.vbhmm_ll(h, data)[0] for h in FACE_HMMS])
    refs = [sr.vbhmm_map_state(h, data) for h in FACE_HMMS]
    lr = np.concatenate([sr.emissions(h, x)[1].reshape(-1) for h in FACE_HMMS])
    assert sr.outside_denormal_zone(lr) and min(r[2] for r in refs) > MARGIN
    hset = score.HmmSet(FACE_HMMS, DEV)
    assert hset.covmode == 1
    ll = score.ll_matrix(hset, data).cpu().numpy()
    assert stat_err(ll, ref_ll) < RTOL_PAIRS
    path, vll = score.viterbi(hset, data)
    path = path.cpu().numpy()
    assert stat_err(vll.cpu().numpy(), np.array([r[1] for r in refs])) < RTOL_PAIRS
    for h in range(3):
        got = split_paths(path[h], data, 2)
        assert all(np.array_equal(g, r) for g, r in zip(got, refs[h][0]))
    # sequences are stored subject by subject: the per-subject means
    subs = sorted(set(subject.tolist()))
    assert (np.diff(subject) >= 0).all()
    by_subject = [[data[n] for n in np.nonzero(subject == s)[0]] for s in subs]
    m = score.mean_ll(hset, by_subject).cpu().numpy()
    want = np.stack([[ref_ll[h, subject == s].mean() for s in subs] for h in range(3)])
    assert m.shape == (3, len(subs)) and stat_err(m, want) < RTOL_PAIRS


# ----------------------------------------------------------------------------
# KL
# ----------------------------------------------------------------------------
def test_kld(score):
    rng = np.random.default_rng(21)
    h1, h2, h3 = (sr.make_hmm(rng, K, 2, False) for K in (3, 2, 4))
    data = sr.sample_data(rng, [h1], [4, 7, 1, 9], 2)
    kld, ll1, ll2, _ = score.vbhmm_kld(h1, h1, data, device=DEV)
    assert kld == 0.0 and np.array_equal(ll1, ll2)
    kld, ll1, ll2, samples = score.vbhmm_kld(h1, h2, [200, 10], seed=3, device=DEV)
    assert len(samples) == 200 and all(s.shape == (10, 2) for s in samples)
    r1, r2 = sr.vbhmm_ll(h1, samples)[0], sr.vbhmm_ll(h2, samples)[0]
    bound = 1e-10 * max(np.abs(r1).max(), np.abs(r2).max())
    print("kld", kld, "ref", np.mean(r1 - r2), "bound", bound)
    assert abs(kld - np.mean(r1 - r2)) < bound
    assert stat_err(ll1, r1) < RTOL_PAIRS and stat_err(ll2, r2) < RTOL_PAIRS
    assert kld > 0
    # unnormalised option
    k0, a0, _, _ = score.vbhmm_kld(h1, h2, samples, opt="", device=DEV)
    assert stat_err(a0, ll1 * 10) < RTOL_PAIRS and abs(k0 - 10 * kld) < 10 * bound
    # the matrix: zero diagonal, entries = the pairwise calls
    hs = [h1, h2, h3]
    sets = [score.vbhmm_random_sample(h, 6, 30 + 5 * i, seed=40 + i)[1] for i, h in enumerate(hs)]
    D = score.kld_matrix(hs, sets, device=DEV).cpu().numpy()
    assert D.shape == (3, 3) and (np.diag(D) == 0).all()
    for i in range(3):
        for j in range(3):
            kij, li, _, _ = score.vbhmm_kld(hs[i], hs[j], sets[i], device=DEV)
            assert abs(D[i, j] - kij) <= 1e-10 * np.abs(li).max(), (i, j)


# ----------------------------------------------------------------------------
# the zero floor on the device (fp64 denormals are kept)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["all-floored", "one-floored"])
def test_zero_floor_on_device(score, single):
    hmm, data = sr.floor_case(single)
    ref, _ = sr.vbhmm_ll(hmm, data, "")
    ll = score.ll_matrix(score.HmmSet([hmm], DEV), data, normalize=False).cpu().numpy()[0]
    print("floor", ll, ref)
    assert np.isfinite(ll).all() and stat_err(ll, ref) < RTOL_PAIRS
    if not single:
        assert abs(ll[2] - np.log(4.94e-323)) < 1.0


def test_ieee_cases_on_device(score):
    hmm = dict(prior=np.zeros(2), trans=np.array([[0.5, 0.5], [0.2, 0.8]]),
               pdf=[dict(mean=np.zeros(2), cov=np.eye(2)), dict(mean=np.ones(2), cov=np.eye(2))])
    data = [np.array([[0.1, 0.2]]), np.zeros((0, 2)), np.array([[0.1, 0.2], [0.3, 0.1]])]
    ll, err = score.vbhmm_ll(hmm, data, device=DEV)
    assert ll[0] == -np.inf and np.isnan(ll[1]) and np.isnan(ll[2])
    assert list(err) == [True, False, False]
    ll0, _ = score.vbhmm_ll(hmm, data, opt="", device=DEV)
    assert ll0[0] == -np.inf and ll0[1] == 0.0
