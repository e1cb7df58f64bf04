"""The batched GMM fit on the GPU (csrc/vbhmm_gmm.hip): the kernels against the host walker
of the same routines and against gmm_fit_randsample, bitwise independence of a fit from
its position, the launch chunking and KM, containment of ill-conditioned and bad fits,
init="device" of vbhmm_learn_batch against init="host", and vbhmm_em_batch(post=...).
Inputs, tolerances and the condition under which a fit may be left out: tests/gmm_ref.py.
"""
import numpy as np
import pytest

import gmm_ref as G
import vbhmm_em_batch_ref as R
from conftest import post_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(vb):
    """Every input of the CPU tests: (tag, subj, fits, dim)."""
    subj, fits, _ = G.demo_fits()
    out = [("demo", subj, fits, 2)]
    for dim in (3, 8):
        s, f = G.dim_fits(dim)
        out.append((f"dim{dim}", s, f, dim))
    s, f = G.edge_fits()
    out.append(("edge", s, f, 2))
    out.append(("planted", G.planted_subject(), [(0, 2, G.PLANTED_ROWS, 0.0), (0, 2, G.PLANTED_ROWS, 1e-10)], 2))
    bad_subj = [R.gaussian_subject(41, [30]), R.gaussian_subject(42, [2])]
    out.append(("bad", bad_subj, [(0, 2, np.array([0, 29]), 0.0), (0, 1, np.array([3]), 0.0),
                                  (1, 2, np.array([0, 1]), 0.0), (0, 2, np.array([4, 30]), 0.0),
                                  (0, 2, np.array([5, 20]), 0.0)], 2))
    return out


def test_kernels_match_walker_and_reference(vb):
    for tag, subj, fits, dim in _inputs(vb):
        hv, _ = G.hyper_vector(R.options(dim))
        dev = G.run_fits(subj, fits, dim, "device", hyper=hv)
        host = G.run_fits(subj, fits, dim, "host", hyper=hv)
        G.compare_runs(dev, host, post_err, tag)
        if tag != "bad":
            G.compare_with_reference(dev, subj, fits, post_err, tag)
    subj, fits, _ = G.demo_fits()
    d5 = G.run_fits(subj, fits[:6], 2, "device", max_iter=5)
    h5 = G.run_fits(subj, fits[:6], 2, "host", max_iter=5)
    G.compare_runs(d5, h5, post_err, "max_iter")
    assert d5[0]["status"] == G.MAX_ITER and d5[0]["iters"] == 5


@pytest.mark.parametrize("K,dim", G.CORNERS)
def test_kernels_match_walker_and_reference_at_the_bucket_corners(vb, K, dim):
    """K = KM, K * dim = 64 lanes, 8 rounds of the covariance loops: the device against the
    walker and against gmm_fit_randsample itself, no fit left out."""
    subj, fits = G.corner_fits(K, dim)
    hv, _ = G.hyper_vector(R.options(dim))
    dev = G.run_fits(subj, fits, dim, "device", hyper=hv)
    host = G.run_fits(subj, fits, dim, "host", hyper=hv)
    assert all(g["status"] < G.ILL for g in dev)
    G.compare_runs(dev, host, post_err, f"K{K}d{dim}")
    assert G.compare_with_reference(dev, subj, fits, post_err, f"K{K}d{dim}") == 0


def test_initial_posterior_at_the_full_bucket_with_a_diagonal_W0(vb):
    subj, fits = G.corner_fits(8, 8)
    opt = R.options(8, W0=R.diag_W0(8))
    hv, _ = G.hyper_vector(opt)
    got = G.run_fits(subj, fits, 8, "device", hyper=hv, KM=8)
    G.check_initial_posterior(got, subj, fits, opt, post_err, 8, "K8d8w")
    assert all(g["status"] < G.ILL for g in got)


def test_KM_independence_bitwise_at_dim_8(vb):
    subj, fits = G.corner_fits(4, 8)
    hv, _ = G.hyper_vector(R.options(8))
    four = G.run_fits(subj, fits, 8, "device", hyper=hv, KM=4)
    eight = G.run_fits(subj, fits, 8, "device", hyper=hv, KM=8)
    for i, (a, b) in enumerate(zip(four, eight)):
        assert a["status"] < G.ILL and G.same_bits(a, b, KM_differs=True), i


def test_initial_posterior_on_the_device(vb):
    subj, fits, _ = G.demo_fits()
    fits = fits[:24] + fits[72:]
    opt = R.options(W0=[0.001, 0.004])
    hv, _ = G.hyper_vector(opt)
    for KM in (4, 8):
        got = G.run_fits(subj, fits, 2, "device", hyper=hv, KM=KM)
        G.check_initial_posterior(got, subj, fits, opt, post_err, KM, f"KM{KM}")


def test_position_chunk_and_KM_independence_bitwise(vb):
    subj, fits, _ = G.demo_fits()
    hv, _ = G.hyper_vector(R.options())
    base = G.run_fits(subj, fits, 2, "device", hyper=hv)
    again = G.run_fits(subj, fits, 2, "device", hyper=hv)
    perm = np.random.default_rng(3).permutation(len(fits))
    shuffled = G.run_fits(subj, [fits[i] for i in perm], 2, "device", hyper=hv)
    rev = G.run_fits(subj, fits[::-1], 2, "device", hyper=hv)
    one = G.run_fits(subj, fits, 2, "device", hyper=hv, chunk_runs=1)
    seven = G.run_fits(subj, fits, 2, "device", hyper=hv, chunk_runs=7)
    eight = G.run_fits(subj, fits, 2, "device", hyper=hv, KM=8)
    for i in range(len(fits)):
        assert G.same_bits(base[i], again[i]), i
        assert G.same_bits(base[i], one[i]), i
        assert G.same_bits(base[i], seven[i]), i
        assert G.same_bits(base[i], rev[len(fits) - 1 - i]), i
        assert G.same_bits(base[i], eight[i], KM_differs=True), i
    for j, i in enumerate(perm):
        assert G.same_bits(base[i], shuffled[j]), i


def test_ill_conditioned_and_bad_fits_are_contained(vb):
    """The planted ill-conditioned fit and a bad fit between ordinary fits: the ordinary
    fits come out with the bits they have in a list without them.  Nothing is provoked
    beyond a status code: the kernel ends such a fit by its own test on the pivot."""
    demo, fits, _ = G.demo_fits()
    subj = [demo[0], G.planted_subject()[0], demo[1]]
    good = [(0, 2, fits[0][2], 0.0), (2, 3, [f for f in fits if f[0] == 1 and f[1] == 3][0][2], 0.0),
            (0, 2, fits[1][2], 0.0)]
    mixed = [good[0], (1, 2, G.PLANTED_ROWS, 0.0), good[1], (1, 2, np.array([0, 41]), 0.0), good[2]]
    hv, _ = G.hyper_vector(R.options())
    got = G.run_fits(subj, mixed, 2, "device", hyper=hv)
    alone = G.run_fits(subj, good, 2, "device", hyper=hv)
    assert got[1]["status"] == G.ILL and (got[1]["post_init"] == G.SENTINEL).all()
    assert G.untouched(got[3])
    for a, b in zip((got[0], got[2], got[4]), alone):
        assert a["status"] == G.CONVERGED and G.same_bits(a, b)


def test_gmm_fit_batch_and_random_gmm_batch(vb):
    """The Python entry points on the device: gmm_fit_batch against the check library's
    call (bit for bit), random_gmm_batch against _draw_inits."""
    from vbhem_amd import vbhmm, vbhmm_em as em
    subj, fits, _ = G.demo_fits()
    sb = vbhmm.SubjectBatch(subj, 2, DEV)
    hv, _ = G.hyper_vector(R.options())
    res, post = em.gmm_fit_batch(sb, fits, keep_lls=True, hyper=hv)
    chk = G.run_fits(subj, fits, 2, "device", hyper=hv)
    post = post.cpu().numpy()
    for i, (a, b) in enumerate(zip(res, chk)):
        assert a["status"] == G.STATUS[b["status"]] and a["iters"] == b["iters"], i
        assert np.array_equal(a["lls"], b["lls"]), i
        if b["status"] < G.ILL:
            assert all(np.array_equal(a[k], b[k]) for k in ("prior", "mean", "cov")), i
            assert np.array_equal(post[i], b["post_init"]), i
        else:
            assert a["prior"] is None and a["cov"] is None
    opt = R.options(numtrials=12)
    info = {}
    one = vbhmm.SubjectBatch([R.demo_subjects()[2]], 2, DEV)
    got = em.random_gmm_batch(one, [1, 2, 3], opt, info=info)
    assert info["rounds"] == 2 and info["regularised"] == {(0, 2): [3], (0, 3): [10]}
    for K in (1, 2, 3):
        want = em._draw_inits(one.datas[0], K, opt, None)
        assert len(got[(0, K)]) == len(want)
        for t, (a, b) in enumerate(zip(got[(0, K)], want)):
            for k in ("prior", "mean", "cov"):
                assert post_err(a[k], b[k]) < 1e-8, (K, t, k)


@pytest.fixture(scope="module")
def inits(vb):
    from vbhem_amd.vbhmm_em import vbhmm_learn_batch
    subj = R.demo_subjects()
    opt = R.options(numtrials=4)
    plain = vbhmm_learn_batch(subj, [1, 2, 3], opt, device=DEV, engine="fused")
    host = vbhmm_learn_batch(subj, [1, 2, 3], opt, device=DEV, engine="fused", init="host")
    dev = vbhmm_learn_batch(subj, [1, 2, 3], opt, device=DEV, engine="fused", init="device")
    return subj, plain, host, dev


def test_learn_batch_inits_agree(vb, inits):
    subj, _, (hh, Lh), (hd, Ld) = inits
    np.testing.assert_allclose(Ld, Lh, rtol=1e-9)
    for s, (a, b) in enumerate(zip(hh, hd)):
        assert a["model_bestK"] == b["model_bestK"], s
        np.testing.assert_allclose(b["model_LL"], a["model_LL"], rtol=1e-9)
        for ka, kb in zip(a["model_all"], b["model_all"]):
            np.testing.assert_allclose(kb["trials_LL"], ka["trials_LL"], rtol=1e-9)
        assert len(b["gamma"]) == len(subj[s])


def test_init_host_is_the_existing_fused_path_bit_for_bit(vb, inits):
    _, (hp, Lp), (hh, Lh), _ = inits
    assert np.array_equal(Lp, Lh)
    for a, b in zip(hp, hh):
        assert np.array_equal(a["model_LL"], b["model_LL"])
        for ka, kb in zip(a["model_all"], b["model_all"]):
            assert np.array_equal(ka["trials_LL"], kb["trials_LL"])
            for k in R.POST_KEYS:
                assert np.array_equal(ka["varpar"][k], kb["varpar"][k]), k


def test_injected_gmms_win_under_init_device(vb):
    from vbhem_amd.vbhmm_em import vbhmm_learn
    data = R.demo_subjects()[0]
    opt = R.options(numtrials=3)
    g = {2: R.gmm_trials(data, 2, 2, seed=7)}
    a = vbhmm_learn(data, [1, 2], opt, device=DEV, gmms=g, engine="fused")
    b = vbhmm_learn(data, [1, 2], opt, device=DEV, gmms=g, engine="fused", init="device")
    assert np.array_equal(a["model_LL"], b["model_LL"])
    for ka, kb in zip(a["model_all"], b["model_all"]):
        assert np.array_equal(ka["trials_LL"], kb["trials_LL"])


def test_em_batch_takes_prepacked_posteriors(vb):
    import torch
    from vbhem_amd import vbhmm, vbhmm_em as em
    subj, runs = R.runs_a()
    runs = runs[:27]
    opt = R.options()
    sb = vbhmm.SubjectBatch(subj, 2, DEV)
    ref = em.vbhmm_em_batch(sb, runs, opt, keep_LLs=True)
    copt, _ = em.vbhmm_clip_hyps(opt)
    post = np.stack([em.pack_posterior(em.vbhmm_init([sb.X[s]], K, copt, g), K, 4, 2) for s, K, g in runs])
    got = em.vbhmm_em_batch(sb, [(s, K, None) for s, K, _ in runs], opt, keep_LLs=True,
                            post=torch.from_numpy(post).to(DEV))
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a["LL"] == b["LL"] and a["iters"] == b["iters"] and a["status"] == b["status"], i
        assert np.array_equal(a["LLs"], b["LLs"]), i
        for k in R.POST_KEYS:
            assert np.array_equal(a["varpar"][k], b["varpar"][k]), (i, k)
            assert np.array_equal(a["varpar_estep"][k], b["varpar_estep"][k]), (i, k)
