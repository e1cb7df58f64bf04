"""The batched 'wtkmeans' initialisation on the GPU (csrc/vbhem_wtk.hip): the kernels
against h3m.kmeans_pp / h3m.weighted_kmeans and against the host walker, the edge cases,
bitwise independence of a trial from the batch, wtkmeans_init_batch against wtkmeans_init,
and vbhem_h3m_c with init_engine="device" against "host".  Inputs, conditions and
tolerances: tests/wtk_ref.py."""
import numpy as np
import pytest

import wtk_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n,d,K,S", W.SHAPES)
def test_kernels_match_reference(vb, n, d, K, S):
    W.scenario_shape(W.DEVICE, n, d, K, S)
    X, w, j0, u = W.case(n, d, K, S)
    dev, host = (W.run_cluster(where, X, w, K, [j0], [u]) for where in (W.DEVICE, W.HOST))
    assert all(np.array_equal(dev[k], host[k]) for k in ("labels", "counts", "status", "iters"))


def test_singletons(vb):
    W.scenario_singletons(W.DEVICE)


def test_weightless_cluster_and_zero_weights(vb):
    W.scenario_weightless(W.DEVICE)


def test_emptied_cluster_is_reseeded(vb):
    W.scenario_emptied(W.DEVICE)


def test_bad_and_degenerate_are_contained(vb):
    """Nothing is provoked beyond a status code: the kernels end such a trial by their own
    tests on the inputs."""
    W.scenario_contained(W.DEVICE)


@pytest.mark.parametrize("R", [1, 3, 300])
def test_batching_bit_for_bit(vb, R):
    base = W.scenario_batching(W.DEVICE, R)
    assert (base["counts"].sum(1) == W.BLOCK + 1).all()


def test_limits_raise(vb):
    X, w = W.blobs(40, 2, 2, 1)
    W.run_cluster(W.DEVICE, X, w, 33, [0], [np.zeros(32)], expect=-2)
    W.run_cluster(W.DEVICE, np.zeros((40, 17)), w, 2, [0], [[0.5]], expect=-2)


def _options(vb, K, S, d, **over):
    return vb.default_options(K, S, d, **dict(dict(Nv=10, seed=1), **over))


def test_init_batch_equals_wtkmeans_init(vb):
    h3m = vb.h3m
    base = vb.synth_base_set(9, 3, 2, 2, vb.COV_FULL, seed=21)
    o = _options(vb, 4, 3, 2)
    pts = h3m.wtkmeans_points(base, "r0")
    seeds = [s for s in range(100, 160) if W.admissible(vb, base, o, s)][:12]
    want = [h3m.wtkmeans_init(base, o, s, pts) for s in seeds]
    got = h3m.wtkmeans_init_batch(base, o, seeds, DEV)
    for a, b in zip(got, want):
        W.posterior_equal(a, b, pts[0].shape[0], np.abs(pts[0]).max())
    for chunk in (1, 7):
        ch = h3m.wtkmeans_init_batch(base, o, seeds, DEV, chunk_trials=chunk)
        for a, b in zip(got, ch):
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("alpha", "eta", "epsilon", "m", "W"))
    # a larger set with d = 8: stage two on every cluster
    big = vb.synth_base_set(300, 4, 4, 8, vb.COV_FULL, seed=31)
    ob = _options(vb, 4, 3, 8, v0=10.0)
    sb = [s for s in range(10, 30) if W.admissible(vb, big, ob, s)][:3]
    pb = h3m.wtkmeans_points(big, "r0")
    for a, s in zip(h3m.wtkmeans_init_batch(big, ob, sb, DEV), sb):
        W.posterior_equal(a, h3m.wtkmeans_init(big, ob, s, pb), pb[0].shape[0], np.abs(pb[0]).max())
    with pytest.raises(ValueError, match="K <= 32"):
        h3m.wtkmeans_init_batch(base, _options(vb, 33, 2, 2), [1], DEV)


def test_points_batched_on_the_device(vb):
    base = vb.synth_base_set(40, 3, 4, 3, vb.COV_FULL, seed=30, ragged=True)
    a = vb.h3m.wtkmeans_points(base, "r0")
    b = vb.h3m.wtkmeans_points_batched(base, "r0", DEV)
    assert np.array_equal(a[0], b[0].cpu().numpy())
    np.testing.assert_allclose(b[1].cpu().numpy(), a[1], rtol=1e-13, atol=0)


def test_cluster_device_init_equals_host(vb):
    """vbhem_h3m_c on the planted HMMs, initmode 'wtkmeans', 5 trials: the same best trial
    and labels, every trial's bound within 1e-8 relative; 'auto' runs with the device
    engine (the other modes on the host)."""
    from vbhem_amd import cluster, vhem
    hmms, _ = vhem.planted_hmms(20, seed=3)
    base = vhem.hmms_to_h3m(hmms, "full")
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20, Nv=100,
               seed=1001, trials=5, max_iter=30, minDiff=1e-5, learn_hyps=0, initmode="wtkmeans")
    o = vb.default_options(2, 2, 2, **opt)
    host = cluster.vbhem_h3m_c(base, dict(o, init_engine="host"), DEV)
    plain = cluster.vbhem_h3m_c(base, o, DEV)
    dev = cluster.vbhem_h3m_c(base, dict(o, init_engine="device"), DEV)
    assert np.array_equal(host["LLall"], plain["LLall"])          # the default is the host path
    print("bounds host", host["LLall"], "device", dev["LLall"])
    assert dev["best"] == host["best"] and np.array_equal(dev["label"], host["label"])
    np.testing.assert_allclose(dev["LLall"], host["LLall"], rtol=1e-8)
    auto = cluster.vbhem_h3m_cluster(None, 2, 2, dict(opt, initmode="auto", trials=2, init_engine="device"), DEV,
                                     base=base)
    assert np.isfinite(auto["init_trials_LL"]).all()
