"""The batched 'gmmNew' initialisation on the GPU (csrc/vbhem_ghem.hip): the kernels against
h3m.gmm_mix_hier_em and against the host walker, trials that end at different E-steps, the
contained cases, bitwise independence of a trial from the batch, gmmnew_init_batch against
gmmnew_init, and vbhem_h3m_c with init_engine="device" against "host".  Inputs, conditions
and tolerances: tests/ghem_ref.py."""
import numpy as np
import pytest

import ghem_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _against_walker(X, C, full, T, iterations, j0, u, init=None):
    vs = G.samples_of(X.shape[0])
    dev, host = (G.run_fit(where, X, C, full, T, vs, iterations, j0, u, init) for where in (G.DEVICE, G.HOST))
    assert np.array_equal(dev["status"], host["status"]) and np.array_equal(dev["iters"], host["iters"])
    for r in range(len(dev["status"])):
        if host["status"][r] == G.OK:
            G.assert_close(dev, {k: host[k][r] for k in ("mxwt", "centres", "covars", "logp", "logpost")}, r, X, C)
    return dev


@pytest.mark.parametrize("n,d,T,full", G.SHAPES)
def test_kernels_match_reference_and_walker(vb, n, d, T, full):
    _, _, dev = G.scenario_shape(G.DEVICE, n, d, T, full)
    print("units", dev)
    X, C, j0, u, _ = G.case(n, d, T, full)
    _against_walker(X, C, full, T, 30, [j0], [u])


def test_large_tiles(vb):
    """n beyond 262,144: tiles of 1,024 points, four 256-point parts each in the E-step."""
    n, d, T, full = G.LARGE
    G.scenario_shape(G.DEVICE, n, d, T, full)
    X, C, j0, u, _ = G.case(n, d, T, full)
    _against_walker(X, C, full, T, 30, [j0], [u])


def test_trials_end_at_different_steps(vb):
    """One call whose trials stop after different numbers of E-steps, one of them at the
    cap: the done flags keep a finished trial as it ended."""
    n, T, cap = 256, 16, 10
    X, C = G.points(n, 16, True, 8, 91)
    seeds = (1, 2, 6)
    dr = [G.draws_of(s, n, T) for s in seeds]
    refs = [G.ref_fit(X, C, True, T, G.samples_of(n), cap, j, u) for j, u in dr]
    steps = [r["iters"][1] for r in refs]
    assert len(set(steps)) == 3 and max(steps) == cap, steps
    longer = G.ref_fit(X, C, True, T, G.samples_of(n), 30, *dr[int(np.argmax(steps))])
    assert longer["iters"][1] > cap
    dev = _against_walker(X, C, True, T, cap, [j for j, _ in dr], [u for _, u in dr])
    assert dev["iters"][:, 1].tolist() == steps
    for r, ref in enumerate(refs):
        G.assert_close(dev, ref, r, X, C)


def test_iterations(vb):
    G.scenario_iterations(G.DEVICE)


def test_init_centres(vb):
    G.scenario_init_centres(G.DEVICE)


def test_bad_trials_are_contained(vb):
    """Nothing is provoked beyond a status code: the kernels end such a trial by their own
    tests on the inputs and the pivots."""
    G.scenario_contained(G.DEVICE)


@pytest.mark.parametrize("R", [1, 3, 300])
def test_batching_bit_for_bit(vb, R):
    G.scenario_batching(G.DEVICE, R)


def test_logpost_is_optional(vb):
    G.scenario_optional(G.DEVICE)


def test_limits(vb):
    X, C = G.points(40, 2, True, 2, 1)
    G.run_fit(G.DEVICE, np.zeros((40, 17)), np.zeros((40, 17)), False, 2, 100.0, 3, [0], [[0.5]], expect=-2)
    G.run_fit(G.DEVICE, X, C, True, 33, 100.0, 3, [0], [np.zeros(32)], expect=-2)
    with pytest.raises(ValueError, match="T <= 32"):
        vb.h3m.gmm_mix_hier_em_batch(X, C, True, 33, 100.0, 3, [1], DEV)


def _points_of(base):
    bn = base.numpy()
    ns = bn["nstates"]
    return (np.concatenate([bn["centres"][i, :int(ns[i])] for i in range(base.N)]),
            np.concatenate([bn["covars"][i, :int(ns[i])] for i in range(base.N)]))


def test_init_batch_equals_gmmnew_init(vb):
    h3m = vb.h3m
    for covmode, mode, d, N, Sb in ((vb.COV_FULL, "r0", 2, 30, 3), (vb.COV_DIAG, "u0", 3, 30, 3),
                                    (vb.COV_FULL, "r0", 8, 150, 4)):
        base = vb.synth_base_set(N, 3, Sb, d, covmode, seed=21)
        o = vb.default_options(3, 3, d, Nv=10, seed=1, covmode=covmode, initopt_mode=mode, v0=d + 3.0)
        X, C = _points_of(base)
        full = covmode == vb.COV_FULL
        seeds = []
        for s in range(100, 130):
            try:
                G.ref_fit(X, C, full, 3, o["Nv"] * base.N, 30, *G.draws_of(s, X.shape[0], 3))
            except AssertionError:
                continue
            seeds.append(s)
        seeds = seeds[:4]
        assert len(seeds) == 4
        info = {}
        got = h3m.gmmnew_init_batch(base, o, seeds, DEV, info=info)
        assert info["replayed"] == []
        for a, s in zip(got, seeds):
            G.posterior_close(a, h3m.gmmnew_init(base, o, s), X.shape[0], X, C, full)
        for chunk in (1, 3):
            ch = h3m.gmmnew_init_batch(base, o, seeds, DEV, chunk_trials=chunk)
            for a, b in zip(got, ch):
                assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("alpha", "eta", "epsilon", "m", "W"))
    with pytest.raises(ValueError, match="S <= 32"):
        h3m.gmmnew_init_batch(base, vb.default_options(2, 33, 8, Nv=10, v0=11.0), [1], DEV)


def test_cluster_device_init_equals_host(vb):
    """vbhem_h3m_c on the planted HMMs, initmode 'gmmNew', 5 trials: the same best trial and
    labels, every trial's bound within 1e-8 relative."""
    from vbhem_amd import cluster, vhem
    hmms, _ = vhem.planted_hmms(20, seed=3)
    base = vhem.hmms_to_h3m(hmms, "full")
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20, Nv=100,
               seed=1001, trials=5, max_iter=30, minDiff=1e-5, learn_hyps=0, initmode="gmmNew")
    o = vb.default_options(2, 2, 2, **opt)
    host = cluster.vbhem_h3m_c(base, dict(o, init_engine="host"), DEV)
    plain = cluster.vbhem_h3m_c(base, o, DEV)
    dev = cluster.vbhem_h3m_c(base, dict(o, init_engine="device"), DEV)
    assert np.array_equal(host["LLall"], plain["LLall"])          # the default is the host path
    print("bounds host", host["LLall"], "device", dev["LLall"])
    assert dev["best"] == host["best"] and np.array_equal(dev["label"], host["label"])
    np.testing.assert_allclose(dev["LLall"], host["LLall"], rtol=1e-8)
