"""Helpers shared by the tests of the batched hyperparameter learner
(test_hyp_batch.py, test_em_trials_hyp_gpu.py)."""
import numpy as np


def trial_posts(cs, R, seed):
    """R cluster posteriors over the same base set: the case's posterior and R-1
    re-perturbed copies (the recipe of tests/test_em_trials_dev_gpu.py::_trial_posts)."""
    posts = [cs["P"].copy()]
    for r in range(1, R):
        P = cs["P"].copy()
        rng = np.random.default_rng(seed * 100 + r)
        P.epsilon = P.epsilon * rng.uniform(0.3, 1.7, P.epsilon.shape)
        P.eta = P.eta * rng.uniform(0.3, 1.7, P.eta.shape)
        P.m = P.m + rng.normal(0.0, 0.5, P.m.shape)
        P.alpha = P.alpha * rng.uniform(0.5, 1.5, P.alpha.shape)
        posts.append(P)
    return posts


def trial_opts(opt, R, seed):
    """Per-trial hyperparameters: trial 0 keeps ``opt``; trial r draws, from
    default_rng(seed 1000 + r): alpha0, eta0, epsilon0, lambda0 x exp(U(-1, 1)),
    v0 + U(0, 3), W0 x exp(U(-0.5, 0.5)) per element, m0 + N(0, 0.3)."""
    out = [dict(opt)]
    for r in range(1, R):
        rng = np.random.default_rng(seed * 1000 + r)
        o = dict(opt)
        for h in ("alpha0", "eta0", "epsilon0", "lambda0"):
            o[h] = float(opt[h]) * float(np.exp(rng.uniform(-1.0, 1.0)))
        o["v0"] = float(opt["v0"]) + float(rng.uniform(0.0, 3.0))
        W0 = np.asarray(opt["W0"], dtype=float)
        W0n = W0 * np.exp(rng.uniform(-0.5, 0.5, W0.shape))
        o["W0"] = float(W0n) if W0n.ndim == 0 else W0n
        m0 = np.asarray(opt["m0"], dtype=float).reshape(-1)
        o["m0"] = m0 + rng.normal(0.0, 0.3, m0.shape)
        out.append(o)
    return out
