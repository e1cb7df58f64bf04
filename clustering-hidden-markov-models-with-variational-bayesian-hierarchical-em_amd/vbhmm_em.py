"""VB-HMM learning of the base HMMs (config C1).

The upstream stage that produces the HMMs VBHEM clusters:
``vbhmm_learn_batch`` -> ``vbhmm_learn`` -> ``vbhmm_em`` -> ``vbhmm_fb`` ->
``vbhmm_fb_mex`` (src/hmm/).  The forward-backward runs on the GPU through the
C-ABI (:func:`vbhmm.vbhmm_fb`, one lane per sequence); the per-iteration
statistics, lower bound and M-step are O(K^2 + K dim^2 + total fixations) host
work, restated here from:

* vbhmm_em.m:112-414  the EM loop (E-step :133-246, bound :251-275, convergence
  and NaN handling :277-349, M-step :352-408) and the output model :426-491;
* vbhmm_em_lb.m:74-257  the lower bound, :260-400 its derivatives with respect to
  the (transformed) hyperparameters;
* vbhmm_em_hyp.m + get_hypinfo.m  hyperparameter learning (``learn_hyps``): the
  bound maximised over the transformed hyperparameters with minimize_new.m's BFGS
  (:func:`hyp.minimize`), every evaluation an EM run from the trial's HMM
  ('inithmm', vbhmm_init.m:154-161) with the derivatives at its last E-step;
  vbhmm_learn.m:482-552 runs it on each unique random trial (uniqueLL.m);
* vbhmm_init.m:122-204  the initial posterior from a GMM; :27-43 the K = 1 and
  N <= K special cases of the 'random' mode;
* vbhmm_clip_hyps.m:20-85, vbhmm_learn.m:252-310 (defaults), :440-480 (random
  trials, best LL), :367-405 (model selection over K with +gammaln(K+1));
* vbhmm_learn_batch.m (one vbhmm_learn per subject);
* vbhmm_remove_empty.m (states with N < thresh removed, as vbhem_h3m_cluster.m:116-134).

The 'random' initialisation fits a GMM with MATLAB's ``gmdistribution.fit``
(Statistics Toolbox, 'Start' 'randSample', TolFun 1e-5; vbhmm_init.m:59-60),
which is not part of the reference.  :func:`gmm_fit_randsample` restates that
published algorithm (random data rows as means, uniform weights, diagonal
covariances of the data variances, EM until the relative log-likelihood change
is below 1e-5); MATLAB's random stream cannot be reproduced, so the draws come
from a seeded numpy generator and parity tests inject the same GMM into both
sides.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
from scipy.special import digamma, gammaln

from . import vbhmm


# ----------------------------------------------------------------------------
# options
# ----------------------------------------------------------------------------
def vbhmm_default_options(dim: int, **over) -> dict:
    """vbhmm_learn.m:252-310 (the fields the EM loop reads)."""
    defmu = {2: [256.0, 192.0], 3: [256.0, 192.0, 150.0]}.get(dim, [0.0] * dim)
    opt = dict(alpha0=0.1, mu0=defmu, W0=0.005, beta0=1.0, v0=5.0, epsilon0=0.1,
               initmode="random", numtrials=50, maxIter=100, minDiff=1e-5, seed=None,
               fix_clusters=0, fix_cov=None, verbose=0, learn_hyps=0, calc_LLderiv=0,
               minimizer="minimize-bfgs", hyp_length=100, sortclusters="f")
    opt["hyps_max"] = dict(alpha0=1.0686e13, epsilon0=1.0686e13, v0=1e4, beta0=1.0686e13,
                           W0=1.0686e13)
    opt["hyps_min"] = dict(alpha0=1.0686e-13, epsilon0=1.0686e-13, v0=2.0612e-09 + dim - 1,
                           beta0=1.0686e-13, W0=1.0686e-13)
    opt.update(over)
    opt["mu0"] = np.asarray(opt["mu0"], dtype=np.float64).reshape(-1)
    if opt["v0"] <= dim - 1:
        raise ValueError("v0 not large enough...should be > D-1")  # vbhmm_learn.m:319-321
    return opt


def vbhmm_clip_hyps(opt: dict):
    """vbhmm_clip_hyps.m:20-85: clip each hyperparameter into [min, max];
    returns (clipped options, clipped flags: +1 at max, -1 at min)."""
    out = dict(opt)
    clipped = {}
    for name in ("alpha0", "epsilon0", "v0", "beta0", "W0"):
        val = np.array(opt[name], dtype=np.float64, ndmin=1)
        flag = np.zeros(val.size)
        hi, lo = opt["hyps_max"][name], opt["hyps_min"][name]
        flag[val >= hi] = +1
        val = np.where(val >= hi, hi, val)
        flag[val <= lo] = -1
        val = np.where(val <= lo, lo, val)
        out[name] = val if np.ndim(opt[name]) else float(val[0])
        clipped[name] = flag
    return out, clipped


# ----------------------------------------------------------------------------
# initialisation
# ----------------------------------------------------------------------------
def gmm_fit_randsample(X: np.ndarray, K: int, rng: np.random.Generator, tolfun: float = 1e-5,
                       max_iter: int = 100, reg: float = 0.0, trace: Optional[list] = None) -> dict:
    """Stand-in for MATLAB gmdistribution.fit(X, K, 'Start', 'randSample',
    'Options', struct('TolFun', 1e-5)) (vbhmm_init.m:59-60): K random rows of X
    as means, uniform proportions, every covariance diag(var(X)); full-covariance
    EM until |dLL| <= TolFun * |LL|.  Returns dict(prior [K], mean [K][dim],
    cov [K][dim][dim]).  ``trace`` (a list) receives every iteration's log-likelihood."""
    N, dim = X.shape
    mu = X[rng.choice(N, K, replace=False)].copy()
    var = X.var(axis=0, ddof=1) if N > 1 else np.ones(dim)
    cov = np.repeat(np.diag(var)[None], K, axis=0)
    pi = np.full(K, 1.0 / K)
    last = -np.inf
    for _ in range(max_iter):
        logp = np.zeros((N, K))
        for k in range(K):
            L = np.linalg.cholesky(cov[k] + reg * np.eye(dim))
            z = np.linalg.solve(L, (X - mu[k]).T)
            logp[:, k] = (np.log(pi[k]) - 0.5 * (z * z).sum(0) - np.log(np.diag(L)).sum()
                          - 0.5 * dim * np.log(2 * np.pi))
        mx = logp.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(logp - mx).sum(1))
        ll = lse.sum()
        if trace is not None:
            trace.append(float(ll))
        post = np.exp(logp - lse[:, None])
        nk = post.sum(0) + 1e-300
        pi = nk / N
        mu = (post.T @ X) / nk[:, None]
        for k in range(K):
            d = X - mu[k]
            cov[k] = (d * post[:, k:k + 1]).T @ d / nk[k] + reg * np.eye(dim)
            cov[k] = 0.5 * (cov[k] + cov[k].T)
        if abs(ll - last) <= tolfun * abs(ll):
            break
        last = ll
    return dict(prior=pi, mean=mu, cov=cov)


def random_gmm(data: Sequence[np.ndarray], K: int, rng: np.random.Generator) -> dict:
    """The 'random' initmode's GMM (vbhmm_init.m:27-91): one Gaussian for K = 1,
    the data points themselves when N <= K, else a GMM fit."""
    X = np.concatenate([np.asarray(a, dtype=np.float64) for a in data], axis=0)
    N, dim = X.shape
    if K == 1:
        return dict(prior=np.ones(1), mean=X.mean(0, keepdims=True),
                    cov=np.cov(X.T, ddof=1).reshape(1, dim, dim))
    if N <= K:
        tmp = np.concatenate([np.ones(N), 1e-6 * np.ones(K - N)])
        mean = np.concatenate([X, np.zeros((K - N, dim))])
        v = X.var(axis=0, ddof=1) if N > 1 else np.ones(dim)
        return dict(prior=tmp / tmp.sum(), mean=mean,
                    cov=np.repeat((np.mean(v) * np.eye(dim))[None], K, axis=0))
    try:
        return gmm_fit_randsample(X, K, rng)
    except np.linalg.LinAlgError:  # ill-conditioned: regularised fit (vbhmm_init.m:63-70)
        return gmm_fit_randsample(X, K, rng, reg=1e-10)


def vbhmm_init(data: Sequence[np.ndarray], K: int, opt: dict, gmm: dict) -> dict:
    """vbhmm_init.m:122-204: the initial variational posterior from a GMM
    (prior [K], mean [K][dim], cov [K][dim][dim]), or ('inithmm') an HMM's own."""
    X = np.concatenate([np.asarray(a, dtype=np.float64) for a in data], axis=0)
    N, dim = X.shape
    if len(opt["mu0"]) != dim:
        raise ValueError(f"vbopt.mu0 should have dimension D={dim}")
    W0 = np.asarray(opt["W0"], dtype=np.float64)
    W0m = float(W0) * np.eye(dim) if W0.size == 1 else np.diag(W0.reshape(-1))
    W0inv = np.linalg.inv(W0m)
    beta0, v0, m0 = float(opt["beta0"]), float(opt["v0"]), opt["mu0"]
    W0mode = "iid" if W0.size == 1 else "diag"
    if opt.get("initmode") == "inithmm":  # vbhmm_init.m:154-161: the HMM's own posterior
        vp = opt["inithmm"]["varpar"]
        return dict(alpha=np.array(vp["alpha"], float), epsilon=np.array(vp["epsilon"], float),
                    beta=np.array(vp["beta"], float), v=np.array(vp["v"], float),
                    m=np.array(vp["m"], float), W=np.array(vp["W"], float), W0inv=W0inv,
                    W0mode=W0mode)
    Nk = N * np.asarray(gmm["prior"], dtype=np.float64).reshape(-1)
    Nk2 = np.full(K, N / K)
    xbar = np.asarray(gmm["mean"], dtype=np.float64).reshape(K, dim)
    S = np.asarray(gmm["cov"], dtype=np.float64).reshape(K, dim, dim)
    alpha = opt["alpha0"] + Nk2
    epsilon = np.repeat((opt["epsilon0"] + Nk2)[None, :], K, axis=0)
    beta = beta0 + Nk
    v = v0 + Nk + 1
    m = (beta0 * m0[None, :] + Nk[:, None] * xbar) / beta[:, None]
    W = np.zeros((K, dim, dim))
    for k in range(K):
        mult1 = beta0 * Nk[k] / (beta0 + Nk[k])
        diff3 = xbar[k] - m0
        W[k] = np.linalg.inv(W0inv + Nk[k] * S[k] + mult1 * np.outer(diff3, diff3))
    return dict(alpha=alpha, epsilon=epsilon, beta=beta, v=v, m=m, W=W, W0inv=W0inv,
                W0mode=W0mode)


# ----------------------------------------------------------------------------
# lower bound (vbhmm_em_lb.m) and its hyperparameter derivatives
# ----------------------------------------------------------------------------
def vbhmm_em_lb(st: dict, opt: dict, vp: dict, fb: dict, do_deriv: bool = False,
                clipped: Optional[dict] = None):
    """vbhmm_em_lb.m:74-257 (usegroups = 0); with ``do_deriv`` also :260-400, the
    bound's derivatives with respect to the hyperparameters at this posterior
    (returns (LB, dLB), dLB keyed as the reference's d_LB: d_logalpha0,
    d_logepsilon0, d_logv0D1, d_sqrtv0D1, d_logbeta0, d_sqrtbeta0, d_sqrtW0inv,
    d_logW0, d_m0), a derivative set to 0 where its hyperparameter is clipped and
    moving past the limit would raise the bound."""
    dim, K = st["dim"], st["K"]
    alpha0, epsilon0, beta0, v0 = opt["alpha0"], opt["epsilon0"], opt["beta0"], opt["v0"]
    m0, W0inv = opt["mu0"], st["W0inv"]
    v, W, eps, alpha, m, beta = vp["v"], vp["W"], vp["epsilon"], vp["alpha"], vp["m"], vp["beta"]
    lLT, lPi, lA = fb["logLambdaTilde"], fb["logPiTilde"], fb["logATilde"]
    logdetW0inv = (dim * np.log(W0inv[0, 0]) if st["W0mode"] == "iid"
                   else np.log(np.diag(W0inv)).sum())
    q = np.arange(1, dim + 1)
    logCalpha0 = gammaln(K * alpha0) - K * gammaln(alpha0)
    logCepsilon0 = np.full(K, gammaln(K * epsilon0) - K * gammaln(epsilon0))
    logB0 = ((v0 / 2) * logdetW0inv - (v0 * dim / 2) * np.log(2) - (dim * (dim - 1) / 4) * np.log(np.pi)
             - gammaln(0.5 * (v0 + 1 - q)).sum())
    logCalpha = gammaln(alpha.sum()) - gammaln(alpha).sum()
    logCeps = gammaln(eps.sum(1)) - gammaln(eps).sum(1)
    H = 0.0
    trSW = np.zeros(K)
    xWx = np.zeros(K)
    mWm = np.zeros(K)
    trW0W = np.zeros(K)
    for k in range(K):
        logBk = (-(v[k] / 2) * np.log(np.linalg.det(W[k])) - (v[k] * dim / 2) * np.log(2)
                 - (dim * (dim - 1) / 4) * np.log(np.pi) - gammaln(0.5 * (v[k] + 1 - q)).sum())
        H = H - logBk - 0.5 * (v[k] - dim - 1) * lLT[k] + 0.5 * v[k] * dim
        trSW[k] = np.trace(st["t1_S"][k] @ W[k])
        dx = st["xbar"][k] - m[k]
        xWx[k] = dx @ W[k] @ dx
        dm = m[k] - m0
        mWm[k] = dm @ W[k] @ dm
        trW0W[k] = np.trace(W0inv @ W[k])
    Nk = st["Nk"]
    Lt1 = 0.5 * (Nk * (lLT - dim / beta - v * trSW - v * xWx - dim * np.log(2 * np.pi))).sum()
    gamma1 = fb["gamma_all"][:, :, 0]
    Lt2a = (gamma1 * lPi[:, None]).sum()
    Lt2b = (st["M"] * lA).sum()
    Lt2 = Lt2a + Lt2b
    Lt3 = logCalpha0 + (alpha0 - 1) * lPi.sum()
    Lt4 = (logCepsilon0 + (epsilon0 - 1) * lA.sum(1)).sum()
    Lt51 = 0.5 * (dim * np.log(beta0 / (2 * np.pi)) + lLT - dim * beta0 / beta - beta0 * v * mWm).sum()
    Lt52 = K * logB0 + 0.5 * (v0 - dim - 1) * lLT.sum() - 0.5 * (v * trW0W).sum()
    Lt5 = Lt51 + Lt52
    Lt63 = (fb["gamma_all"] * fb["logrho_Saved"]).sum()
    Lt64 = fb["phi_norm"].sum()
    Lt6 = Lt2a + Lt2b + Lt63 - Lt64
    Lt7 = ((alpha - 1) * lPi).sum() + logCalpha + (((eps - 1) * lA).sum(1) + logCeps).sum()
    Lt8 = 0.5 * (lLT + dim * np.log(beta / (2 * np.pi))).sum() - 0.5 * dim * K - H
    LB = float(Lt1 + Lt2 + Lt3 + Lt4 + Lt5 - Lt6 - Lt7 - Lt8)
    if not do_deriv:
        return LB
    return LB, vbhmm_em_lb_derivs(st, opt, vp, fb, clipped)


def vbhmm_em_lb_derivs(st: dict, opt: dict, vp: dict, pre: dict, clipped: Optional[dict] = None) -> dict:
    """vbhmm_em_lb.m:260-400: the bound's derivatives with respect to the (transformed)
    hyperparameters at the posterior ``vp``.  They need the posterior and its prelude
    alone (``pre``: logLambdaTilde, logPiTilde, logATilde), no statistics: ``st`` gives
    dim, K, W0inv and W0mode.  The batched EM calls this on the posterior it kept from
    the last E-step."""
    dim, K = st["dim"], st["K"]
    alpha0, epsilon0, beta0, v0 = opt["alpha0"], opt["epsilon0"], opt["beta0"], opt["v0"]
    m0, W0inv = opt["mu0"], st["W0inv"]
    v, W, m, beta = vp["v"], vp["W"], vp["m"], vp["beta"]
    lLT, lPi, lA = pre["logLambdaTilde"], pre["logPiTilde"], pre["logATilde"]
    logdetW0inv = (dim * np.log(W0inv[0, 0]) if st["W0mode"] == "iid"
                   else np.log(np.diag(W0inv)).sum())
    q = np.arange(1, dim + 1)
    mWm = np.zeros(K)
    for k in range(K):
        dm = m[k] - m0
        mWm[k] = dm @ W[k] @ dm
    # vbhmm_em_lb.m:263-320: the partial derivatives of Lt3 (alpha0), Lt4 (epsilon0)
    # and Lt5 (v0, beta0, W0, m0) -- the only terms holding hyperparameters
    d = {}
    d["alpha0"] = np.atleast_1d(K * digamma(K * alpha0) - K * digamma(alpha0) + lPi.sum())
    d["epsilon0"] = np.atleast_1d(K * (K * digamma(K * epsilon0) - K * digamma(epsilon0)) + lA.sum())
    dlogB0_dv0 = 0.5 * logdetW0inv - (dim / 2) * np.log(2) - 0.5 * digamma(0.5 * (v0 + 1 - q)).sum()
    d["v0"] = np.atleast_1d(K * dlogB0_dv0 + 0.5 * lLT.sum())
    d["beta0"] = np.atleast_1d(0.5 * (dim / beta0 - dim / beta - v * mWm).sum())
    trW = np.array([np.trace(W[k]) for k in range(K)])
    if st["W0mode"] == "iid":
        myW0inv = W0inv[0, 0]
        d_trW0invW = -(myW0inv ** 2) * trW                                  # [K]
        d["W0"] = np.atleast_1d(K * (-0.5 * v0 * dim * myW0inv) - 0.5 * (v * d_trW0invW).sum())
    else:
        myW0inv = np.diag(W0inv).copy()
        d_trW0invW = -(myW0inv[:, None] ** 2) * np.stack([np.diag(W[k]) for k in range(K)], 1)  # [dim][K]
        d["W0"] = K * (-0.5 * v0 * myW0inv) - 0.5 * (v[None, :] * d_trW0invW).sum(1)
    myW0 = 1.0 / myW0inv
    d["m0"] = sum(beta0 * v[k] * (W[k] @ (m[k] - m0)) for k in range(K))
    # :326-341: a clipped hyperparameter's derivative is zeroed where moving further
    # past its limit would raise the bound
    for name, flags in (clipped or {}).items():
        g = d[name]
        for j, fl in enumerate(np.atleast_1d(flags)):
            if (fl == +1 and g[j] > 0) or (fl == -1 and g[j] < 0):
                g[j] = 0.0
    # :387-398: derivatives of the transformed hyperparameters
    dLB = dict(d_logalpha0=d["alpha0"] * alpha0, d_logepsilon0=d["epsilon0"] * epsilon0,
               d_logv0D1=d["v0"] * (v0 - dim + 1), d_sqrtv0D1=d["v0"] * 2 * np.sqrt(v0 - dim + 1),
               d_logbeta0=d["beta0"] * beta0, d_sqrtbeta0=d["beta0"] * 2 * np.sqrt(beta0),
               d_sqrtW0inv=d["W0"] * (myW0 ** 1.5) * (-2), d_logW0=d["W0"] * myW0,
               d_m0=np.asarray(d["m0"], dtype=np.float64))
    return dLB


# ----------------------------------------------------------------------------
# EM
# ----------------------------------------------------------------------------
def vbhmm_em(data: Sequence[np.ndarray], K: int, opt: dict, gmm: Optional[dict] = None,
             rng: Optional[np.random.Generator] = None, device="cuda",
             batch: Optional["vbhmm.SequenceBatch"] = None) -> dict:
    """vbhmm_em.m:1-491 (usegroups = 0): EM from the posterior vbhmm_init builds
    out of ``gmm`` (or a 'random' GMM drawn with ``rng``; or opt['inithmm'] when
    opt['initmode'] == 'inithmm').  Returns the output HMM (prior, trans, pdf, LL,
    gamma, M, N1, N, varpar) plus the bound trajectory ``LLs``, and with
    opt['calc_LLderiv'] the bound's hyperparameter derivatives ``dLL``."""
    data = [np.asarray(a, dtype=np.float64).reshape(-1, len(opt["mu0"])) for a in data]
    opt, clipped = vbhmm_clip_hyps(opt)
    if gmm is None and opt.get("initmode") != "inithmm":
        gmm = random_gmm(data, K, rng if rng is not None else np.random.default_rng(0))
    mix = vbhmm_init(data, K, opt, gmm)
    dim = len(opt["mu0"])
    lens = np.array([a.shape[0] for a in data])
    N, maxT = len(data), int(lens.max())
    X = np.concatenate(data, axis=0)
    n_idx = np.repeat(np.arange(N), lens)
    t_idx = np.concatenate([np.arange(n) for n in lens])
    sb = batch if batch is not None else vbhmm.SequenceBatch(data, dim, device)
    alpha, eps, beta, v, m, W = (mix[k].copy() for k in ("alpha", "epsilon", "beta", "v", "m", "W"))
    alpha0, eps0, beta0, v0, m0 = opt["alpha0"], opt["epsilon0"], opt["beta0"], opt["v0"], opt["mu0"]
    W0inv = mix["W0inv"]
    L = lastL = -np.finfo(float).max
    LLs: List[float] = []
    dLL = None
    C = np.zeros((K, dim, dim))
    unstable = False
    for it in range(1, int(opt["maxIter"]) + 1):
        vp = dict(v=v, W=W, epsilon=eps, alpha=alpha, m=m, beta=beta)
        fb = vbhmm.vbhmm_fb(data, vp, batch=sb)                      # GPU (vbhmm_fb_mex.c)
        g_all = fb["gamma_all"]                                       # [K, N, maxT]
        Nk1 = g_all[:, :, 0].sum(1) + 1e-50
        Nk = g_all.sum(axis=(1, 2)) + 1e-50
        M = fb["xi_sum"].sum(2)
        G = g_all[:, n_idx, t_idx]                                    # gamma_block [K, totalT]
        xbar = (G @ X) / Nk[:, None]
        t1_S = np.zeros((K, dim, dim))
        for k in range(K):
            d1 = X - xbar[k]
            t1_S[k] = (d1 * G[k][:, None]).T @ d1 / Nk[k]
        if it > 1:
            lastL = L
        st = dict(dim=dim, K=K, N=N, W0inv=W0inv, W0mode=mix["W0mode"], t1_S=t1_S, xbar=xbar,
                  Nk=Nk, M=M)
        L = vbhmm_em_lb(st, opt, vp, fb)
        do_break = False
        if it > 1 and abs((L - lastL) / lastL) <= opt["minDiff"]:
            do_break = True
        if it == opt["maxIter"]:
            do_break = True
        if np.isnan(L):  # vbhmm_em.m:314-330
            do_break, unstable, L = True, True, -np.inf
        LLs.append(L)
        if do_break and opt.get("calc_LLderiv", 0):
            # vbhmm_em.m:332-343: the derivatives at the last E-step, before its M-step
            # (NaN when the run went unstable)
            _, dLL = vbhmm_em_lb(st, opt, vp, fb, do_deriv=True, clipped=clipped)
            if unstable:
                dLL = {k: np.full_like(np.asarray(g, dtype=float), np.nan) for k, g in dLL.items()}
        if do_break and unstable:
            break
        # M-step (vbhmm_em.m:352-408)
        alpha = alpha0 + Nk1
        eps = eps0 + M
        if not opt.get("fix_clusters", 0):
            beta = beta0 + Nk
            v = v0 + Nk + 1
            m = (beta0 * m0[None, :] + Nk[:, None] * xbar) / beta[:, None]
            for k in range(K):
                if opt.get("fix_cov") is None:
                    mult1 = beta0 * Nk[k] / (beta0 + Nk[k])
                    diff3 = xbar[k] - m0
                    Wk = np.linalg.inv(W0inv + Nk[k] * t1_S[k] + mult1 * np.outer(diff3, diff3))
                    W[k] = 0.5 * (Wk + Wk.T)
                else:
                    W[k] = np.linalg.inv(opt["fix_cov"]) / (v[k] - dim - 1)
        for k in range(K):
            Ck = np.linalg.inv(W[k]) / ((v[k] - dim - 1) if v[k] > dim + 1 else v[k])
            C[k] = 0.5 * (Ck + Ck.T)
        if do_break:
            break
    prior = alpha / alpha.sum()
    sc = eps.sum(1, keepdims=True)
    trans = eps / np.where(sc == 0, 1.0, sc)
    return dict(prior=prior, trans=trans,
                pdf=[dict(mean=m[k].copy(), cov=C[k].copy()) for k in range(K)],
                LL=float(L), LLs=np.array(LLs), iters=it, unstable=unstable,
                gamma=[g_all[:, n, :lens[n]].copy() for n in range(N)], M=M, N1=Nk1, N=Nk,
                varpar=dict(epsilon=eps, alpha=alpha, beta=beta, v=v, m=m, W=W.copy()),
                clipped=clipped, dLL=dLL)


# ----------------------------------------------------------------------------
# batched EM: every run of a list in one fused call (include/vbhmm_em.h)
# ----------------------------------------------------------------------------
FUSED_MAX_K, FUSED_MAX_DIM = 8, 8
EM_STATUS = ("converged", "max_iter", "unstable", "bad_run")


def em_bucket(Ks, over: int = 8) -> int:
    """The state bucket KM (4 or 8) of the fused kernels for runs or fits of ``Ks`` states;
    ``over`` where a K passes FUSED_MAX_K (16: a KM the library refuses as unsupported)."""
    kmax = int(np.max(Ks))
    return 4 if kmax <= 4 else 8 if kmax <= FUSED_MAX_K else over


def em_post_len(KM: int, dim: int) -> int:
    return KM * (3 + KM + dim + dim * dim)


def em_stats_len(KM: int, dim: int) -> int:
    return KM * (2 + KM + dim + dim * dim)


def pack_posterior(vp: dict, K: int, KM: int, dim: int) -> np.ndarray:
    """A posterior as include/vbhmm_em.h packs it: [alpha KM | epsilon KM x KM | beta KM |
    v KM | m KM x dim | W KM x dim x dim], states and epsilon rows padded to KM (alpha,
    epsilon, beta, v with 1, W with I: values no run reads)."""
    al, be, v = np.ones(KM), np.ones(KM), np.ones(KM)
    eps, m = np.ones((KM, KM)), np.zeros((KM, dim))
    W = np.repeat(np.eye(dim)[None], KM, axis=0)
    al[:K], be[:K], v[:K] = np.reshape(vp["alpha"], -1), np.reshape(vp["beta"], -1), np.reshape(vp["v"], -1)
    eps[:K, :K], m[:K], W[:K] = vp["epsilon"], vp["m"], vp["W"]
    return np.concatenate([al, eps.ravel(), be, v, m.ravel(), W.ravel()])


def unpack_posterior(vec: np.ndarray, K: int, KM: int, dim: int) -> dict:
    o = np.cumsum([0, KM, KM * KM, KM, KM, KM * dim, KM * dim * dim])
    part = [np.asarray(vec[o[i]:o[i + 1]], dtype=np.float64) for i in range(6)]
    return dict(alpha=part[0][:K].copy(), epsilon=part[1].reshape(KM, KM)[:K, :K].copy(),
                beta=part[2][:K].copy(), v=part[3][:K].copy(), m=part[4].reshape(KM, dim)[:K].copy(),
                W=part[5].reshape(KM, dim, dim)[:K].copy())


def unpack_stats(vec: np.ndarray, K: int, KM: int, dim: int) -> dict:
    o = np.cumsum([0, KM, KM, KM * KM, KM * dim, KM * dim * dim])
    part = [np.asarray(vec[o[i]:o[i + 1]], dtype=np.float64) for i in range(5)]
    return dict(Nk1=part[0][:K].copy(), Nk=part[1][:K].copy(), M=part[2].reshape(KM, KM)[:K, :K].copy(),
                xbar=part[3].reshape(KM, dim)[:K].copy(), t1_S=part[4].reshape(KM, dim, dim)[:K].copy())


def em_hyper_vector(opt: dict, W0inv: np.ndarray) -> np.ndarray:
    """[alpha0, epsilon0, beta0, v0, m0[8], diag(W0^-1)[8]] of (clipped) options."""
    dim = len(opt["mu0"])
    h = np.zeros(20)
    h[:4] = opt["alpha0"], opt["epsilon0"], opt["beta0"], opt["v0"]
    h[4:4 + dim] = opt["mu0"]
    h[12:20] = 1.0
    h[12:12 + dim] = np.diag(W0inv)
    return h


def fused_supported(opt: dict, Ks, dim: int) -> bool:
    """The batched EM covers the EM loop without fix_clusters / fix_cov for K <= 8 and
    dim <= 8; everything else stays with the loop engine."""
    return (not opt.get("fix_clusters", 0) and opt.get("fix_cov") is None
            and max(int(k) for k in np.atleast_1d(Ks)) <= FUSED_MAX_K and dim <= FUSED_MAX_DIM)


def _check_engine(engine: str) -> bool:
    if engine not in ("loop", "fused"):
        raise ValueError("engine is 'loop' or 'fused'")
    return engine == "fused"


def _initial_posterior(subjects, s: int, K: int, opt: dict, init: dict) -> dict:
    """vbhmm_init for one run: ``init`` is a GMM (prior, mean, cov) or an HMM whose own
    posterior starts the run ('inithmm')."""
    if "varpar" in init:
        return vbhmm_init([subjects.X[s]], K, dict(opt, initmode="inithmm", inithmm=init), None)
    o = dict(opt)
    if o.get("initmode") == "inithmm":
        o["initmode"] = "random"
    return vbhmm_init([subjects.X[s]], K, o, init)


def _check_init(init: str) -> bool:
    if init not in ("host", "device"):
        raise ValueError("init is 'host' or 'device'")
    return init == "device"


def _w0inv(opt: dict, dim: int):
    """(W0^-1, W0mode) as :func:`vbhmm_init` takes them from the options."""
    W0 = np.asarray(opt["W0"], dtype=np.float64)
    W0m = float(W0) * np.eye(dim) if W0.size == 1 else np.diag(W0.reshape(-1))
    return np.linalg.inv(W0m), ("iid" if W0.size == 1 else "diag")


def _em_runs_desc(subjects, sub: np.ndarray, Ks: np.ndarray, post, KM: int):
    """``post``: the packed posteriors [R][PL], a host array or a tensor already on the
    subjects' device."""
    import torch
    from . import _capi
    dev = subjects.device
    if not isinstance(post, torch.Tensor):
        post = torch.from_numpy(np.ascontiguousarray(post, dtype=np.float64)).to(dev)
    t = dict(sub=torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32)).to(dev),
             K=torch.from_numpy(np.ascontiguousarray(Ks, dtype=np.int32)).to(dev),
             post=post)
    return _capi.EmRunsT(len(sub), KM, _capi.ptr(t["sub"]), _capi.ptr(t["K"]), _capi.ptr(t["post"])), t


# ----------------------------------------------------------------------------
# batched GMM fits: the random trials' starting GMMs in one fused call
# (include/vbhmm_gmm.h)
# ----------------------------------------------------------------------------
GMM_STATUS = ("converged", "max_iter", "ill_conditioned", "bad_fit")


def _hyper_struct(hv: np.ndarray):
    import ctypes
    from . import _capi
    return _capi.EmHyperT(hv[0], hv[1], hv[2], hv[3], (ctypes.c_double * 8)(*hv[4:12]),
                          (ctypes.c_double * 8)(*hv[12:20]))


def gmm_fit_batch(subjects, fits, tolfun: float = 1e-5, max_iter: int = 100, keep_lls: bool = False,
                  hyper: Optional[np.ndarray] = None, chunk_runs: int = 0, KM: Optional[int] = None):
    """:func:`gmm_fit_randsample` for every fit of ``fits`` in one fused call on the GPU
    (vbhmm_gmm_fit_batch, include/vbhmm_gmm.h).  ``subjects`` is a
    :class:`vbhmm.SubjectBatch`; ``fits`` a list of (subject index, K, rows, reg): the K
    start rows index the subject's observations (what ``rng.choice(N, K, replace=False)``
    gave).  One dict per fit: prior [K], mean [K][dim], cov [K][dim][dim] (None unless the
    status is 'converged' or 'max_iter'), ll, iters, status (one of GMM_STATUS;
    'ill_conditioned' is where numpy raises LinAlgError), ``lls`` with keep_lls.  With
    ``hyper`` (:func:`em_hyper_vector` of clipped options) returns (results, post): the
    device tensor [R][PL] of the packed initial posteriors of the fitted GMMs
    (:func:`vbhmm_init`), rows of failed fits unwritten.  2 <= K <= 8 and dim <= 8; ``KM``
    (4 or 8) fixes the padding of ``post``, by default the bucket of the largest K."""
    import ctypes
    import torch
    from . import _capi
    if not len(fits):
        return ([], None) if hyper is not None else []
    lib = _capi.lib()
    dim, dev = subjects.dim, subjects.device
    R = len(fits)
    Ks = np.array([int(f[1]) for f in fits], dtype=np.int32)
    if KM is None:
        KM = em_bucket(Ks, over=16)
    rows = np.zeros((R, KM), dtype=np.int32)
    for i, f in enumerate(fits):
        r = np.asarray(f[2], dtype=np.int64).reshape(-1)
        if r.size != Ks[i]:
            raise ValueError("a fit needs K start rows")
        rows[i, :min(r.size, KM)] = r[:KM]
    f64 = torch.float64
    d_sub = torch.from_numpy(np.array([int(f[0]) for f in fits], dtype=np.int32)).to(dev)
    d_K, d_rows = torch.from_numpy(Ks).to(dev), torch.from_numpy(rows).to(dev)
    d_reg = torch.from_numpy(np.array([float(f[3]) for f in fits], dtype=np.float64)).to(dev)
    ft = _capi.GmmFitsT(R, KM, _capi.ptr(d_sub), _capi.ptr(d_K), _capi.ptr(d_rows), _capi.ptr(d_reg))
    go = _capi.GmmOptT(int(max_iter), float(tolfun), int(chunk_runs))
    o_pr = torch.zeros((R, KM), dtype=f64, device=dev)
    o_me = torch.zeros((R, KM, dim), dtype=f64, device=dev)
    o_co = torch.zeros((R, KM, dim, dim), dtype=f64, device=dev)
    o_ll = torch.zeros(R, dtype=f64, device=dev)
    o_it, o_st = (torch.zeros(R, dtype=torch.int32, device=dev) for _ in range(2))
    o_lls = torch.zeros((R, int(max_iter)), dtype=f64, device=dev) if keep_lls else None
    o_post = torch.zeros((R, em_post_len(KM, dim)), dtype=f64, device=dev) if hyper is not None else None
    hy = _hyper_struct(np.asarray(hyper, dtype=np.float64)) if hyper is not None else None
    sd = subjects.desc()
    nb = int(lib.vbhmm_gmm_fit_workspace_bytes(ctypes.byref(sd), R, KM, int(chunk_runs)))
    ws = _capi.workspace(nb, dev)
    _capi.check(lib.vbhmm_gmm_fit_batch(ctypes.byref(sd), ctypes.byref(ft), ctypes.byref(go), _capi.ptr(o_pr),
                                        _capi.ptr(o_me), _capi.ptr(o_co), _capi.ptr(o_ll), _capi.ptr(o_it),
                                        _capi.ptr(o_st), _capi.ptr(o_lls),
                                        ctypes.byref(hy) if hy is not None else None, _capi.ptr(o_post),
                                        _capi.ptr(ws), ws.numel(), _capi.stream(dev)), "vbhmm_gmm_fit_batch")
    h_pr, h_me, h_co = o_pr.cpu().numpy(), o_me.cpu().numpy(), o_co.cpu().numpy()
    h_ll, h_it, h_st = o_ll.cpu().numpy(), o_it.cpu().numpy(), o_st.cpu().numpy()
    h_lls = o_lls.cpu().numpy() if keep_lls else None
    out = []
    for r in range(R):
        K, done = int(Ks[r]), int(h_st[r]) < 2
        g = dict(prior=h_pr[r, :K].copy() if done else None, mean=h_me[r, :K].copy() if done else None,
                 cov=h_co[r, :K].copy() if done else None, ll=float(h_ll[r]), iters=int(h_it[r]),
                 status=GMM_STATUS[int(h_st[r])])
        if keep_lls:
            # a fit that fails at the factorisation of iteration iters has no ll of that iteration
            g["lls"] = h_lls[r, :g["iters"] - (int(h_st[r]) == 2)].copy()
        out.append(g)
    return (out, o_post) if hyper is not None else out


def random_gmm_batch(subjects, Ks, opt: dict, fit_batch=None, hyper: Optional[np.ndarray] = None,
                     info: Optional[dict] = None, skip=()) -> dict:
    """The GMMs of every (subject, K, trial) as :func:`_draw_inits` / :func:`random_gmm`
    define them, generator stream included, with the fits of all of them in batched calls
    (``fit_batch``: :func:`gmm_fit_batch` or a stand-in with its signature).  Returns
    {(subject, K): [gmm of each trial]}; pairs in ``skip`` are left out.

    K = 1 and N <= K are closed forms on the host and consume no draws.  For the rest each
    (subject, K) has its own default_rng(opt['seed']) and the numtrials row sets are drawn
    up front; one call fits them all.  Where a (subject, K) has an ill-conditioned trial,
    t its first, the host path draws once more and refits trial t with reg = 1e-10, then
    goes on: so the generator is replayed through trial t, the regularised start of t and
    new starts of the trials after t are drawn, and those fits go into the next call, until
    a round brings no new failure (at most numtrials rounds, one call each).  A regularised
    fit that fails again raises numpy.linalg.LinAlgError, as the host path does.

    ``info`` (a dict) receives rounds, regularised {(subject, K): [trials]}, draws
    {(subject, K): count} and, with ``hyper``, post_rounds (each call's device tensor of
    packed initial posteriors) and post_src {(subject, K): [(round, row) of each trial]}."""
    from . import _capi
    fit = fit_batch if fit_batch is not None else gmm_fit_batch
    Ks = [int(k) for k in np.atleast_1d(Ks)]
    KM = em_bucket(Ks)
    numtrials = int(opt["numtrials"])
    out, plan, src = {}, {}, {}
    for s, X in enumerate(subjects.X):
        N = X.shape[0]
        for K in Ks:
            if (s, K) in skip:
                continue
            if K == 1 or N <= K:
                rng = np.random.default_rng(opt["seed"])
                out[(s, K)] = [random_gmm([X], K, rng) for _ in range(1 if K == 1 else numtrials)]
                continue
            rng = np.random.default_rng(opt["seed"])
            plan[(s, K)] = dict(rows=[rng.choice(N, K, replace=False) for _ in range(numtrials)],
                                reg=[0.0] * numtrials, regd=[])
            out[(s, K)] = [None] * numtrials
            src[(s, K)] = [None] * numtrials
    todo = [(key, t) for key in plan for t in range(numtrials)]
    rounds, posts = 0, []
    while todo:
        fits = [(key[0], key[1], plan[key]["rows"][t], plan[key]["reg"][t]) for key, t in todo]
        res = fit(subjects, fits, hyper=hyper, KM=KM)
        if hyper is not None:
            res, post = res
            posts.append(post)
        first_fail = {}
        for i, ((key, t), g) in enumerate(zip(todo, res)):
            if g["status"] == "bad_fit":
                raise _capi.VbhemError("gmm_fit_batch: a fit's subject, K or rows are out of range")
            if g["status"] == "ill_conditioned":
                if plan[key]["reg"][t] > 0:
                    raise np.linalg.LinAlgError("the regularised GMM fit is ill-conditioned too")
                first_fail.setdefault(key, t)    # todo is in trial order: the first failure
            elif key not in first_fail:
                out[key][t] = dict(prior=g["prior"], mean=g["mean"], cov=g["cov"])
                src[key][t] = (rounds, i)
        rounds += 1
        todo = []
        for key, t in first_fail.items():
            p, N = plan[key], subjects.X[key[0]].shape[0]
            p["regd"].append(t)
            rng = np.random.default_rng(opt["seed"])
            for u in range(numtrials):
                r = rng.choice(N, key[1], replace=False)
                if u in p["regd"]:               # the failed draw, then the regularised fit's own
                    r = rng.choice(N, key[1], replace=False)
                if u >= t:
                    p["rows"][u] = r
            p["reg"][t] = 1e-10
            todo += [(key, u) for u in range(t, numtrials)]
    if info is not None:
        info.update(rounds=rounds, regularised={k: list(p["regd"]) for k, p in plan.items() if p["regd"]},
                    draws={k: numtrials + len(p["regd"]) for k, p in plan.items()})
        if hyper is not None:
            info.update(post_rounds=posts, post_src=src)
    return out


def vbhmm_em_gamma(subjects, items, chunk_runs: int = 0) -> list:
    """gamma of the E-step at a posterior, for a list of (subject index, varpar): one
    fused call (vbhmm_em_gamma, include/vbhmm_em.h).  Returns per item the list over the
    subject's sequences of [K][T_n] arrays (the ``gamma`` field of vbhmm_em)."""
    import ctypes
    import torch
    from . import _capi
    if not items:
        return []
    lib = _capi.lib()
    dim, dev = subjects.dim, subjects.device
    Ks = np.array([len(np.reshape(vp["alpha"], -1)) for _, vp in items])
    KM = em_bucket(Ks)
    sub = np.array([s for s, _ in items])
    post = np.stack([pack_posterior(vp, K, KM, dim) for (_, vp), K in zip(items, Ks)])
    rn, keep = _em_runs_desc(subjects, sub, Ks, post, KM)
    rows = np.zeros(len(items) + 1, dtype=np.int64)
    rows[1:] = np.cumsum(subjects.obs[sub])
    d_rows = torch.from_numpy(rows[:-1].copy()).to(dev)
    gam = torch.zeros((max(int(rows[-1]), 1), KM), dtype=torch.float64, device=dev)
    status = torch.zeros(len(items), dtype=torch.int32, device=dev)
    sd = subjects.desc()
    nb = int(lib.vbhmm_em_batch_workspace_bytes(ctypes.byref(sd), len(items), KM, chunk_runs))
    ws = _capi.workspace(nb, dev)
    stream = _capi.stream(dev)
    _capi.check(lib.vbhmm_em_gamma(ctypes.byref(sd), ctypes.byref(rn), _capi.ptr(gam), _capi.ptr(d_rows),
                                   _capi.ptr(status), chunk_runs, _capi.ptr(ws), ws.numel(), stream),
                "vbhmm_em_gamma")
    g = gam.cpu().numpy()
    if int(status.max().item()) != 0:
        raise _capi.VbhemError("vbhmm_em_gamma: a run's subject is out of range")
    del keep
    out = []
    for i, (s, K) in enumerate(zip(sub, Ks)):
        gi = g[rows[i]:rows[i + 1], :K]
        cut = np.concatenate([[0], np.cumsum(subjects.lens[s])])
        out.append([gi[cut[n]:cut[n + 1]].T.copy() for n in range(len(subjects.lens[s]))])
    return out


def em_output_pdf(hmm: dict) -> dict:
    """The output Gaussians of vbhmm_em.m:394-408 from the posterior (W, v), in place."""
    vp = hmm["varpar"]
    K, dim = vp["m"].shape
    pdf = []
    for k in range(K):
        Ck = np.linalg.inv(vp["W"][k]) / ((vp["v"][k] - dim - 1) if vp["v"][k] > dim + 1 else vp["v"][k])
        pdf.append(dict(mean=vp["m"][k].copy(), cov=0.5 * (Ck + Ck.T)))
    hmm["pdf"] = pdf
    return hmm


def fill_gamma(subjects, hmms: Sequence[dict], chunk_runs: int = 0) -> None:
    """The ``gamma`` field of results of :func:`vbhmm_em_batch` (the E-step of the kept
    last-E-step posterior), in one fused call; a result that has it already is left."""
    todo = [h for h in hmms if "gamma" not in h]
    for h, g in zip(todo, vbhmm_em_gamma(subjects, [(h["subject"], h["varpar_estep"]) for h in todo],
                                         chunk_runs)):
        h["gamma"] = g


def vbhmm_em_batch(subjects, runs, opt: dict, device=None, keep_LLs: bool = False, gamma: bool = False,
                   finish: bool = True, chunk_runs: int = 0, timing: Optional[dict] = None,
                   post=None) -> list:
    """The EM of :func:`vbhmm_em` for every run of ``runs`` in one fused call on the GPU
    (vbhmm_em_batch, include/vbhmm_em.h): no host round trip inside the loop.

    ``subjects`` is a :class:`vbhmm.SubjectBatch`; ``runs`` a list of (subject index, K,
    gmm) or (subject index, K, inithmm); the initial posteriors come from
    :func:`vbhmm_init` on the host.  One dict per run with the fields of vbhmm_em's
    result (``LLs`` with keep_LLs, ``gamma`` with gamma=True through one more fused call,
    ``dLL`` with opt['calc_LLderiv'], ``pdf`` unless finish=False: see
    :func:`em_output_pdf`), plus ``subject``, ``status`` and ``varpar_estep``, the
    posterior at the last E-step (``gamma``, ``dLL``, ``N1``, ``N``, ``M`` belong to it).
    K <= 8 and dim <= 8; no fix_clusters / fix_cov.  ``post``: a device tensor [R][PL] of
    packed initial posteriors (:func:`pack_posterior`, padded to the bucket of the largest
    K) used as they are, with runs given as (subject index, K, None): no host
    initialisation.  ``timing`` (a dict) receives the
    seconds of the call's three parts: init (vbhmm_init + packing, host), device (the
    fused call up to the copy back), unpack (host)."""
    import ctypes
    import time
    import torch
    t0 = time.perf_counter()
    from . import _capi
    dim = subjects.dim
    if device is not None and torch.device(device).type != subjects.device.type:
        raise ValueError("the runs execute where the subjects live")
    if opt.get("fix_clusters", 0) or opt.get("fix_cov") is not None:
        raise ValueError("the batched EM has no fix_clusters / fix_cov")
    opt, clipped = vbhmm_clip_hyps(opt)
    if not len(runs):
        return []
    lib = _capi.lib()
    dev = subjects.device
    sub = np.array([int(r[0]) for r in runs])
    Ks = np.array([int(r[1]) for r in runs])
    KM = em_bucket(Ks, over=16)
    PL, SL = em_post_len(KM, dim), em_stats_len(KM, dim)
    if post is None:
        mixes = [_initial_posterior(subjects, s, K, opt, r[2]) for s, K, r in zip(sub, Ks, runs)]
        W0inv, W0mode = mixes[0]["W0inv"], mixes[0]["W0mode"]
        post = np.stack([pack_posterior(mx, K, KM, dim) for mx, K in zip(mixes, Ks)])
    else:
        if (tuple(post.shape) != (len(runs), PL) or post.dtype != torch.float64 or post.device != subjects.device
                or not post.is_contiguous()):
            raise ValueError(f"post is a contiguous float64 tensor [{len(runs)}][{PL}] where the subjects live")
        W0inv, W0mode = _w0inv(opt, dim)
    rn, keep = _em_runs_desc(subjects, sub, Ks, post, KM)
    hv = em_hyper_vector(opt, W0inv)
    hy = _hyper_struct(hv)
    max_iter = int(opt["maxIter"])
    bo = _capi.EmBatchOptT(max_iter, float(opt["minDiff"]), int(chunk_runs))
    R = len(runs)
    f64 = torch.float64
    o_post, o_est = (torch.zeros((R, PL), dtype=f64, device=dev) for _ in range(2))
    o_stats = torch.zeros((R, SL), dtype=f64, device=dev)
    o_LL = torch.zeros(R, dtype=f64, device=dev)
    o_it, o_st = (torch.zeros(R, dtype=torch.int32, device=dev) for _ in range(2))
    o_LLs = torch.zeros((R, max_iter), dtype=f64, device=dev) if keep_LLs else None
    sd = subjects.desc()
    nb = int(lib.vbhmm_em_batch_workspace_bytes(ctypes.byref(sd), R, KM, int(chunk_runs)))
    ws = _capi.workspace(nb, dev)
    stream = _capi.stream(dev)
    t1 = time.perf_counter()
    _capi.check(lib.vbhmm_em_batch(ctypes.byref(sd), ctypes.byref(rn), ctypes.byref(hy), ctypes.byref(bo),
                                   _capi.ptr(o_post), _capi.ptr(o_est), _capi.ptr(o_stats), _capi.ptr(o_LL),
                                   _capi.ptr(o_it), _capi.ptr(o_st), _capi.ptr(o_LLs), _capi.ptr(ws),
                                   ws.numel(), stream), "vbhmm_em_batch")
    h_post, h_est, h_stats = o_post.cpu().numpy(), o_est.cpu().numpy(), o_stats.cpu().numpy()
    h_LL, h_it, h_st = o_LL.cpu().numpy(), o_it.cpu().numpy(), o_st.cpu().numpy()
    h_LLs = o_LLs.cpu().numpy() if keep_LLs else None
    t2 = time.perf_counter()
    del keep
    if (h_st == 3).any():
        raise _capi.VbhemError("vbhmm_em_batch: a run's subject or K is out of range")
    out = []
    for r in range(R):
        K = int(Ks[r])
        vp, vpe, st = (unpack_posterior(h_post[r], K, KM, dim), unpack_posterior(h_est[r], K, KM, dim),
                       unpack_stats(h_stats[r], K, KM, dim))
        sc = vp["epsilon"].sum(1, keepdims=True)
        unstable = int(h_st[r]) == 2
        h = dict(prior=vp["alpha"] / vp["alpha"].sum(), trans=vp["epsilon"] / np.where(sc == 0, 1.0, sc),
                 LL=float(h_LL[r]), iters=int(h_it[r]), unstable=unstable, status=EM_STATUS[int(h_st[r])],
                 M=st["M"], N1=st["Nk1"], N=st["Nk"], varpar=vp, varpar_estep=vpe, clipped=clipped, dLL=None,
                 subject=int(sub[r]))
        if keep_LLs:
            h["LLs"] = h_LLs[r, :h["iters"]].copy()
        if opt.get("calc_LLderiv", 0):
            # vbhmm_em.m:332-343: the derivatives at the last E-step, before its M-step
            stt = dict(dim=dim, K=K, W0inv=W0inv, W0mode=W0mode)
            if unstable:
                with np.errstate(all="ignore"):
                    d = vbhmm_em_lb_derivs(stt, opt, vpe, dict(logLambdaTilde=np.zeros(K), logPiTilde=np.zeros(K),
                                                                logATilde=np.zeros((K, K))), clipped)
                h["dLL"] = {k: np.full_like(np.asarray(g, dtype=float), np.nan) for k, g in d.items()}
            else:
                h["dLL"] = vbhmm_em_lb_derivs(stt, opt, vpe, vbhmm.prelude(vpe), clipped)
        if finish:
            em_output_pdf(h)
        out.append(h)
    if gamma:
        fill_gamma(subjects, out, chunk_runs)
    if timing is not None:
        for k, v in (("init", t1 - t0), ("device", t2 - t1), ("unpack", time.perf_counter() - t2)):
            timing[k] = timing.get(k, 0.0) + v
    return out


# ----------------------------------------------------------------------------
# hyperparameter learning (vbhmm_em_hyp.m, get_hypinfo.m, uniqueLL.m)
# ----------------------------------------------------------------------------
VBHMM_HYPS = ("alpha0", "epsilon0", "v0", "beta0", "W0", "mu0")


def vbhmm_hypinfo(learn_hyps, opt: dict) -> list:
    """get_hypinfo.m:13-79: per learnable hyperparameter its optimiser-space
    transform, inverse, derivative key and size ('W0' = the sqrt(W0inv) transform)."""
    from .hyp import HypInfo
    dim = len(opt["mu0"])
    names = VBHMM_HYPS if (learn_hyps is True or (np.isscalar(learn_hyps) and learn_hyps == 1)) \
        else tuple(learn_hyps)
    out = []
    for h in names:
        if h in ("alpha0", "epsilon0", "beta0"):
            out.append(HypInfo(h, "d_log" + h, np.exp, np.log, 1))
        elif h == "v0":
            out.append(HypInfo("v0", "d_logv0D1", lambda x: np.exp(x) + dim - 1,
                               lambda x: np.log(x - dim + 1), 1))
        elif h in ("W0", "W0isqrt"):
            out.append(HypInfo("W0", "d_sqrtW0inv", lambda x: x ** (-2.0),
                               lambda x: 1.0 / np.sqrt(x), int(np.size(opt["W0"]))))
        elif h == "W0log":
            out.append(HypInfo("W0", "d_logW0", np.exp, np.log, int(np.size(opt["W0"]))))
        elif h == "mu0":
            out.append(HypInfo("mu0", "d_m0", lambda x: x, lambda x: x, dim))
        else:
            raise ValueError("bad value of learn_hyp")
    return out


def _set_hyps(X: np.ndarray, opt: dict, info: list) -> dict:
    """vbhmm_em_hyp.m set_vbopt: optimiser vector -> options."""
    o = dict(opt)
    i = 0
    for h in info:
        with np.errstate(over="ignore"):  # a line-search probe may overflow; clipped later
            val = np.asarray(h.trans(X[i:i + h.dims]), dtype=np.float64)
        o[h.optname] = float(val[0]) if (h.dims == 1 and np.ndim(opt[h.optname]) == 0) else val
        i += h.dims
    o["mu0"] = np.asarray(o["mu0"], dtype=np.float64).reshape(-1)
    return o


def vbhmm_em_hyp(data: Sequence[np.ndarray], K: int, opt: dict, inithmm: dict, device="cuda",
                 batch: Optional["vbhmm.SequenceBatch"] = None, engine: str = "loop",
                 subjects: Optional["vbhmm.SubjectBatch"] = None, subject: int = 0) -> dict:
    """vbhmm_em_hyp.m:15-126: maximise the bound over the transformed
    hyperparameters (minimize_new.m, p.length = opt['hyp_length'], BFGS by default),
    every evaluation an EM run from ``inithmm`` with its derivatives (vbhmm_grad,
    :172-190), then one EM run at the optimum; the result carries ``learn_hyps``
    (hypinfo names, opt_transhyp, opt_L, the optimised hyperparameters).  With
    engine="fused" every evaluation is one :func:`vbhmm_em_batch` call of one run
    (``subjects`` / ``subject``: where ``data`` already lives on the GPU)."""
    from . import hyp
    dim = len(opt["mu0"])
    data = [np.asarray(a, dtype=np.float64).reshape(-1, dim) for a in data]
    fused = _check_engine(engine) and fused_supported(opt, K, dim)
    if fused:
        if subjects is None:
            subjects, subject = vbhmm.SubjectBatch([data], dim, device), 0

        def run_em(o, last=False):
            return vbhmm_em_batch(subjects, [(subject, K, o["inithmm"])], o, keep_LLs=True, gamma=last)[0]
    else:
        sb = batch if batch is not None else vbhmm.SequenceBatch(data, dim, device)

        def run_em(o, last=False):
            return vbhmm_em(data, K, o, batch=sb)
    info = vbhmm_hypinfo(opt.get("learn_hyps", 1) or 1, opt)
    base = dict(opt, initmode="inithmm", inithmm=inithmm)
    n_eval = [0]

    def grad(X):
        o = _set_hyps(X, base, info)
        o["calc_LLderiv"] = 1
        h = run_em(o)
        n_eval[0] += 1
        return -h["LL"], np.concatenate([-np.atleast_1d(h["dLL"][i.derivname]).reshape(-1) for i in info])

    methods = {"minimize-bfgs": "BFGS", "minimize-lbfgs": "LBFGS", "minimize-cg": "CG"}
    name = opt.get("minimizer", "minimize-bfgs")
    if name not in methods:  # 'fminunc' needs MATLAB's Optimization Toolbox
        raise ValueError("bad minimizer specified")
    X0 = hyp.init_x(opt, info)
    Xopt, fX, nls = hyp.minimize(X0, grad, length=int(opt.get("hyp_length", 100)), method=methods[name])
    o2 = _set_hyps(Xopt, base, info)
    o2["calc_LLderiv"] = 0
    h = run_em(o2, last=True)
    h["learn_hyps"] = dict(hypinfo=[i.optname for i in info], opt_transhyp=Xopt, opt_L=-fX[-1],
                           fX=fX, line_searches=nls, evaluations=n_eval[0],
                           vbopt={i.optname: o2[i.optname] for i in info})
    return h


def vbhmm_learn(data: Sequence[np.ndarray], Ks, opt: dict, device="cuda",
                gmms: Optional[dict] = None, engine: str = "loop", init: str = "host") -> dict:
    """vbhmm_learn.m (initmode 'random'): for each K, numtrials EM runs from random
    GMMs (seeded by opt['seed'], vbhmm_learn.m:443-451; K = 1 needs one); with
    opt['learn_hyps'] every unique trial (uniqueLL, 2 minDiff 10 apart) is re-run
    through :func:`vbhmm_em_hyp` (:482-552); keep the best bound; over several K,
    select by LL + gammaln(K+1) (:367-405).  ``gmms[K]`` = list of GMMs to inject
    instead of random draws.  engine="fused": the EM runs of every K and trial in one
    :func:`vbhmm_em_batch` call (the loop engine where that does not apply).
    init="device": under the fused engine the random trials' GMMs are fitted on the GPU
    too (:func:`random_gmm_batch`; "host" wherever the fused engine does not apply)."""
    Ks = [int(k) for k in np.atleast_1d(Ks)]
    dim = len(opt["mu0"])
    data = [np.asarray(a, dtype=np.float64).reshape(-1, dim) for a in data]
    _check_init(init)
    if _check_engine(engine) and fused_supported(opt, Ks, dim):
        return _learn_fused([data], Ks, opt, device, [gmms], init=init)[0]
    sb = vbhmm.SequenceBatch(data, dim, device)
    out_all = []
    for K in Ks:
        inits = _draw_inits(data, K, opt, gmms)
        trials = [vbhmm_em(data, K, opt, gmm=g, batch=sb) for g in inits]
        out_all.append(_learn_pick(data, K, opt, trials, lambda q: vbhmm_em_hyp(data, K, opt, q, batch=sb)))
    return _learn_select(out_all, Ks, opt)


def _device_inits(sbt, Ks: list, opt: dict, gmms_list, runs: list, where: list, timing: Optional[dict]):
    """init="device" of :func:`_learn_fused`: fills ``runs`` with (subject, K, None) and
    ``where`` in the order of the host path and returns the device tensor [R][PL] of their
    packed initial posteriors.  The fitted GMMs' rows come from :func:`random_gmm_batch`
    and never leave the device; the rows of injected GMMs and of the host's closed forms
    (K = 1, N <= K) are packed on the host and copied into their places."""
    import time
    import torch
    t0 = time.perf_counter()
    dim, dev = sbt.dim, sbt.device
    copt, _ = vbhmm_clip_hyps(opt)
    KM = em_bucket(Ks)
    given = {(s, K): list(g[K]) for s, g in enumerate(gmms_list or []) if g is not None for K in Ks if K in g}
    info = {}
    drawn = random_gmm_batch(sbt, Ks, opt, hyper=em_hyper_vector(copt, _w0inv(copt, dim)[0]), info=info,
                             skip=given)
    t1 = time.perf_counter()
    base = np.concatenate([[0], np.cumsum([p.shape[0] for p in info["post_rounds"]])]).astype(np.int64)
    dev_rows, dev_src, host_rows, host_post = [], [], [], []
    for s in range(sbt.S):
        for K in Ks:
            gm = given.get((s, K), drawn.get((s, K)))
            src = info["post_src"].get((s, K)) if (s, K) not in given else None
            for t, g in enumerate(gm):
                if src is not None:
                    dev_rows.append(len(runs))
                    dev_src.append(base[src[t][0]] + src[t][1])
                else:
                    host_rows.append(len(runs))
                    host_post.append(pack_posterior(_initial_posterior(sbt, s, K, copt, g), K, KM, dim))
                runs.append((s, K, None))
                where.append((s, K))
    post = torch.empty((len(runs), em_post_len(KM, dim)), dtype=torch.float64, device=dev)
    if dev_rows:
        allp = torch.cat(info["post_rounds"])
        post[torch.from_numpy(np.array(dev_rows, dtype=np.int64)).to(dev)] = \
            allp[torch.from_numpy(np.array(dev_src, dtype=np.int64)).to(dev)]
    if host_rows:
        post[torch.from_numpy(np.array(host_rows, dtype=np.int64)).to(dev)] = \
            torch.from_numpy(np.stack(host_post)).to(dev)
    if timing is not None:
        timing["gmm"] = timing.get("gmm", 0.0) + (t1 - t0)
        timing["gmm_rounds"] = timing.get("gmm_rounds", 0) + info["rounds"]
        timing["init"] = timing.get("init", 0.0) + (time.perf_counter() - t1)
    return post


def _learn_fused(datas, Ks: list, opt: dict, device, gmms_list, subjects=None, init: str = "host",
                 timing: Optional[dict] = None) -> list:
    """vbhmm_learn for every subject under the fused engine: the GMMs of all subjects, Ks
    and trials are drawn on the host exactly as the loop engine draws them, ONE
    :func:`vbhmm_em_batch` call runs them all (ordered by subject, so neighbouring
    wavefronts read the same data), then each subject's trials go through the same
    selection.  Output Gaussians are computed for every run (they are cheap next to the
    GMM fits); gamma comes from one more fused call for each (subject, K)'s best random
    trial.  init="device": the GMMs are fitted on the GPU (:func:`random_gmm_batch`, the
    same draws) and their packed initial posteriors go straight into the EM call; injected
    ``gmms`` win.  ``timing`` (a dict) receives the seconds of the parts."""
    dim = len(opt["mu0"])
    sbt = subjects if subjects is not None else vbhmm.SubjectBatch(datas, dim, device)
    runs, where = [], []
    if _check_init(init):
        post = _device_inits(sbt, Ks, opt, gmms_list, runs, where, timing)
    else:
        import time
        post, t0 = None, time.perf_counter()
        for s, data in enumerate(sbt.datas):
            g = gmms_list[s] if gmms_list is not None else None
            for K in Ks:
                for gmm in _draw_inits(data, K, opt, g):
                    runs.append((s, K, gmm))
                    where.append((s, K))
        if timing is not None:
            timing["gmm"] = timing.get("gmm", 0.0) + (time.perf_counter() - t0)
    res = vbhmm_em_batch(sbt, runs, opt, keep_LLs=True, timing=timing, post=post)
    per = {}
    for w, h in zip(where, res):
        per.setdefault(w, []).append(h)
    fill_gamma(sbt, [t[int(np.argmax([h["LL"] for h in t]))] for t in per.values()])
    out = []
    for s, data in enumerate(sbt.datas):
        out_all = [_learn_pick(data, K, opt, per[(s, K)],
                               lambda q, K=K: vbhmm_em_hyp(data, K, opt, q, engine="fused", subjects=sbt, subject=s))
                   for K in Ks]
        out.append(_learn_select(out_all, Ks, opt))
    return out


def _draw_inits(data, K: int, opt: dict, gmms: Optional[dict]) -> list:
    """vbhmm_learn.m:443-451: the GMMs of one K's random trials, each K from its own
    generator seeded by opt['seed'] (K = 1 needs one trial), or the injected ones."""
    rng = np.random.default_rng(opt["seed"])
    if gmms is not None and K in gmms:
        return list(gmms[K])
    numits = 1 if K == 1 else int(opt["numtrials"])
    return [random_gmm(data, K, rng) for _ in range(numits)]


def _learn_pick(data, K: int, opt: dict, trials: list, em_hyp) -> dict:
    """vbhmm_learn.m:453-640 for one K: the best of the trials' bounds, after
    hyperparameter learning on the unique ones (``em_hyp(trial)``) where asked for."""
    LLall = np.array([h["LL"] for h in trials])
    LLall_random, trials_random = LLall.copy(), list(trials)
    learn = _do_learn_hyps(opt.get("learn_hyps", 0))
    if learn or opt.get("keep_suboptimal_hmms", 0):
        from .cluster import unique_ll   # uniqueLL.m
        uniq = unique_ll(LLall, 2 * opt["minDiff"] * 10)
    if learn:
        LLall = np.full(len(trials), np.nan)
        for it in uniq:
            trials[it] = em_hyp(trials_random[it])
            LLall[it] = trials[it]["LL"]
    best = trials[int(np.nanargmax(LLall))]
    best["trials_LL"] = LLall
    if opt.get("keep_suboptimal_hmms", 0):  # vbhmm_learn.m:600-602 (the random trials)
        best["suboptimal_hmms"] = [trials_random[it] for it in uniq]
    if learn:
        best["trials_LL_random"] = LLall_random
        if opt.get("keep_best_random_trial", 0):  # vbhmm_learn.m:587-596
            tmp = trials_random[int(np.argmax(LLall_random))]
            if opt.get("sortclusters"):
                tmp = vbhmm_standardize(tmp, opt["sortclusters"])
            best["learn_hyps"]["hmm_best_random_trial"] = tmp
    if opt.get("sortclusters"):  # vbhmm_learn.m:635-640
        best = vbhmm_standardize(best, opt["sortclusters"])
    return best


def _learn_select(out_all: list, Ks: list, opt: dict) -> dict:
    """vbhmm_learn.m:367-424: over several K, select by LL + gammaln(K+1)."""
    if len(Ks) == 1:
        return out_all[0]
    LLk = np.array([h["LL"] for h in out_all]) + gammaln(np.array(Ks) + 1.0)
    ind = int(np.argmax(LLk))
    h = dict(out_all[ind])
    h.update(model_LL=LLk, model_k=Ks, model_bestK=Ks[ind], model_all=out_all, LL=float(LLk[ind]))
    if opt.get("keep_suboptimal_hmms", 0):  # :417-424: every K's unique trials
        h["suboptimal_hmms"] = [q for o in out_all for q in o["suboptimal_hmms"]]
    if opt.get("sortclusters"):  # :635-640 (again; idempotent for the sub-calls' order)
        h = vbhmm_standardize(h, opt["sortclusters"])
    return h


def vbhmm_permute(hmm: dict, cl) -> dict:
    """vbhmm_permute.m (usegroups = 0): the states reordered by ``cl`` (0-based)."""
    cl = np.asarray(cl, dtype=np.int64)
    out = dict(hmm)
    out["prior"] = np.asarray(hmm["prior"])[cl]
    out["trans"] = np.asarray(hmm["trans"])[np.ix_(cl, cl)]
    for k in ("M",):
        if k in hmm:
            out[k] = np.asarray(hmm[k])[np.ix_(cl, cl)]
    for k in ("N1", "N"):
        if k in hmm:
            out[k] = np.asarray(hmm[k])[cl]
    out["pdf"] = [hmm["pdf"][k] for k in cl]
    if "gamma" in hmm:
        out["gamma"] = [np.asarray(g)[cl] for g in hmm["gamma"]]
    for key in ("varpar", "varpar_estep"):
        if key not in hmm:
            continue
        vp = hmm[key]
        out[key] = dict(vp, epsilon=np.asarray(vp["epsilon"])[np.ix_(cl, cl)],
                        alpha=np.asarray(vp["alpha"])[cl], beta=np.asarray(vp["beta"])[cl],
                        v=np.asarray(vp["v"])[cl], m=np.asarray(vp["m"])[cl], W=np.asarray(vp["W"])[cl])
    return out


def vbhmm_prob_steadystate(hmm: dict) -> np.ndarray:
    """vbhmm_prob_steadystate.m computep: the stationary distribution (least squares
    of [A' - I; 1] p = [0; 1]), or the prior for an identity transition matrix."""
    A = np.asarray(hmm["trans"], dtype=float)
    d = A.shape[0]
    if np.all(np.abs(A - np.eye(d)) < 1e-6):
        return np.asarray(hmm["prior"], dtype=float)
    M = np.vstack([A.T - np.eye(d), np.ones((1, d))])
    return np.linalg.lstsq(M, np.r_[np.zeros(d), 1.0], rcond=None)[0]


def vbhmm_standardize(hmm: dict, mode: str) -> dict:
    """vbhmm_standardize.m: reorder the states -- 'e' (or 'd') by size N, 's' by the
    steady-state probability, 'p' by the prior (all descending, stable), 'f' along the
    most likely fixation path (the prior's argmax, then each row's argmax among the
    states not visited yet), 'l' / 'r' by the first mean coordinate ascending /
    descending."""
    if mode in ("d", "e"):
        wi = np.argsort(-np.asarray(hmm["N"], dtype=float), kind="stable")
    elif mode == "s":
        wi = np.argsort(-vbhmm_prob_steadystate(hmm), kind="stable")
    elif mode == "p":
        wi = np.argsort(-np.asarray(hmm["prior"], dtype=float).reshape(-1), kind="stable")
    elif mode == "f":
        A = np.array(hmm["trans"], dtype=float)
        p = np.asarray(hmm["prior"], dtype=float).reshape(-1)
        wi = []
        for t in range(p.size):
            cur = int(np.argmax(p)) if t == 0 else int(np.argmax(A[cur]))
            wi.append(cur)
            A[:, cur] = -1.0
    elif mode in ("l", "r"):
        x = np.array([np.asarray(q["mean"]).reshape(-1)[0] for q in hmm["pdf"]])
        wi = np.argsort(x if mode == "l" else -x, kind="stable")
    else:
        raise ValueError("unknown mode")
    return vbhmm_permute(hmm, wi)


def _do_learn_hyps(v) -> bool:
    """vbhmm_learn.m:357-361: a list of names, or 1."""
    return isinstance(v, (list, tuple)) or (np.isscalar(v) and v == 1)


def vbhmm_learn_batch(datas: Sequence[Sequence[np.ndarray]], Ks, opt: dict, device="cuda",
                      gmms: Optional[list] = None, engine: str = "loop", init: str = "host",
                      timing: Optional[dict] = None):
    """vbhmm_learn_batch.m: one vbhmm_learn per subject; returns (hmms, LLs).  With
    opt['learn_hyps_batch'] (:84-189) one set of hyperparameters shared by every
    subject: each subject's unique random trials (keep_suboptimal_hmms) seed EM runs,
    and BFGS (minimize_new.m, length 100) minimises the mean over subjects of the
    best -(LL + gammaln(K+1)) among that subject's runs (vbhmm_grad_batch_parfor,
    :347-457); the returned HMMs are the final run's, each with its ``vbopt``.

    engine="fused": the EM runs of all subjects, Ks and trials are one
    :func:`vbhmm_em_batch` call, and every evaluation of the shared-hyperparameter
    objective is one call over all (subject, suboptimal HMM) runs; fix_clusters,
    fix_cov, K > 8 and dim > 8 stay with the loop engine.

    init="device": under the fused engine the GMMs of all random trials are fitted in
    batched GPU calls (:func:`random_gmm_batch`, the draws of the host path) and their
    initial posteriors never leave the device; "host" wherever the fused engine does not
    apply.  ``timing`` (a dict) receives the seconds of the fused engine's parts."""
    lhb = opt.get("learn_hyps_batch", 0)
    Ks = [int(k) for k in np.atleast_1d(Ks)]
    fused = _check_engine(engine) and fused_supported(opt, Ks, len(opt["mu0"]))
    _check_init(init)
    if not (isinstance(lhb, (list, tuple)) or lhb):
        if fused:
            hmms = _learn_fused(datas, Ks, opt, device, gmms, init=init, timing=timing)
            return hmms, np.array([h["LL"] for h in hmms])
        hmms = [vbhmm_learn(d, Ks, opt, device, gmms[i] if gmms is not None else None)
                for i, d in enumerate(datas)]
        return hmms, np.array([h["LL"] for h in hmms])
    from . import hyp
    grad_batch, X0, info, opt = hyps_batch_objective(datas, Ks, opt, device, gmms, engine, init)
    methods = {"minimize-bfgs": "BFGS", "minimize-lbfgs": "LBFGS", "minimize-cg": "CG"}
    name = opt.get("minimizer", "minimize-bfgs")
    if name not in methods:
        raise ValueError("bad minimizer specified")
    Xopt, fX, nls = hyp.minimize(X0, grad_batch, length=100, method=methods[name])
    _, _, hmms = grad_batch(Xopt, keep=True)
    for h in hmms:
        h["learn_hyps_batch"] = dict(hypinfo=[i.optname for i in info], opt_transhyp=Xopt,
                                     opt_L=-fX[-1], fX=fX, line_searches=nls)
    if opt.get("sortclusters"):  # vbhmm_learn_batch.m:202-209
        hmms = [vbhmm_standardize(h, opt["sortclusters"]) for h in hmms]
    return hmms, np.array([h["LL"] for h in hmms])


def hyps_batch_objective(datas, Ks, opt: dict, device="cuda", gmms: Optional[list] = None,
                         engine: str = "loop", init: str = "host"):
    """The objective of opt['learn_hyps_batch'] (vbhmm_grad_batch_parfor,
    vbhmm_learn_batch.m:347-457): learns every subject's unique random trials, then
    returns (grad_batch, X0, hypinfo, options) with grad_batch(X, keep=False) -> (mean
    over subjects of the best -(LL + gammaln(K+1)), its gradient[, the best HMMs])."""
    from . import hyp
    lhb = opt["learn_hyps_batch"]
    Ks = [int(k) for k in np.atleast_1d(Ks)]
    fused = _check_engine(engine) and fused_supported(opt, Ks, len(opt["mu0"]))
    _check_init(init)
    if not isinstance(lhb, (list, tuple)):
        if lhb != 1:
            raise ValueError("learn_hyps_batch not set properly")
        lhb = list(VBHMM_HYPS)
    opt = dict(opt, learn_hyps=0)            # :97-101: individual learning is switched off
    info = vbhmm_hypinfo(list(lhb), opt)
    dim = len(opt["mu0"])
    datas = [[np.asarray(a, dtype=np.float64).reshape(-1, dim) for a in d] for d in datas]
    iopt = dict(opt, keep_suboptimal_hmms=1)
    if fused:
        sbt = vbhmm.SubjectBatch(datas, dim, device)
        inithmms = _learn_fused(datas, Ks, iopt, device, gmms, subjects=sbt, init=init)
    else:
        batches = [vbhmm.SequenceBatch(d, dim, device) for d in datas]
        inithmms = [vbhmm_learn(d, Ks, iopt, device, gmms[i] if gmms is not None else None)
                    for i, d in enumerate(datas)]

    def grad_batch_fused(X, keep=False):
        # one call over every (subject, suboptimal HMM) run; then the loop engine's choice
        o = _set_hyps(X, dict(opt, initmode="inithmm", calc_LLderiv=1), info)
        runs = [(n, len(q["pdf"]), q) for n in range(len(datas)) for q in inithmms[n]["suboptimal_hmms"]]
        res = vbhmm_em_batch(sbt, runs, o, keep_LLs=True)
        nL, dnL, out, i = 0.0, 0.0, [], 0
        for n in range(len(datas)):
            best = None
            for q in inithmms[n]["suboptimal_hmms"]:
                qh, K = res[i], len(q["pdf"])
                i += 1
                qnL = -qh["LL"] - gammaln(K + 1)
                if best is None or qnL < best[0]:   # MATLAB min: the first of equal values
                    best = (qnL, qh)
            nL += best[0]
            dnL = dnL - np.concatenate([np.atleast_1d(best[1]["dLL"][i_.derivname]).reshape(-1) for i_ in info])
            if keep:
                best[1]["vbopt"] = {i_.optname: o[i_.optname] for i_ in info}
                out.append(best[1])
        if keep:
            fill_gamma(sbt, out)
        N = len(datas)
        return (nL / N, dnL / N, out) if keep else (nL / N, dnL / N)

    def grad_batch(X, keep=False):
        if fused:
            return grad_batch_fused(X, keep)
        nL, dnL, out = 0.0, 0.0, []
        for n, d in enumerate(datas):
            o = _set_hyps(X, dict(opt, initmode="inithmm", calc_LLderiv=1), info)
            best = None
            for q in inithmms[n]["suboptimal_hmms"]:
                K = len(q["pdf"])
                qh = vbhmm_em(d, K, dict(o, inithmm=q), batch=batches[n])
                qnL = -qh["LL"] - gammaln(K + 1)
                if best is None or qnL < best[0]:   # MATLAB min: the first of equal values
                    best = (qnL, qh)
            nL += best[0]
            dnL = dnL - np.concatenate([np.atleast_1d(best[1]["dLL"][i.derivname]).reshape(-1) for i in info])
            if keep:
                best[1]["vbopt"] = {i.optname: o[i.optname] for i in info}
                out.append(best[1])
        N = len(datas)
        return (nL / N, dnL / N, out) if keep else (nL / N, dnL / N)

    return grad_batch, hyp.init_x(opt, info), info, opt


def vbhmm_remove_empty(hmm: dict, thresh: float = 1.0) -> dict:
    """vbhmm_remove_empty.m:32-103 (usegroups = 0): drop states with N < thresh,
    renormalise gamma, prior and trans from the kept variational parameters."""
    keep = np.flatnonzero(~(np.asarray(hmm["N"]) < thresh))
    if keep.size == len(hmm["N"]):
        return hmm
    vp = hmm["varpar"]
    nvp = dict(alpha=vp["alpha"][keep], epsilon=vp["epsilon"][np.ix_(keep, keep)],
               beta=vp["beta"][keep], v=vp["v"][keep], m=vp["m"][keep], W=vp["W"][keep])
    out = dict(hmm)
    out["varpar"] = nvp
    out["M"] = hmm["M"][np.ix_(keep, keep)]
    out["N1"] = hmm["N1"][keep]
    out["N"] = hmm["N"][keep]
    out["gamma"] = [g[keep] / g[keep].sum(0, keepdims=True) for g in hmm["gamma"]]
    out["prior"] = nvp["alpha"] / nvp["alpha"].sum()
    out["trans"] = nvp["epsilon"] / nvp["epsilon"].sum(1, keepdims=True)
    out["pdf"] = [hmm["pdf"][k] for k in keep]
    return out
