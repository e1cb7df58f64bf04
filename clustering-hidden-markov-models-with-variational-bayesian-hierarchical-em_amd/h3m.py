"""Packed H3M containers, input conversion and synthetic workloads.

* :class:`BaseSet` -- the N base HMMs ``h3m_b`` in the packed, zero-padded
  layout the device E-step consumes (include/vbhem_estep.h).
* :class:`Posterior` -- the K cluster HMMs' variational parameters ``h3m_r``
  (eta, epsilon, lambda, v, m, W per cluster; alpha over clusters).
* :func:`hmms_to_h3m_hem` -- src/vbhem/hmms_to_h3m_hem.m:1-144 (host), and
  :func:`hmms_to_h3m_hem_device` -- the same conversion as a HIP kernel.
* :func:`baseem_init` -- the 'baseem' initialisation of
  src/vbhem/vbhemhmm_init.m:58-100 with the random draws injected.
* :func:`synth_workload` -- the synthetic (N, K, S, d) grids of BASELINE.md.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional

import numpy as np
import torch

COV_DIAG, COV_FULL = 0, 1


@dataclasses.dataclass
class BaseSet:
    """h3m_b, packed: nstates [N], prior [N,SB], A [N,SB,SB] (A[i][from][to]),
    centres [N,SB,d], covars [N,SB,d,d] (full) | [N,SB,d] (diag), omega [N]."""
    nstates: torch.Tensor
    prior: torch.Tensor
    A: torch.Tensor
    centres: torch.Tensor
    covars: torch.Tensor
    omega: torch.Tensor
    covmode: int

    @property
    def N(self) -> int:
        return int(self.prior.shape[0])

    @property
    def SB(self) -> int:
        return int(self.prior.shape[1])

    @property
    def d(self) -> int:
        return int(self.centres.shape[2])

    def to(self, device) -> "BaseSet":
        f = lambda t: t.to(device).contiguous()
        return BaseSet(f(self.nstates), f(self.prior), f(self.A), f(self.centres), f(self.covars),
                       f(self.omega), self.covmode)

    def shard(self, lo: int, hi: int) -> "BaseSet":
        return BaseSet(self.nstates[lo:hi], self.prior[lo:hi], self.A[lo:hi], self.centres[lo:hi],
                       self.covars[lo:hi], self.omega[lo:hi], self.covmode)

    def numpy(self) -> dict:
        return dict(nstates=self.nstates.cpu().numpy().astype(np.int32),
                    prior=self.prior.cpu().numpy(), A=self.A.cpu().numpy(),
                    centres=self.centres.cpu().numpy(), covars=self.covars.cpu().numpy(),
                    omega=self.omega.cpu().numpy(), covmode=self.covmode)

    @staticmethod
    def from_numpy(d: dict) -> "BaseSet":
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
        return BaseSet(torch.as_tensor(np.asarray(d["nstates"], dtype=np.int32)), t(d["prior"]),
                       t(d["A"]), t(d["centres"]), t(d["covars"]), t(d["omega"]), int(d["covmode"]))


@dataclasses.dataclass
class Posterior:
    """h3m_r variational parameters (vbhemhmm_init.m:77-99, vbhem_mstep_component.m:42-69):
    alpha [K]; eta [K,S]; epsilon [K,S,S]; lam [K,S]; v [K,S]; m [K,S,d];
    W [K,S,d,d] (full) | [K,S,d] (diag)."""
    alpha: np.ndarray
    eta: np.ndarray
    epsilon: np.ndarray
    lam: np.ndarray
    v: np.ndarray
    m: np.ndarray
    W: np.ndarray
    W0mode: str = "iid"

    @property
    def K(self) -> int:
        return int(self.m.shape[0])

    @property
    def S(self) -> int:
        return int(self.m.shape[1])

    def copy(self) -> "Posterior":
        return Posterior(*(np.array(getattr(self, f.name)) if f.name != "W0mode" else self.W0mode
                           for f in dataclasses.fields(self)))

    def asdict(self) -> dict:
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}


# ----------------------------------------------------------------------------
# input conversion (hmms_to_h3m_hem.m)
# ----------------------------------------------------------------------------
def hmms_to_h3m_hem(hmms: List[Optional[dict]], covmode: int = COV_FULL,
                    use_post: bool = True) -> BaseSet:
    """Convert a list of VB-HMMs (dicts with prior, trans, pdf[{mean,cov}],
    varpar{alpha,epsilon,beta}) into a packed :class:`BaseSet`.

    use_post=True (the vbhem_h3m_cluster default, :237): prior/A become
    exp(E[log]) -- sub-stochastic, never renormalised (:42-58) -- and each
    covariance is inflated by (beta+1)/beta (:82,88).  Empty entries (None)
    become a one-state dummy with weight 0 (:113-133)."""
    from scipy.special import digamma

    nin = next(len(h["pdf"][0]["mean"]) for h in hmms if h is not None)
    N = len(hmms)
    SB = max(len(h["prior"]) if h is not None else 1 for h in hmms)
    d = nin
    ns = np.ones(N, dtype=np.int32)
    prior = np.zeros((N, SB))
    A = np.zeros((N, SB, SB))
    cen = np.zeros((N, SB, d))
    cov = np.zeros((N, SB, d, d) if covmode == COV_FULL else (N, SB, d))
    omega = np.ones(N)
    for j, h in enumerate(hmms):
        if h is None:
            prior[j, 0] = 1.0
            A[j, 0, 0] = 1.0
            cov[j, 0] = np.eye(d) if covmode == COV_FULL else 1.0
            omega[j] = 0.0
            continue
        S = len(h["prior"])
        ns[j] = S
        if use_post:
            al = np.asarray(h["varpar"]["alpha"], float)
            ep = np.asarray(h["varpar"]["epsilon"], float)
            prior[j, :S] = np.exp(digamma(al) - digamma(al.sum()))
            A[j, :S, :S] = np.exp(digamma(ep) - digamma(ep.sum(1, keepdims=True)))
            infl = (np.asarray(h["varpar"]["beta"], float) + 1) / np.asarray(h["varpar"]["beta"], float)
        else:
            prior[j, :S] = h["prior"]
            A[j, :S, :S] = h["trans"]
            infl = np.ones(S)
        for s in range(S):
            cen[j, s] = h["pdf"][s]["mean"]
            c = np.asarray(h["pdf"][s]["cov"], float)
            cov[j, s] = infl[s] * (np.diag(c) if covmode == COV_DIAG else c)
    omega = omega / omega.sum()
    return BaseSet.from_numpy(dict(nstates=ns, prior=prior, A=A, centres=cen, covars=cov,
                                   omega=omega, covmode=covmode))


def hmms_to_h3m_hem_device(hmms: List[Optional[dict]], covmode: int = COV_FULL,
                           use_post: bool = True, device="cuda") -> BaseSet:
    """:func:`hmms_to_h3m_hem` with the conversion on the device
    (vbhem_hmms_to_h3m, csrc/vbhem_h3m.hip): the HMM list is packed into padded
    arrays of the raw variational counts, point estimates, means and covariances
    here, uploaded once, and the digamma / exp / inflation / weights run as a
    kernel; the BaseSet comes back on ``device``."""
    from . import _capi
    nin = next(len(h["pdf"][0]["mean"]) for h in hmms if h is not None)
    N, d = len(hmms), nin
    SB = max(len(h["prior"]) if h is not None else 1 for h in hmms)
    ns = np.zeros(N, dtype=np.int32)
    al, be = np.ones((N, SB)), np.ones((N, SB))
    ep = np.ones((N, SB, SB))
    pr, tr = np.zeros((N, SB)), np.zeros((N, SB, SB))
    mu, cv = np.zeros((N, SB, d)), np.zeros((N, SB, d, d))
    for j, h in enumerate(hmms):
        if h is None:
            continue
        S = len(h["prior"])
        ns[j] = S
        if use_post:
            al[j, :S] = h["varpar"]["alpha"]
            ep[j, :S, :S] = h["varpar"]["epsilon"]
            be[j, :S] = h["varpar"]["beta"]
        else:
            pr[j, :S] = h["prior"]
            tr[j, :S, :S] = h["trans"]
        for st in range(S):
            mu[j, st] = h["pdf"][st]["mean"]
            cv[j, st] = h["pdf"][st]["cov"]
    dev = torch.device(device)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    ins = dict(ns=torch.as_tensor(ns, device=dev), al=t(al), ep=t(ep), be=t(be), pr=t(pr), tr=t(tr),
               mu=t(mu), cv=t(cv))
    out = dict(prior=torch.empty((N, SB), dtype=torch.float64, device=dev),
               A=torch.empty((N, SB, SB), dtype=torch.float64, device=dev),
               centres=torch.empty((N, SB, d), dtype=torch.float64, device=dev),
               covars=torch.empty((N, SB, d, d) if covmode == COV_FULL else (N, SB, d),
                                  dtype=torch.float64, device=dev),
               omega=torch.empty((N,), dtype=torch.float64, device=dev))
    ws = torch.zeros((1,), dtype=torch.int32, device=dev)
    st = _capi.stream(dev)
    p = _capi.ptr
    _capi.check(_capi.lib().vbhem_hmms_to_h3m(
        N, SB, d, int(covmode), 1 if use_post else 0, p(ins["ns"]), p(ins["al"]), p(ins["ep"]),
        p(ins["be"]), p(ins["pr"]), p(ins["tr"]), p(ins["mu"]), p(ins["cv"]), p(out["prior"]),
        p(out["A"]), p(out["centres"]), p(out["covars"]), p(out["omega"]), p(ws), st),
        "vbhem_hmms_to_h3m")
    nstates = torch.as_tensor(np.maximum(ns, 1), dtype=torch.int32, device=dev)
    return BaseSet(nstates, out["prior"], out["A"], out["centres"], out["covars"], out["omega"],
                   int(covmode))


# ----------------------------------------------------------------------------
# options (vbhem_h3m_cluster.m defaults consumed by the EM loop)
# ----------------------------------------------------------------------------
def default_options(K: int, S: int, d: int, **over) -> dict:
    """vbhem_h3m_cluster.m:150-229 (the subset the EM loop reads)."""
    m0 = {2: [256.0, 192.0], 3: [256.0, 192.0, 150.0]}.get(d, [0.0] * d)
    opt = dict(K=K, S=S, alpha0=1.0, eta0=1.0, epsilon0=1.0, m0=m0, W0=0.005, lambda0=1.0, v0=5.0,
               max_iter=200, minDiff=1e-5, Nv=100, tau=10, covmode=COV_FULL, verbose=0)
    opt["hyps_max"] = dict(alpha0=1.0686e13, eta0=1.0686e13, epsilon0=1.0686e13, v0=1e4,
                           lambda0=1.0686e13, W0=1.0686e13)
    opt["hyps_min"] = dict(alpha0=1.0686e-13, eta0=1.0686e-13, epsilon0=1.0686e-13,
                           v0=2.0612e-09 + d - 1, lambda0=1.0686e-13, W0=1.0686e-13)
    opt.update(over)
    opt["m0"] = np.asarray(opt["m0"], dtype=float).reshape(-1)
    if opt["v0"] <= d - 1:
        raise ValueError("v0 not large enough...should be > D-1")  # vbhem_h3m_cluster.m:233
    return opt


def clip_hyps(opt: dict, with_flags: bool = False):
    """vbhem_clip_hyps.m:20-85: clip each hyperparameter into [hyps_min, hyps_max].
    with_flags: also return the clipped flags (+1 at the max, -1 at the min), which
    vbhemh3m_lb.m:326-343 uses to zero derivatives pointing out of range."""
    out = dict(opt)
    flags = {}
    for name in ("alpha0", "eta0", "epsilon0", "v0", "lambda0", "W0"):
        val = np.array(opt[name], dtype=float, ndmin=1)
        fl = np.zeros(val.size)
        hi, lo = opt["hyps_max"][name], opt["hyps_min"][name]
        fl[val >= hi] = 1.0
        val = np.where(val >= hi, hi, val)
        fl[val <= lo] = -1.0
        val = np.where(val <= lo, lo, val)
        out[name] = val if np.ndim(opt[name]) else float(val[0])
        flags[name] = fl
    return (out, flags) if with_flags else out


def baseem_init(base: BaseSet, opt: dict, randomb: np.ndarray, randomg: np.ndarray,
                omega_rand: np.ndarray, n_total: Optional[int] = None) -> Posterior:
    """'baseem' initialisation (vbhemhmm_init.m:58-100, initopt.mode='u').

    randomb/randomg [K,S]: 0-based base-HMM / state draws (MATLAB randi);
    omega_rand [K]: uniform draws (MATLAB rand).  ``n_total`` = Kb when the
    draws come from a subset of a larger base set."""
    opt = clip_hyps(opt)
    K, S = opt["K"], opt["S"]
    Kb, d = (base.N if n_total is None else int(n_total)), base.d
    Nv = opt["Nv"] * Kb
    NLr = Nv / K
    lam = np.full((K, S), opt["lambda0"] + NLr / S)
    v = np.full((K, S), opt["v0"] + NLr / S + 1)
    rb = np.asarray(randomb, dtype=np.int64)
    rg = np.asarray(randomg, dtype=np.int64)
    ib = torch.as_tensor(rb.reshape(-1), device=base.centres.device)
    ig = torch.as_tensor(rg.reshape(-1), device=base.centres.device)
    cen = base.centres[ib, ig]
    cov = base.covars[ib, ig]
    m = cen.cpu().numpy().reshape(K, S, d)
    cov = cov.cpu().numpy()
    scale = (v.reshape(-1) - d - 1)
    if base.covmode == COV_DIAG:
        W = (1.0 / (scale[:, None] * cov)).reshape(K, S, d)
    else:
        W = np.linalg.inv(scale[:, None, None] * cov).reshape(K, S, d, d)
    eta = np.full((K, S), (1.0 / S) * NLr + opt["eta0"])
    epsilon = np.full((K, S, S), ((1.0 / S) * NLr) / S + opt["epsilon0"])
    omega = np.asarray(omega_rand, dtype=float)
    omega = omega / omega.sum()
    alpha = opt["alpha0"] + omega * Nv
    return Posterior(alpha=alpha, eta=eta, epsilon=epsilon, lam=lam, v=v, m=m, W=W,
                     W0mode="iid" if np.size(opt["W0"]) == 1 else "diag")


def baseem_draws(base: BaseSet, K: int, S: int, seed: int):
    """Seeded stand-in for MATLAB's randi/rand in baseem (numpy PCG64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rb = rng.integers(0, base.N, size=(K, S))
    ns = base.nstates.cpu().numpy()
    rg = np.floor(rng.random((K, S)) * ns[rb]).astype(np.int64)
    om = rng.random(K)
    return rb, rg, om


# ----------------------------------------------------------------------------
# 'wtkmeans' initialisation (vbhemhmm_init.m:294-425, my_weighted_kmeans.m)
# ----------------------------------------------------------------------------
def make_gmm_weights(p: np.ndarray, A: np.ndarray, mode: str) -> np.ndarray:
    """vbhemhmm_init.m makeGMMweights (:1109-1135): a base HMM's state weights."""
    p = np.asarray(p, dtype=float).reshape(-1)
    if "0" in mode:
        for _ in range(50):
            p = p @ A
        return p
    if "3" in mode:
        out = p.copy()
        for _ in range(2):
            p = p @ A
            out = out + p
        return out / 3.0
    if "x" in mode:
        return np.full(p.size, 1.0 / p.size)
    raise ValueError("unknown mode")


def make_a_prior(N: int, mode: str, rng: np.random.Generator):
    """vbhemhmm_init.m makeAprior (:1138-1150): uniform ('u') or random ('r') prior / A."""
    if "u" in mode:
        return np.full(N, 1.0 / N), np.full((N, N), 1.0 / N)
    if "r" in mode:
        prior = rng.random(N)
        prior = prior / prior.sum()
        A = rng.random((N, N))
        return prior, A / A.sum(1, keepdims=True)
    raise ValueError("unknown mode")


def _wk_centroids(point, cluster, weight, K):
    """my_weighted_kmeans.m gcentroids: weighted centres (zero for a weightless cluster)."""
    cen = np.zeros((K, point.shape[1]))
    cw = np.zeros(K)
    for j in range(K):
        mem = cluster == j
        cw[j] = weight[mem].sum()
        cen[j] = (point[mem] * weight[mem, None]).sum(0)
        if cw[j] > 0:
            cen[j] = cen[j] / cw[j]
    return cen, cw


def _wk_energy(point, weight, cen, cw, cluster):
    """my_weighted_kmeans.m genergy: member distances scaled by cw / (cw - w)."""
    f = np.zeros(point.shape[0])
    energy = np.zeros(cen.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):  # MATLAB: x/0 = Inf, 0/0 = NaN
        for j in range(cen.shape[0]):
            mem = cluster == j
            fm = ((point[mem] - cen[j]) ** 2).sum(1)
            energy[j] = (weight[mem] * fm).sum()
            f[mem] = fm * cw[j] / (cw[j] - weight[mem])
    return f, energy


def _nanargmin0(fmat: np.ndarray) -> np.ndarray:
    """MATLAB min(x, [], 1): NaN skipped, the first of equal minima; all-NaN -> 1st."""
    x = np.where(np.isnan(fmat), np.inf, fmat)
    return np.argmin(x, axis=0)


def weighted_kmeans(K: int, it_max: int, point: np.ndarray, weight: np.ndarray,
                    centres: np.ndarray):
    """my_weighted_kmeans.m: points [n][dim] with weights [n] from initial centres
    [K][dim]; returns (0-based cluster [n], centres [K][dim], energies)."""
    point = np.asarray(point, dtype=float)
    weight = np.asarray(weight, dtype=float).reshape(-1)
    cen = np.asarray(centres, dtype=float)
    d2 = ((point[None, :, :] - cen[:, None, :]) ** 2).sum(2)          # [K][n]
    cluster = _nanargmin0(d2)
    cen, cw = _wk_centroids(point, cluster, weight, K)
    f, energy = _wk_energy(point, weight, cen, cw, cluster)
    old = energy.sum()
    energies = [old]
    it = 0
    while it < it_max:
        fmat = np.zeros((K, point.shape[0]))
        with np.errstate(divide="ignore", invalid="ignore"):
            for j in range(K):
                mem = cluster == j
                fmat[j, mem] = f[mem]
                non = ~mem
                adj = cw[j] / (cw[j] + weight[non])
                fmat[j, non] = ((point[non] - cen[j]) ** 2).sum(1) * adj
        cluster = _nanargmin0(fmat)
        cen, cw = _wk_centroids(point, cluster, weight, K)
        f, energy = _wk_energy(point, weight, cen, cw, cluster)
        new = energy.sum()
        if abs(new - old) < 1e-6:
            break
        old = new
        it += 1
        energies.append(new)
    return cluster, cen, np.array(energies)


def kmeans_pp(X: np.ndarray, k: int, rng: np.random.Generator, max_iter: int = 100) -> np.ndarray:
    """Stand-in for MATLAB's kmeans(X, k, 'Replicates', 1) (Statistics Toolbox, absent):
    k-means++ seeding from ``rng``, then batch (Lloyd) updates, an emptied cluster
    re-seeded with the point farthest from its centre ('singleton').  Its draws are not
    MATLAB's twister stream, so the centres are not the reference's: parity unpinned."""
    X = np.asarray(X, dtype=float)
    n = X.shape[0]
    cen = np.empty((k, X.shape[1]))
    cen[0] = X[rng.integers(n)]
    d2 = ((X - cen[0]) ** 2).sum(1)
    for c in range(1, k):
        tot = d2.sum()
        i = rng.choice(n, p=d2 / tot) if tot > 0 else rng.integers(n)
        cen[c] = X[i]
        d2 = np.minimum(d2, ((X - cen[c]) ** 2).sum(1))
    lab = None
    for _ in range(max_iter):
        dist = ((X[None, :, :] - cen[:, None, :]) ** 2).sum(2)
        new = np.argmin(dist, axis=0)
        if lab is not None and np.array_equal(new, lab):
            break
        lab = new
        for c in range(k):
            mem = lab == c
            if mem.any():
                cen[c] = X[mem].mean(0)
            else:
                far = int(np.argmax(dist[lab, np.arange(n)]))
                cen[c] = X[far]
                lab[far] = c
    return cen


def wtkmeans_points(base: BaseSet, mode: str = "r0"):
    """vbhemhmm_init.m:296-323: every base state's mean [n][d] and its normalised
    weight [n] (makeGMMweights of its HMM), plus the first base state's covariance."""
    bn = base.numpy()
    ns = bn["nstates"]
    pts, w = [], []
    for i in range(base.N):
        m = int(ns[i])
        pts.append(bn["centres"][i, :m])
        w.append(make_gmm_weights(bn["prior"][i, :m], bn["A"][i, :m, :m], mode))
    wv = np.concatenate(w)
    return np.concatenate(pts, 0), wv / wv.sum(), bn["covars"][0, 0]


def wtkmeans_init(base: BaseSet, opt: dict, wtseed: int, points=None) -> Posterior:
    """'wtkmeans' initialisation (vbhemhmm_init.m:294-425, initopt.mode 'r0' by default,
    ``points`` = :func:`wtkmeans_points` computed once for all trials;
    vbhem_h3m_cluster.m:213-221): every base state's mean, weighted by its HMM's
    50-step state distribution (makeGMMweights), is clustered into K groups (k-means
    seed, then my_weighted_kmeans); each group's means into S state centres (k-means, or
    the means themselves padded with the first when there are at most S); random prior /
    A per cluster (makeAprior 'r'); counts NJ = (Nv Kb) Kb / K as the reference computes
    them (:386).  MATLAB's kmeans and twister draws are replaced by :func:`kmeans_pp` on
    numpy generators seeded with wtseed and wtseed + 1 (vbhem_h3m_c.m:53 sets wtseed =
    seed + trial): parity of the centres is unpinned, the construction around them
    follows the reference."""
    opt = clip_hyps(opt)
    mode = opt.get("initopt_mode", "r0")
    K, S = opt["K"], opt["S"]
    Kb, d = base.N, base.d
    mumtx, alpha_w, c11 = points if points is not None else wtkmeans_points(base, mode)
    g1 = np.random.Generator(np.random.PCG64(wtseed))
    init_c = kmeans_pp(mumtx, K, g1)
    cluster, _, _ = weighted_kmeans(K, 100, mumtx, alpha_w, init_c)
    centres = [None] * K
    g2 = g1
    for i in range(K):
        mi = mumtx[cluster == i]
        if mi.shape[0] == 0:
            continue
        if mi.shape[0] <= S:
            centres[i] = np.concatenate([mi, np.repeat(mi[:1], S - mi.shape[0], 0)], 0)
        else:
            g2 = np.random.Generator(np.random.PCG64(wtseed + 1))
            centres[i] = kmeans_pp(mi, S, g2)
    return _wtk_posterior(opt, mode, Kb, d, base.covmode, centres, g2, c11)


def _wtk_posterior(opt: dict, mode: str, Kb: int, d: int, covmode: int, centres: list, g2, c11) -> Posterior:
    """The rest of 'wtkmeans' after the state centres (vbhemhmm_init.m:372-425): an empty
    cluster takes the first non-empty cluster's centres, prior / A per cluster from ``g2``
    (makeAprior), the counts and W.  ``opt`` is already clipped."""
    K, S = opt["K"], opt["S"]
    first = next(i for i in range(K) if centres[i] is not None)
    centres = [c if c is not None else centres[first] for c in centres]
    Nv = opt["Nv"] * Kb
    NJ = Nv * Kb / K
    nsj = NJ / S
    eta = np.empty((K, S))
    eps = np.empty((K, S, S))
    for j in range(K):
        prior, A = make_a_prior(S, mode, g2)
        eta[j] = prior * NJ + opt["eta0"]
        eps[j] = A * NJ + opt["epsilon0"]
    v = np.full((K, S), opt["v0"] + nsj + 1)
    lam = np.full((K, S), opt["lambda0"] + nsj)
    if covmode == COV_DIAG:
        W = np.broadcast_to(1.0 / ((opt["v0"] + nsj + 1 - d - 1) * c11), (K, S, d)).copy()
    else:
        W = np.broadcast_to(np.linalg.inv((opt["v0"] + nsj + 1 - d - 1) * c11), (K, S, d, d)).copy()
    alpha = opt["alpha0"] + NJ * np.ones(K)
    return Posterior(alpha=alpha, eta=eta, epsilon=eps, lam=lam, v=v, m=np.stack(centres), W=W,
                     W0mode="iid" if np.size(opt["W0"]) == 1 else "diag")


# ----------------------------------------------------------------------------
# 'wtkmeans' for every trial in batched device calls (include/vbhem_init.h)
# ----------------------------------------------------------------------------
WTK_OK, WTK_DEGENERATE, WTK_BAD = 0, 1, 2
WTK_MAX_DIM, WTK_MAX_K, WTK_MAX_S = 16, 32, 16
# how the k-means of the batched initialisations is laid out on the device: 'block' gives a
# trial to one workgroup; 'tiled' spreads every pass of every trial over a grid of point
# tiles (csrc/vbhem_wtk_tiled.hip)
INIT_SCHEDULES = ("block", "tiled")


def _init_schedule(schedule) -> str:
    if schedule not in INIT_SCHEDULES:
        raise ValueError(f"schedule {schedule!r}: 'block' or 'tiled'")
    return schedule


def wtkmeans_points_batched(base: BaseSet, mode: str = "r0", device=None):
    """:func:`wtkmeans_points` with its loop over the base HMMs as batched tensor
    operations on ``device`` (default: where ``base`` lies): (points [n][d], weights [n])
    as float64 tensors there and the first base state's covariance as numpy.  Only the
    batched initialisation uses it."""
    dev = base.prior.device if device is None else torch.device(device)
    ns = base.nstates.to(dev).long()
    SB = base.SB
    mask = torch.arange(SB, device=dev)[None, :] < ns[:, None]
    p = base.prior.to(dev) * mask
    if "0" in mode or "3" in mode:
        A = base.A.to(dev) * mask[:, :, None] * mask[:, None, :]
        step = lambda q: torch.bmm(q[:, None, :], A)[:, 0, :]
        if "0" in mode:
            for _ in range(50):
                p = step(p)
            wts = p
        else:
            wts = p.clone()
            for _ in range(2):
                p = step(p)
                wts = wts + p
            wts = wts / 3.0
    elif "x" in mode:
        wts = mask / ns[:, None].to(torch.float64)
    else:
        raise ValueError("unknown mode")
    wv = wts[mask]
    pts = base.centres.to(dev)[mask].contiguous()
    return pts, (wv / wv.sum()).contiguous(), base.covars[0, 0].cpu().numpy()


class WtkDeviceEngine:
    """The two batched calls of include/vbhem_init.h on one device.  ``cluster`` keeps the
    trials' labels on the device for ``states``; ``labels_of`` fetches one trial's.
    ``schedule``: 'block' (one workgroup per trial) or 'tiled' (vbhem_wtk_cluster_tiled_batch)
    for ``cluster``; ``states`` is the same under both."""

    def __init__(self, device, chunk_trials=None, schedule="block"):
        self.dev = torch.device(device)
        self.chunk = int(chunk_trials or 0)
        self.schedule = _init_schedule(schedule)

    def cluster(self, pts, w, K, j0, u):
        """pts [n][d], w [n] on the device; j0 [R], u [R][max(K-1, 1)] numpy.  Returns
        (labels handle, counts [R][K], status [R], iters [R][2]) -- numpy but the handle."""
        from . import _capi
        n, d = int(pts.shape[0]), int(pts.shape[1])
        R = len(j0)
        lib, dev = _capi.lib(), self.dev
        self.pts, self.n, self.d, self.K, self.R = pts, n, d, int(K), R
        tj = torch.as_tensor(np.asarray(j0, dtype=np.int32), device=dev)
        tu = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64).reshape(R, max(K - 1, 1)), device=dev)
        labels = torch.full((R, n), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros((R, K), dtype=torch.int32, device=dev)
        status = torch.full((R,), -1, dtype=torch.int32, device=dev)
        iters = torch.zeros((R, 2), dtype=torch.int32, device=dev)
        name = "vbhem_wtk_cluster_tiled" if self.schedule == "tiled" else "vbhem_wtk_cluster"
        wb = getattr(lib, name + "_workspace_bytes")(n, d, K, R, self.chunk)
        ws = _capi.workspace(wb, dev, 16)
        p = _capi.ptr
        _capi.check(getattr(lib, name + "_batch")(n, d, K, R, p(pts), p(w), p(tj), p(tu), self.chunk, p(labels),
                                                  p(counts), p(status), p(iters), p(ws), ws.numel(),
                                                  _capi.stream(dev)), name + "_batch")
        return labels, counts.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()

    def labels_of(self, labels, r):
        return labels[r].cpu().numpy()

    def states(self, labels, S, trial, cluster, nmem, j0, u):
        """The items (trial, cluster, nmem, j0, u [I][max(S-1, 1)]) over the labels of
        ``cluster``.  Returns (centres [R][K][S][d], status [I], iters [I]) as numpy; only
        the rows of OK items are meaningful."""
        from . import _capi
        lib, dev, I = _capi.lib(), self.dev, len(trial)
        centres = torch.zeros((self.R, self.K, S, self.d), dtype=torch.float64, device=dev)
        if I == 0:
            return centres.cpu().numpy(), np.zeros(0, np.int32), np.zeros(0, np.int32)
        nm = np.asarray(nmem, dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(nm)])
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
        tt, tc, tn, tj = (t(a, np.int32) for a in (trial, cluster, nmem, j0))
        to = t(off[:-1], np.int64)
        tu = t(np.asarray(u, dtype=np.float64).reshape(I, max(S - 1, 1)), np.float64)
        status = torch.full((I,), -1, dtype=torch.int32, device=dev)
        iters = torch.zeros((I,), dtype=torch.int32, device=dev)
        wb = lib.vbhem_wtk_states_workspace_bytes(int(off[-1]))
        ws = _capi.workspace(wb, dev, 16)
        p = _capi.ptr
        _capi.check(lib.vbhem_wtk_states_batch(self.n, self.d, self.K, S, self.R, p(self.pts), p(labels), I, p(tt),
                                               p(tc), p(tn), p(to), int(off[-1]), p(tj), p(tu), p(centres),
                                               p(status), p(iters), p(ws), ws.numel(), _capi.stream(dev)),
                    "vbhem_wtk_states_batch")
        return centres.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()


def wtkmeans_init_batch(base: BaseSet, opt: dict, wtseeds, device="cuda", chunk_trials=None,
                        engine=None, info: Optional[dict] = None, schedule="block") -> List[Posterior]:
    """``[wtkmeans_init(base, opt, s, pts) for s in wtseeds]`` with the k-means of every
    trial in two batched device calls (csrc/vbhem_wtk.hip): all trials' K-way clustering,
    then the S-way k-means of every (trial, cluster) with more than S members.  The host
    draws from the same generators in the same order -- PCG64(wtseed) for the first stage,
    a fresh PCG64(wtseed + 1) per cluster with more than S members, makeAprior from
    whichever of them wtkmeans_init would hold -- and reads the member counts between the
    calls, because the second stage's first draw is an index into the members.  Clusters
    with at most S members and empty clusters are filled in here as wtkmeans_init does;
    a trial whose D2 total vanishes (the host's generator takes another branch there) is
    replayed through wtkmeans_init.  ``schedule``: 'block' or 'tiled', the first stage's
    layout on the device (:class:`WtkDeviceEngine`); a given ``engine`` keeps its own.
    ``engine``: a stand-in for :class:`WtkDeviceEngine`;
    ``info``: a dict that receives the seconds of the parts (points, cluster, states: each
    ends in a copy back to the host; host: the rest), the number of second-stage items, the
    replayed trials and the first stage's statuses and iteration counts."""
    import time
    t0 = time.perf_counter()
    copt = clip_hyps(opt)
    mode = copt.get("initopt_mode", "r0")
    K, S = int(copt["K"]), int(copt["S"])
    Kb, d = base.N, base.d
    for name, val, lim in (("d", d, WTK_MAX_DIM), ("K", K, WTK_MAX_K), ("S", S, WTK_MAX_S)):
        if val > lim:
            raise ValueError(f"wtkmeans_init_batch: {name} = {val} exceeds the device limit {name} <= {lim}")
    _init_schedule(schedule)
    eng = engine if engine is not None else WtkDeviceEngine(device, chunk_trials, schedule)
    dev = getattr(eng, "dev", torch.device("cpu"))
    pts, w, c11 = wtkmeans_points_batched(base, mode, dev)
    n = int(pts.shape[0])
    t1 = time.perf_counter()
    seeds = [int(s) for s in wtseeds]
    R = len(seeds)
    if R == 0:
        return []
    g1s = [np.random.Generator(np.random.PCG64(s)) for s in seeds]
    j0 = np.array([g.integers(n) for g in g1s], dtype=np.int64)
    u = np.array([[g.random() for _ in range(K - 1)] + [0.0] * (K == 1) for g in g1s])
    t2 = time.perf_counter()
    labels, counts, status, iters1 = eng.cluster(pts, w, K, j0, u)
    t3 = time.perf_counter()
    if (status == WTK_BAD).any():
        raise ValueError("wtkmeans_init_batch: non-finite base-state means or weights")
    g2s = list(g1s)
    items = []
    for r in range(R):
        if status[r] != WTK_OK:
            continue
        for i in range(K):
            cnt = int(counts[r, i])
            if cnt > S:
                g2s[r] = np.random.Generator(np.random.PCG64(seeds[r] + 1))
                items.append((r, i, cnt, int(g2s[r].integers(cnt)),
                              [g2s[r].random() for _ in range(S - 1)] + [0.0] * (S == 1)))
    t4 = time.perf_counter()
    cen, st2, _ = eng.states(labels, S, *[[it[q] for it in items] for q in range(5)])
    t5 = time.perf_counter()
    if (st2 == WTK_BAD).any():
        raise ValueError("wtkmeans_init_batch: a second-stage item was refused")
    replay = set(np.flatnonzero(status != WTK_OK).tolist())
    replay.update(items[q][0] for q in np.flatnonzero(st2 != WTK_OK))
    host_pts = None
    posts = []
    for r in range(R):
        if r in replay:
            if host_pts is None:
                host_pts = (pts.cpu().numpy(), w.cpu().numpy(), c11)
            posts.append(wtkmeans_init(base, opt, seeds[r], host_pts))
            continue
        centres = [None] * K
        lab = None
        for i in range(K):
            cnt = int(counts[r, i])
            if cnt > S:
                centres[i] = cen[r, i]
            elif cnt > 0:
                if lab is None:
                    lab = eng.labels_of(labels, r)
                    host_pts = host_pts or (pts.cpu().numpy(), w.cpu().numpy(), c11)
                mi = host_pts[0][lab == i]
                centres[i] = np.concatenate([mi, np.repeat(mi[:1], S - mi.shape[0], 0)], 0)
        posts.append(_wtk_posterior(copt, mode, Kb, d, base.covmode, centres, g2s[r], c11))
    if info is not None:
        total = time.perf_counter() - t0
        info.update(points=t1 - t0, cluster=t3 - t2, states=t5 - t4, items=len(items), replayed=sorted(replay),
                    status=np.asarray(status), iters=np.asarray(iters1))
        info["host"] = total - info["points"] - info["cluster"] - info["states"]
    return posts


# ----------------------------------------------------------------------------
# 'gmmNew' initialisation (vbhemhmm_init.m:103-293, GMM_MixHierEM.m, naiveWordMix.m)
# ----------------------------------------------------------------------------
def gmm_mix_hier_em(centres: np.ndarray, covars: np.ndarray, full: bool, T: int,
                    virtual_samples: float, iterations: int, rng: np.random.Generator,
                    init_centres: Optional[np.ndarray] = None):
    """GMM_MixHierEM.m: the mixture of all base Gaussians (naiveWordMix: equal priors)
    reduced to T components by hierarchical EM with ``virtual_samples`` virtual samples;
    returns (priors [T], centres [T][d], covars [T][d][d] | [T][d], log-posteriors
    [T][n]).  The initial centres come from :func:`kmeans_pp` (the reference's arKmeans
    with its anchors start): parity of the result unpinned."""
    X = np.asarray(centres, dtype=float)
    C = np.asarray(covars, dtype=float)
    n, dim = X.shape
    prior = np.full(n, 1.0 / n)
    if T == 1:
        # (:60-73: second moments about the origin, as the reference computes them)
        cov = (prior[:, None, None] * (X[:, :, None] * X[:, None, :] + C)).sum(0) if full \
            else (prior[:, None] * (X ** 2 + C)).sum(0)
        return np.ones(1), (prior @ X)[None, :], cov[None], np.zeros((1, n))
    rng.random((T, n))                                   # (:91 post = rand(T, n): overwritten)
    cent = kmeans_pp(X, T, rng) if init_centres is None else np.array(init_centres, dtype=float)
    vr = np.repeat(C.mean(0)[None], T, 0) if full else np.repeat(C.max(0)[None], T, 0)
    mxwt = np.full(T, 1.0 / T)
    coef = -(dim / 2.0) * np.log(2 * np.pi)
    dpp = prior * virtual_samples
    last = -np.finfo(float).max
    logpost = np.zeros((T, n))
    for _ in range(int(iterations)):
        with np.errstate(divide="ignore", invalid="ignore"):
            if full:
                ivr = np.linalg.inv(vr)
                trc = np.einsum("tab,nab->tn", ivr, C)
                ld = np.log(np.linalg.det(vr))
                diff = cent[:, None, :] - X[None, :, :]
                quad = np.einsum("tna,tab,tnb->tn", diff, ivr, diff)
                xpt = np.log(mxwt)[:, None] + dpp[None, :] * (coef - 0.5 * (trc + quad + ld[:, None]))
            else:
                ivr = 1.0 / vr                                   # [T][d]
                trc = ivr @ C.T
                nrm = (cent * cent * ivr + np.log(vr)).sum(1)
                xpt = np.log(mxwt)[:, None] + dpp[None, :] * (
                    coef - 0.5 * (ivr @ (X * X).T - 2 * (cent * ivr) @ X.T + nrm[:, None] + trc))
            mv = xpt.max(0)
            lx = mv + np.log(np.exp(xpt - mv).sum(0))
            logpost = xpt - lx
            post = np.exp(logpost)
        logp = lx.mean()
        if not np.isfinite(logp) or logp - last < 1e-6:   # (:129-141: stop, keep the last update)
            break
        last = logp
        mxwt = post.mean(1)
        wts = post * prior[None, :]
        wts = wts / wts.sum(1, keepdims=True)
        cent = wts @ X
        for c in range(T):
            dx = X - cent[c]
            if full:
                vr[c] = np.einsum("n,nab->ab", wts[c], dx[:, :, None] * dx[:, None, :] + C)
            else:
                vr[c] = wts[c] @ (dx ** 2 + C)
    return mxwt, cent, vr, logpost


def gmmnew_init(base: BaseSet, opt: dict, seed: int, points=None) -> Posterior:
    """'gmmNew' initialisation (vbhemhmm_init.m:103-293, initopt.mode 'r0' by default):
    the base states' Gaussians reduced to S components (:func:`gmm_mix_hier_em`, Nv Kb
    virtual samples, initopt.iter = 30 iterations) shared by every cluster's states;
    random prior / A per cluster (makeAprior) and random cluster weights omega, counts
    Nsj = omega Nv Kb (:262-291).  ``points`` = (centres, covars) of all base states.
    Draws from one numpy generator seeded with ``seed`` (MATLAB's twister stream in the
    reference): parity unpinned."""
    opt = clip_hyps(opt)
    mode = opt.get("initopt_mode", "r0")
    if "m" in mode:
        raise ValueError("initopt.mode 'm' (priors from the base HMMs) is not supported for gmmNew")
    K, S = opt["K"], opt["S"]
    Kb, d = base.N, base.d
    full = base.covmode == COV_FULL
    if points is None:
        bn = base.numpy()
        ns = bn["nstates"]
        points = (np.concatenate([bn["centres"][i, :int(ns[i])] for i in range(Kb)]),
                  np.concatenate([bn["covars"][i, :int(ns[i])] for i in range(Kb)]))
    rng = np.random.Generator(np.random.PCG64(seed))
    Nv = opt["Nv"] * Kb
    _, cen, cov, _ = gmm_mix_hier_em(points[0], points[1], full, S, Nv,
                                     int(opt.get("initopt_iter", 30)), rng)
    return _gmmnew_posterior(opt, mode, Kb, d, full, cen, cov, rng)


def _gmmnew_posterior(opt: dict, mode: str, Kb: int, d: int, full: bool, cen, cov, rng) -> Posterior:
    """The rest of 'gmmNew' after the reduced mixture (vbhemhmm_init.m:249-291): the draws
    from ``rng`` in the reference's order, the counts and W.  ``opt`` is already clipped."""
    K, S = opt["K"], opt["S"]
    Nv = opt["Nv"] * Kb
    rng.random((K, S))                                   # (:249-250 the emissions' priors)
    pa = [make_a_prior(S, mode, rng) for _ in range(K)]
    omega = rng.random(K)
    omega = omega / omega.sum()
    Nsj = omega * Nv
    eta = np.stack([pa[j][0] * Nsj[j] + opt["eta0"] for j in range(K)])
    eps = np.stack([pa[j][1] * Nsj[j] + opt["epsilon0"] for j in range(K)])
    v = opt["v0"] + Nsj[:, None] / S + 1 + np.zeros((K, S))
    lam = opt["lambda0"] + Nsj[:, None] / S + np.zeros((K, S))
    m = np.repeat(cen[None], K, 0)
    if full:
        W = np.linalg.inv((v - d - 1)[:, :, None, None] * cov[None])
    else:
        W = 1.0 / ((v - d - 1)[:, :, None] * cov[None])
    return Posterior(alpha=opt["alpha0"] + Nsj, eta=eta, epsilon=eps, lam=lam, v=v, m=m, W=W,
                     W0mode="iid" if np.size(opt["W0"]) == 1 else "diag")


# ----------------------------------------------------------------------------
# 'gmmNew' for every trial in one batched device call (include/vbhem_init.h)
# ----------------------------------------------------------------------------
GHEM_OK, GHEM_DEGENERATE, GHEM_BAD, GHEM_NONFINITE, GHEM_SINGULAR = 0, 1, 2, 3, 4
GHEM_MAX_DIM, GHEM_MAX_T = 16, 32


class GhemDeviceEngine:
    """vbhem_ghem_fit_batch of include/vbhem_init.h on one device."""

    def __init__(self, device, chunk_trials=None):
        self.dev = torch.device(device)
        self.chunk = int(chunk_trials or 0)

    def fit(self, X, C, full, T, virtual_samples, iterations, j0, u, init, want_logpost):
        """X [n][d], C [n][d][d] | [n][d] numpy; j0 [R], u [R][max(T-1, 1)] numpy, or init
        [R][T][d].  Returns dict(mxwt, centres, covars, logpost | None, logp, status, iters)
        as numpy; only the rows of OK trials are meaningful."""
        from . import _capi
        lib, dev = _capi.lib(), self.dev
        n, d = X.shape
        R = len(init) if init is not None else len(j0)
        cd = (d, d) if full else (d,)
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
        tx, tc = t(X, np.float64), t(C, np.float64)
        tj = tu = ti = None
        if init is not None:
            ti = t(np.asarray(init, dtype=np.float64).reshape(R, T, d), np.float64)
        else:
            tj, tu = t(j0, np.int32), t(np.asarray(u, dtype=np.float64).reshape(R, max(T - 1, 1)), np.float64)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        mxwt, cen, cov, logp = z(R, T), z(R, T, d), z(R, T, *cd), z(R)
        lpost = z(R, T, n) if want_logpost else None
        status = torch.full((R,), -1, dtype=torch.int32, device=dev)
        iters = torch.zeros((R, 2), dtype=torch.int32, device=dev)
        wb = lib.vbhem_ghem_workspace_bytes(n, d, int(full), T, R, self.chunk)
        ws = _capi.workspace(wb, dev, 16)
        p = _capi.ptr
        _capi.check(lib.vbhem_ghem_fit_batch(n, d, int(full), T, R, p(tx), p(tc), float(virtual_samples),
                                             int(iterations), p(tj), p(tu), p(ti), self.chunk, p(mxwt), p(cen),
                                             p(cov), p(lpost), p(logp), p(status), p(iters), p(ws), ws.numel(),
                                             _capi.stream(dev)), "vbhem_ghem_fit_batch")
        return dict(mxwt=mxwt.cpu().numpy(), centres=cen.cpu().numpy(), covars=cov.cpu().numpy(),
                    logpost=None if lpost is None else lpost.cpu().numpy(), logp=logp.cpu().numpy(),
                    status=status.cpu().numpy(), iters=iters.cpu().numpy())

    def seed(self, X, T, j0, u):
        """kmeans_pp alone by the tiled schedule (vbhem_wtk_seed_tiled_batch): X [n][d], j0
        [R], u [R][T-1] numpy.  Returns (centres [R][T][d], status [R], Lloyd passes [R]) as
        numpy; only the rows of OK trials are meaningful."""
        from . import _capi
        lib, dev = _capi.lib(), self.dev
        n, d = X.shape
        R = len(j0)
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
        tx, tj = t(X, np.float64), t(j0, np.int32)
        tu = t(np.asarray(u, dtype=np.float64).reshape(R, max(T - 1, 1)), np.float64)
        cen = torch.zeros((R, T, d), dtype=torch.float64, device=dev)
        status = torch.full((R,), -1, dtype=torch.int32, device=dev)
        iters = torch.zeros((R,), dtype=torch.int32, device=dev)
        wb = lib.vbhem_wtk_seed_tiled_workspace_bytes(n, d, T, R, self.chunk)
        ws = _capi.workspace(wb, dev, 16)
        p = _capi.ptr
        _capi.check(lib.vbhem_wtk_seed_tiled_batch(n, d, T, R, p(tx), p(tj), p(tu), self.chunk, p(cen), p(status),
                                                   p(iters), p(ws), ws.numel(), _capi.stream(dev)),
                    "vbhem_wtk_seed_tiled_batch")
        return cen.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()


def gmm_mix_hier_em_batch(centres: np.ndarray, covars: np.ndarray, full: bool, T: int, virtual_samples: float,
                          iterations: int, seeds, device="cuda", chunk_trials=None, engine=None,
                          init_centres=None, want_logpost: bool = False, info: Optional[dict] = None,
                          schedule="block"):
    """``[gmm_mix_hier_em(centres, covars, full, T, virtual_samples, iterations,
    Generator(PCG64(s))) for s in seeds]`` with the hierarchical EM of every trial in one
    batched device call (csrc/vbhem_ghem.hip); the fourth entry of a trial's tuple is None
    unless ``want_logpost``.  The host keeps the generators: per trial it skips the
    discarded rand(T, n) (``bit_generator.advance(T * n)``: one 64-bit step per double),
    draws kmeans_pp's first index and its T - 1 uniform draws, and leaves the generator
    where gmm_mix_hier_em would (``info['rngs']``).  ``init_centres`` [R][T][d]: the start
    centres of every trial, no seeding.  T = 1 is the closed form on the host.  A trial
    whose status is not OK (a vanished D2 total, a logp that is not finite, a failed pivot,
    non-finite points) is replayed through gmm_mix_hier_em with a fresh generator of its
    seed and behaves as it does there.  ``schedule`` = 'tiled' (without ``init_centres``):
    the same draws go to the tiled k-means++ seeding (``engine.seed``,
    vbhem_wtk_seed_tiled_batch) and its centres start the EM call; a trial whose seeding is
    not OK is replayed like the others (its slot of the EM call gets zero centres and is
    ignored), and the seeding's Lloyd passes are reported where the EM call's were
    (``info['seed']``: its seconds).  ``engine``: a stand-in for
    :class:`GhemDeviceEngine`; ``info`` also receives the seconds of the parts (fit: the
    device call and its copies; host: the rest), the statuses, the iteration counts and
    the replayed trials."""
    import time
    t0 = time.perf_counter()
    X = np.ascontiguousarray(centres, dtype=float)
    C = np.ascontiguousarray(covars, dtype=float)
    n, d = X.shape
    T = int(T)
    for name, val, lim in (("d", d, GHEM_MAX_DIM), ("T", T, GHEM_MAX_T)):
        if val > lim:
            raise ValueError(f"gmm_mix_hier_em_batch: {name} = {val} exceeds the device limit {name} <= {lim}")
    seeds = [int(s) for s in seeds]
    R = len(seeds)
    rngs = [np.random.Generator(np.random.PCG64(s)) for s in seeds]
    inits = None if init_centres is None else np.asarray(init_centres, dtype=float).reshape(R, T, d)
    fresh = lambda r: gmm_mix_hier_em(X, C, full, T, virtual_samples, iterations, rngs[r],
                                      None if inits is None else inits[r])
    if T == 1 or R == 0:
        out = [fresh(r) for r in range(R)]
        if info is not None:
            info.update(rngs=rngs, replayed=[], fit=0.0, host=time.perf_counter() - t0)
        return out
    j0 = np.zeros(R, dtype=np.int64)
    u = np.zeros((R, T - 1))
    for r, g in enumerate(rngs):
        g.bit_generator.advance(T * n)                   # (:91 post = rand(T, n): overwritten)
        if inits is None:
            j0[r] = g.integers(n)
            u[r] = [g.random() for _ in range(T - 1)]
    eng = engine if engine is not None else GhemDeviceEngine(device, chunk_trials)
    t1 = time.perf_counter()
    seeded = None
    if _init_schedule(schedule) == "tiled" and inits is None:
        scen, sst, sit = eng.seed(X, T, j0, u)
        seeded = (np.asarray(sst), np.asarray(sit))
        start = np.where((seeded[0] == WTK_OK)[:, None, None], scen, 0.0)
        ts = time.perf_counter()
        got = eng.fit(X, C, bool(full), T, float(virtual_samples), int(iterations), None, None, start,
                      bool(want_logpost))
        got = dict(got, status=np.where(seeded[0] == WTK_OK, got["status"], seeded[0]).astype(np.int32),
                   iters=np.stack([seeded[1], got["iters"][:, 1]], 1).astype(np.int32))
    else:
        ts = t1
        got = eng.fit(X, C, bool(full), T, float(virtual_samples), int(iterations), j0, u, inits,
                      bool(want_logpost))
    t2 = time.perf_counter()
    out, replay = [], []
    for r in range(R):
        if got["status"][r] != GHEM_OK:
            replay.append(r)
            rngs[r] = np.random.Generator(np.random.PCG64(seeds[r]))
            out.append(fresh(r))
            continue
        out.append((got["mxwt"][r], got["centres"][r], got["covars"][r],
                    got["logpost"][r] if want_logpost else None))
    if info is not None:
        info.update(rngs=rngs, replayed=replay, status=got["status"], iters=got["iters"], logp=got["logp"],
                    fit=t2 - t1, seed=ts - t1)
        info["host"] = time.perf_counter() - t0 - info["fit"]
    return out


def gmmnew_init_batch(base: BaseSet, opt: dict, seeds, device="cuda", chunk_trials=None, engine=None,
                      info: Optional[dict] = None, schedule="block") -> List[Posterior]:
    """``[gmmnew_init(base, opt, s) for s in seeds]`` with the hierarchical EM of every
    trial in one batched device call (:func:`gmm_mix_hier_em_batch`); the draws after the
    EM come from the trial's generator as gmmnew_init takes them.  ``info`` receives the
    seconds of the parts (points, fit, host: the rest; seed: the part of fit the tiled
    seeding took), the replayed trials and the E-steps every device trial evaluated.
    ``schedule``: 'block' or 'tiled', the layout of the k-means++ seeding on the device
    (:func:`gmm_mix_hier_em_batch`)."""
    import time
    t0 = time.perf_counter()
    copt = clip_hyps(opt)
    mode = copt.get("initopt_mode", "r0")
    if "m" in mode:
        raise ValueError("initopt.mode 'm' (priors from the base HMMs) is not supported for gmmNew")
    S = int(copt["S"])
    Kb, d = base.N, base.d
    full = base.covmode == COV_FULL
    for name, val, lim in (("d", d, GHEM_MAX_DIM), ("S", S, GHEM_MAX_T)):
        if val > lim:
            raise ValueError(f"gmmnew_init_batch: {name} = {val} exceeds the device limit {name} <= {lim}")
    bn = base.numpy()
    ns = bn["nstates"]
    X = np.concatenate([bn["centres"][i, :int(ns[i])] for i in range(Kb)])
    C = np.concatenate([bn["covars"][i, :int(ns[i])] for i in range(Kb)])
    t1 = time.perf_counter()
    sub = {}
    fits = gmm_mix_hier_em_batch(X, C, full, S, copt["Nv"] * Kb, int(copt.get("initopt_iter", 30)), seeds, device,
                                 chunk_trials, engine, info=sub, schedule=schedule)
    posts = [_gmmnew_posterior(copt, mode, Kb, d, full, cen, cov, g) for (_, cen, cov, _), g in zip(fits, sub["rngs"])]
    if info is not None:
        total = time.perf_counter() - t0
        info.update(points=t1 - t0, fit=sub["fit"], seed=sub.get("seed", 0.0), replayed=sub["replayed"],
                    esteps=[int(v) for v in sub["iters"][:, 1]] if "iters" in sub else [],
                    lloyd=[int(v) for v in sub["iters"][:, 0]] if "iters" in sub else [])
        info["host"] = total - info["points"] - info["fit"]
    return posts


# ----------------------------------------------------------------------------
# synthetic workloads
# ----------------------------------------------------------------------------
CONFIGS = {
    # name: (N, K, S, Sb, d, covmode, tau, Nv, option overrides)
    "C2": dict(N=100, K=4, S=3, Sb=2, d=2, covmode=COV_FULL, tau=50, Nv=100,
               opt=dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0,
                        m0=[1.5, 1.5])),
    "C3": dict(N=10_000, K=8, S=5, Sb=5, d=2, covmode=COV_DIAG, tau=10, Nv=100, opt={}),
    # v0 must exceed d-1 (vbhem_h3m_cluster.m:233); the default 5 only suits d <= 5
    "C4": dict(N=100_000, K=16, S=8, Sb=8, d=8, covmode=COV_FULL, tau=10, Nv=100, opt=dict(v0=10.0)),
    "C5": dict(N=1_000_000, K=32, S=12, Sb=12, d=16, covmode=COV_FULL, tau=10, Nv=100,
               opt=dict(v0=18.0)),
}


def _digamma(x: torch.Tensor) -> torch.Tensor:
    return torch.special.digamma(x)


def synth_base_set(N: int, K: int, Sb: int, d: int, covmode: int, seed: int,
                   device="cpu", exprmt1: bool = False, ragged: bool = False,
                   n_total: Optional[int] = None, i_offset: int = 0,
                   face: bool = False) -> BaseSet:
    """Synthetic h3m_b built directly in packed form (use_post=1 semantics).

    Ground truth: K HMMs, base i is a noisy copy of GT g = i mod K: means
    U[0,5]^d + N(0,0.1^2) per base, covariance L L'/d + 0.5 I (full) or
    U[0.5,1.5] (diag), prior and A rows ~ Dirichlet(1); VB counts
    alpha = 1+25*pi, epsilon = 1+250*A, beta = 1+250/Sb, then the
    hmms_to_h3m_hem(use_post=1) transform.  exprmt1=True uses the two GT HMMs
    of Synthetic_experiment/exprmt1_sampledata.m:20-43 instead (Sb=d=2).
    face=True draws eye-fixation-scale emissions (demo/vbdemo_face.m: screen
    pixels): GT means [256, 192, 150, ...][:d] + U[-60, 60]^d, per-base mean
    noise N(0, 5^2), covariances 900 (L L'/d + 0.5 I) (about 30 px spread).
    ragged=True draws per-base state counts in [1, Sb] (zero-padded).
    Generated on ``device``; ``n_total``/``i_offset`` place this block of N
    bases inside a larger set (omega = 1/n_total, GT index (i_offset+i) mod K)."""
    device = torch.device(device)
    gcpu = torch.Generator(device="cpu").manual_seed(int(seed))
    g = torch.Generator(device=device).manual_seed(int(seed) + 1)
    dt = torch.float64
    n_total = N if n_total is None else int(n_total)
    if exprmt1:
        G = 2
        gt_prior = torch.tensor([[0.5, 0.5], [0.5, 0.5]], dtype=dt)
        gt_A = torch.tensor([[[0.6, 0.4], [0.4, 0.6]], [[0.4, 0.6], [0.6, 0.4]]], dtype=dt)
        gt_mu = torch.tensor([[[0.0, 0.0], [3.0, 3.0]]] * 2, dtype=dt)
        eye = torch.eye(2, dtype=dt)
        gt_cov = eye.expand(G, 2, 2, 2).clone() if covmode == COV_FULL else torch.ones(G, 2, 2, dtype=dt)
    else:
        G = K
        gt_prior = _dirichlet(gcpu, (G,), Sb)
        gt_A = _dirichlet(gcpu, (G, Sb), Sb)
        gt_mu = torch.rand((G, Sb, d), generator=gcpu, dtype=dt) * 5.0
        if covmode == COV_FULL:
            Lm = torch.randn((G, Sb, d, d), generator=gcpu, dtype=dt)
            gt_cov = Lm @ Lm.transpose(-1, -2) / d + 0.5 * torch.eye(d, dtype=dt)
        else:
            gt_cov = 0.5 + torch.rand((G, Sb, d), generator=gcpu, dtype=dt)
        if face:
            centre = torch.tensor(([256.0, 192.0, 150.0] + [128.0] * d)[:d], dtype=dt)
            gt_mu = centre + (gt_mu / 5.0 - 0.5) * 120.0
            gt_cov = 900.0 * gt_cov
    gt_prior, gt_A, gt_mu, gt_cov = (x.to(device) for x in (gt_prior, gt_A, gt_mu, gt_cov))
    gi = (torch.arange(N, device=device) + int(i_offset)) % G
    alpha = 1.0 + 25.0 * gt_prior[gi]
    eps = 1.0 + 250.0 * gt_A[gi]
    beta = 1.0 + 250.0 / Sb
    prior = torch.exp(_digamma(alpha) - _digamma(alpha.sum(-1, keepdim=True)))
    A = torch.exp(_digamma(eps) - _digamma(eps.sum(-1, keepdim=True)))
    noise = 5.0 if face else 0.1
    centres = gt_mu[gi] + noise * torch.randn((N, Sb, d), generator=g, dtype=dt, device=device)
    covars = ((beta + 1.0) / beta) * gt_cov[gi]
    nstates = torch.full((N,), Sb, dtype=torch.int32, device=device)
    if ragged and Sb > 1:
        nstates = torch.randint(1, Sb + 1, (N,), generator=g, dtype=torch.int32, device=device)
        mask = torch.arange(Sb, device=device)[None, :] < nstates[:, None].long()
        prior = prior * mask
        A = A * mask[:, :, None] * mask[:, None, :]
        centres = centres * mask[:, :, None]
        if covmode == COV_FULL:
            covars = torch.where(mask[:, :, None, None], covars,
                                 torch.eye(d, dtype=dt, device=device).expand_as(covars))
        else:
            covars = torch.where(mask[:, :, None], covars, torch.ones_like(covars))
    omega = torch.full((N,), 1.0 / n_total, dtype=dt, device=device)
    return BaseSet(nstates, prior.contiguous(), A.contiguous(), centres.contiguous(),
                   covars.contiguous(), omega, covmode)


def _dirichlet(g: torch.Generator, batch, n: int) -> torch.Tensor:
    # Dirichlet(1) = normalised Exp(1) draws
    e = -torch.log(torch.rand(tuple(batch) + (n,), generator=g, dtype=torch.float64).clamp_min(1e-300))
    return e / e.sum(-1, keepdim=True)


def synth_workload(name: str, seed: Optional[int] = None, device="cpu", N: Optional[int] = None,
                   shard: Optional[tuple] = None, ragged: bool = False):
    """(BaseSet, Posterior, options) for a named config; seed = 1001 + index
    (BASELINE.md).  ``N`` overrides the number of base HMMs (sub-sampling).
    ``shard=(lo, hi)`` generates only bases [lo, hi) of the N (seeded per
    shard); the Posterior is identical for every shard (baseem over the first
    min(N, 4096) bases of shard 0's seed)."""
    cfg = CONFIGS[name]
    idx = list(CONFIGS).index(name) + 1
    seed = 1001 + idx if seed is None else seed
    n = cfg["N"] if N is None else N
    lo, hi = (0, n) if shard is None else shard
    args = (cfg["K"], cfg["Sb"], cfg["d"], cfg["covmode"])
    ex = name == "C2"
    base = synth_base_set(hi - lo, *args, seed + 7919 * lo, device=device, exprmt1=ex,
                          ragged=ragged, n_total=n, i_offset=lo)
    opt = default_options(cfg["K"], cfg["S"], cfg["d"], tau=cfg["tau"], Nv=cfg["Nv"],
                          covmode=cfg["covmode"], **cfg["opt"])
    if shard is None and n <= 4096:
        init = base
    else:
        # every shard (and the unsharded large case) draws the initial clusters from the
        # same standalone first-4096-bases set, so all ranks hold identical posteriors
        init = synth_base_set(min(n, 4096), *args, seed, device=device, exprmt1=ex, ragged=ragged,
                              n_total=n)
    rb, rg, om = baseem_draws(init, cfg["K"], cfg["S"], seed)
    post = baseem_init(init, opt, rb, rg, om, n_total=n)
    return base, post, opt
