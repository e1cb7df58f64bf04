"""Model selection over a K x S grid: DIC of VBHEM fits, BIC / AIC of VHEM fits, and
the clean-up the reference applies to a result before reading K and S off it.

* :func:`loglik_grid` -- the likelihood term of myDIC.m:160-170 for every model of a
  grid in ONE launch of ``vbhmm_dic_loglik`` (csrc/vbhmm_dic.hip: backward sweep and
  termination only, clusters of different sizes side by side, the mixture log-sum-exp
  and the sum over subjects taken in the kernel), or -- ``engine="pairs"`` -- by looping
  the models through ``EStepEngine.pairs(smooth=1)`` with the log-sum-exp in torch.
* :func:`my_dic` -- src/compare_mtds/dic/myDIC.m (issyn = 0); :func:`dic_grid` --
  Synthetic_experiment/evaluate_vbhem_jounarl.m:125-156 over ``vbhem_h3m_cluster``'s
  ``model_all`` / ``model_all_s``.
* :func:`vhem_bic` / :func:`vhem_aic` -- evaluate_vbhem_jounarl.m:159-235.
* :func:`fit_to_h3m` / :func:`vbh3m_remove_empty` -- src/vbhem/vbh3m_remove_empty.m.

A group-HMM mixture (one model of a grid) is a dict: prior [K,S], A [K,S,S], centres
[K,S,d], covars [K,S,d] (or [K,S,d,d]: the diagonals are taken, as hmms_to_h3m(.,'diag')
does), optional nstates [K] (own states; the rest is padding), omega [K] or logw [K] (the
mixture weights; default uniform) and scale (the N~ that multiplies L; default 1).
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch
from scipy.special import digamma

from . import _capi, host
from .h3m import COV_DIAG, BaseSet

VBHEM_ERR_UNSUPPORTED = -2   # include/vbhem_estep.h


# ----------------------------------------------------------------------------
# the likelihood of a grid of models
# ----------------------------------------------------------------------------
def _as_base(hmms) -> BaseSet:
    if isinstance(hmms, BaseSet):
        if hmms.covmode != COV_DIAG:
            raise ValueError("DIC needs a diag BaseSet (hmms_to_h3m(hmms, 'diag'))")
        return hmms
    from .vhem import hmms_to_h3m
    return hmms_to_h3m(list(hmms), "diag")


def _diag_covars(cov: np.ndarray) -> np.ndarray:
    cov = np.asarray(cov, dtype=np.float64)
    return np.diagonal(cov, axis1=-2, axis2=-1).copy() if cov.ndim == 4 else cov


def pack_models(models: Sequence[dict]) -> dict:
    """The models descriptor of include/vbhmm_dic.h as host arrays: clusters model after
    model, padded to the largest S, each cluster's constants
    (host.vhem_cluster_constants, diag) computed on its own states; padding holds
    logA = logPi = -inf, m = c = 0, P = 1 and is never read."""
    G = len(models)
    Ks = [int(np.asarray(mo["prior"]).shape[0]) for mo in models]
    S = max(int(np.asarray(mo["prior"]).shape[1]) for mo in models)
    d = int(np.asarray(models[0]["centres"]).shape[-1])
    C = int(sum(Ks))
    out = dict(G=G, C=C, S=S, d=d, max_model_clusters=max(Ks),
               model_off=np.concatenate([[0], np.cumsum(Ks)]).astype(np.int32),
               nstates_r=np.zeros(C, np.int32), logw=np.zeros(C), scale=np.zeros(G),
               logA=np.full((C, S, S), -np.inf), logPi=np.full((C, S), -np.inf),
               m=np.zeros((C, S, d)), P=np.ones((C, S, d)), c=np.zeros((C, S)))
    c0 = 0
    for g, mo in enumerate(models):
        K = Ks[g]
        prior = np.asarray(mo["prior"], dtype=np.float64)
        cov = _diag_covars(mo["covars"])
        ns = np.asarray(mo.get("nstates", np.full(K, prior.shape[1])), dtype=np.int32)
        if "logw" in mo:
            logw = np.asarray(mo["logw"], dtype=np.float64)
        elif "omega" in mo:
            with np.errstate(divide="ignore"):
                logw = np.log(np.asarray(mo["omega"], dtype=np.float64))
        else:
            logw = np.full(K, -np.log(K))
        out["scale"][g] = float(mo.get("scale", 1.0))
        for j in range(K):
            n = int(ns[j])
            red = dict(A=np.asarray(mo["A"])[j:j + 1, :n, :n], prior=prior[j:j + 1, :n],
                       centres=np.asarray(mo["centres"])[j:j + 1, :n], covars=cov[j:j + 1, :n])
            k = host.vhem_cluster_constants(red, COV_DIAG)
            c = c0 + j
            out["nstates_r"][c] = n
            out["logw"][c] = logw[j]
            out["logA"][c, :n, :n] = k["logA"][0]
            out["logPi"][c, :n] = k["logPi"][0]
            out["m"][c, :n] = k["m"][0]
            out["P"][c, :n] = k["P"][0]
            out["c"][c, :n] = k["c"][0]
        c0 += K
    return out


def _loglik_fused(base: BaseSet, pk: dict, T: int, device, want_pairs: bool):
    """vbhmm_dic_loglik; None when the library answers VBHEM_ERR_UNSUPPORTED."""
    lib = _capi.lib()
    dv = torch.device(device)
    b = base.to(dv)
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dv)
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dv)
    keep = [b.nstates.to(torch.int32).contiguous(), b.prior.to(torch.float64).contiguous(),
            b.A.to(torch.float64).contiguous(), b.centres.to(torch.float64).contiguous(),
            b.covars.to(torch.float64).contiguous()]
    bt = _capi.BaseT(base.N, base.SB, base.d, base.covmode, *[_capi.ptr(t) for t in keep], None)
    dev = {k: (i32 if k in ("model_off", "nstates_r") else f64)(pk[k])
           for k in ("model_off", "nstates_r", "logw", "scale", "logA", "logPi", "m", "P", "c")}
    mt = _capi.DicModelsT(pk["G"], pk["C"], pk["S"], pk["d"], pk["max_model_clusters"],
                          *[_capi.ptr(dev[k]) for k in ("model_off", "nstates_r", "logw", "scale",
                                                        "logA", "logPi", "m", "P", "c")])
    nb = int(lib.vbhmm_dic_workspace_bytes(ctypes.byref(bt), ctypes.byref(mt), int(T)))
    ws = _capi.workspace(nb, dv, align=16)
    LL = torch.empty((pk["G"],), dtype=torch.float64, device=dv)
    Lp = torch.empty((base.N, pk["C"]), dtype=torch.float64, device=dv) if want_pairs else None
    st = _capi.stream(dv)
    rc = lib.vbhmm_dic_loglik(ctypes.byref(bt), ctypes.byref(mt), int(T), _capi.ptr(LL),
                              _capi.ptr(Lp), _capi.ptr(ws), ws.numel(), st)
    if rc == VBHEM_ERR_UNSUPPORTED:
        return None
    _capi.check(rc, "vbhmm_dic_loglik")
    return LL, Lp


def _loglik_pairs(base: BaseSet, pk: dict, T: int, device, want_pairs: bool):
    """The path without the fused kernel: every model through EStepEngine.pairs(smooth=1)
    (one call per cluster size of the model: a launch's clusters share one S), then
    logw + scale * L, the log-sum-exp (max first) and the sum over subjects in torch."""
    from .estep import EStepEngine
    dv = torch.device(device)
    engines = {}
    LL = torch.empty((pk["G"],), dtype=torch.float64, device=dv)
    Lp = torch.empty((base.N, pk["C"]), dtype=torch.float64, device=dv) if want_pairs else None
    logw = torch.as_tensor(pk["logw"], device=dv)
    for g in range(pk["G"]):
        c0, c1 = int(pk["model_off"][g]), int(pk["model_off"][g + 1])
        ns = pk["nstates_r"][c0:c1]
        L = torch.empty((base.N, c1 - c0), dtype=torch.float64, device=dv)
        for n in sorted(set(int(x) for x in ns)):
            idx = np.flatnonzero(ns == n)
            key = (len(idx), n)
            if key not in engines:
                engines[key] = EStepEngine(base, len(idx), n, int(T), device=dv)
            eng = engines[key]
            cc = c0 + idx
            eng.set_clusters(dict(logA=pk["logA"][cc][:, :n, :n], logPi=pk["logPi"][cc][:, :n],
                                  m=pk["m"][cc][:, :n], P=pk["P"][cc][:, :n], c=pk["c"][cc][:, :n]))
            L[:, torch.as_tensor(idx, device=dv)] = eng.pairs(smooth=1.0)["LL_elbo"]
        if Lp is not None:
            Lp[:, c0:c1] = L
        val = logw[c0:c1][None, :] + float(pk["scale"][g]) * L
        mx = val.max(dim=1, keepdim=True).values
        LL[g] = (mx[:, 0] + torch.log(torch.exp(val - mx).sum(dim=1))).sum()
    return LL, Lp


def loglik_grid(hmms, models: Sequence[dict], T: int, device="cuda", engine: str = "fused",
                return_pairs: bool = False):
    """LL [G] (a device tensor): LL[g] = sum_i LSE_{c in model g}(logw[c] + scale[g] L(i,c)),
    L the VHEM expected log-likelihood (diag, smooth = 1, tau = T) of subject HMM i under
    group HMM c.  ``hmms``: subject HMM dicts (through vhem.hmms_to_h3m(hmms, 'diag')) or
    a diag BaseSet.  engine 'fused': one launch of vbhmm_dic_loglik; 'pairs': the loop
    over EStepEngine.pairs, also taken when the library reports the shape unsupported
    (S > 16).  return_pairs: also L [N][C]."""
    if engine not in ("fused", "pairs"):
        raise ValueError("engine must be 'fused' or 'pairs'")
    base = _as_base(hmms)
    pk = pack_models(models)
    if pk["d"] != base.d:
        raise ValueError("the models' dimension differs from the subject HMMs'")
    out = _loglik_fused(base, pk, T, device, return_pairs) if engine == "fused" else None
    if out is None:
        out = _loglik_pairs(base, pk, T, device, return_pairs)
    return out if return_pairs else out[0]


# ----------------------------------------------------------------------------
# DIC (myDIC.m)
# ----------------------------------------------------------------------------
def _fit_fields(model):
    """post, syn, Nj, point, hyp of a fit: cluster.vbhem_h3m_c's dict (``result``: an
    EMResult, ``hyp``) or an EMResult."""
    hyp = None
    if isinstance(model, dict):
        hyp = model.get("hyp")
        model = model["result"]
    if model.point is None or model.syn is None:
        raise ValueError("the fit has no point estimates (unstable model)")
    return model.post, model.syn, np.asarray(model.Nj, dtype=np.float64), model.point, hyp


def _lambda0(hyp, lambda0):
    if hyp is not None:
        return float(hyp["vbopt"]["lambda0"])
    if lambda0 is None:
        raise ValueError("my_dic: the fit carries no learned hyperparameters "
                         "(hyp['vbopt']['lambda0']); pass lambda0")
    return float(lambda0)


def dic_penalty(model, lambda0: Optional[float] = None) -> float:
    """P_d of myDIC.m:29-96, 156."""
    post, syn, Nj, point, hyp = _fit_fields(model)
    l0 = _lambda0(hyp, lambda0)
    K, S, d = post.m.shape
    q = np.arange(1, d + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        logOmegaTilde = digamma(post.alpha) - digamma(post.alpha.sum())
        term_omega = float(Nj @ (np.log(np.asarray(point["omega"])) - logOmegaTilde))
        term_pi = term_eps = term_mu = term_W = 0.0
        for i in range(K):
            eta = post.eta[i]
            logPiTilde = digamma(eta) - digamma(eta.sum())
            term_pi += float(syn["Nj_rho1"][i] @ (np.log(point["prior"][i]) - logPiTilde))
            e2 = 0.0
            for k in range(S):
                eps = post.epsilon[i, k]
                logEpsTilde = digamma(eps) - digamma(eps.sum())
                e2 += float(syn["Nj_rho2rho"][i, k] @ (np.log(point["A"][i, k]) - logEpsTilde))
            term_eps += e2
            term_mu += float((l0 / post.lam[i]).sum())
            w2 = 0.0
            for k in range(S):
                W = post.W[i, k]
                Wf = W if W.ndim == 2 else np.diag(W)
                v = post.v[i, k]
                logLambdaTilde = digamma(0.5 * (v + 1) - 0.5 * q).sum() + d * np.log(2.0) \
                    + np.log(np.linalg.det(Wf))
                logLambdaHat = np.log(np.linalg.det(v * Wf))
                w2 += 0.5 * syn["Nj_rho"][i, k] * (logLambdaHat - logLambdaTilde)
            term_W += float(w2)
        term_mu = -0.5 * term_mu
    return float(2.0 * (term_omega + term_pi + term_eps + term_mu + term_W))


def dic_model(model, Kb: int) -> dict:
    """The mixture myDIC.m:160-169 scores: the point group HMMs with the diagonals of
    their covariances, UNIFORM weights 1 / K (hmms_to_h3m's omega, not the fit's), and
    scale Ni = sum(Nj) / Kb."""
    _, _, Nj, point, _ = _fit_fields(model)
    K = int(np.asarray(point["prior"]).shape[0])
    return dict(prior=np.asarray(point["prior"]), A=np.asarray(point["A"]),
                centres=np.asarray(point["centres"]), covars=_diag_covars(point["covars"]),
                logw=np.log(np.ones(K) / K),
                scale=float(Nj.sum() / Kb))


def _default_loglik(device, engine) -> Callable:
    return lambda base, models, T: loglik_grid(base, models, T, device, engine).cpu().numpy()


def my_dic(hmms, model, T: int, dt: int = 0, lambda0: Optional[float] = None, device="cuda",
           engine: str = "fused", loglik: Optional[Callable] = None):
    """myDIC.m (issyn = 0): (P_d, DIC) of one VBHEM fit.  ``hmms``: the subject HMMs
    (None = an empty entry, kept as the one-state dummy and counted in Kb, as the
    reference does).  lambda0: the fit's learned hyp['vbopt']['lambda0'], else this
    argument (a missing one is an error).  ``loglik(base, models, T) -> [G]`` replaces
    the device likelihood (tests).  IEEE results (-inf, NaN) are returned."""
    P_d, DIC, _ = _dic_cells(hmms, [model], T, dt, lambda0, device, engine, loglik)
    return float(P_d[0]), float(DIC[0])


def _dic_cells(hmms, fits: List, T, dt, lambda0, device, engine, loglik):
    base = _as_base(hmms)
    Kb = base.N
    P_d = np.array([dic_penalty(f, lambda0) for f in fits])
    models = [dic_model(f, Kb) for f in fits]
    fn = loglik or _default_loglik(device, engine)
    LL = np.asarray(fn(base, models, int(T)), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        DIC = 2.0 * P_d - 2.0 * (LL / T if dt else LL)
    return P_d, DIC, LL


def grid_cells(clustered: dict):
    """[len_K][len_S] fits of vbhem_h3m_cluster's output: cell (k, s) is
    model_all[k]['model_all_s'][s] (a scalar K or S gives one row or column)."""
    rows = clustered.get("model_all", [clustered])
    return [row.get("model_all_s", [row]) for row in rows]


def dic_grid(hmms, clustered: dict, T: int, dt: int = 0, lambda0: Optional[float] = None,
             device="cuda", engine: str = "fused", loglik: Optional[Callable] = None) -> dict:
    """evaluate_vbhem_jounarl.m:135-153: P_d and DIC of every cell of the K x S grid of
    ``vbhem_h3m_cluster``.  The penalties are host math; the likelihoods of ALL cells
    come from one vbhmm_dic_loglik launch.  Returns P_d, DIC ([len_K][len_S]), LL,
    argmin = (k, s) of the smallest DIC (NaN skipped) and the K, S lists."""
    cells = grid_cells(clustered)
    nK, nS = len(cells), len(cells[0])
    flat = [c for row in cells for c in row]
    P_d, DIC, LL = _dic_cells(hmms, flat, T, dt, lambda0, device, engine, loglik)
    P_d, DIC, LL = P_d.reshape(nK, nS), DIC.reshape(nK, nS), LL.reshape(nK, nS)
    arg = None if np.all(np.isnan(DIC)) else tuple(int(x) for x in
                                                   np.unravel_index(np.nanargmin(DIC), DIC.shape))
    return dict(P_d=P_d, DIC=DIC, LL=LL, argmin=arg,
                K=[int(row[0]["K"]) if isinstance(row[0], dict) and "K" in row[0] else None
                   for row in cells],
                S=[int(c["S"]) if isinstance(c, dict) and "S" in c else None for c in cells[0]])


# ----------------------------------------------------------------------------
# VHEM BIC / AIC (evaluate_vbhem_jounarl.m:159-235)
# ----------------------------------------------------------------------------
def _vhem_log_ests(cell: dict, Kb: int, Nv: float) -> float:
    Z = np.asarray(cell["Z"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        omega = Z.sum(0) / Kb
        return float((Z * (np.log(omega)[None, :] - np.log(Z + 1e-50)
                           + Nv * np.asarray(cell["L_elbo1"]))).sum())


def _vhem_criterion(grid, K, S, dim, div_T, kind):
    Ks, Ss = [int(k) for k in np.atleast_1d(K)], [int(s) for s in np.atleast_1d(S)]
    opt = grid[0][0]["hemopt"]
    Nv, T = float(opt["Nv"]), int(opt["tau"])
    out = np.zeros((len(Ks), len(Ss)))
    for k, kk in enumerate(Ks):
        for s, ss in enumerate(Ss):
            cell = grid[k][s]
            Kb = np.asarray(cell["Z"]).shape[0]
            le = _vhem_log_ests(cell, Kb, Nv)
            if kind == "bic":
                npar = (kk - 1) + kk * ((ss - 1) + ss * (ss - 1) + ss * 2 * dim)
                pen = np.log(Nv * Kb * T) * npar
            else:
                pen = 2.0 * (kk * ss * (ss + 2 * dim) - 1)
            out[k, s] = pen - 2.0 * (le / T if div_T else le)
    return out


def vhem_bic(grid, K, S, dim: int, div_T: int = 0) -> np.ndarray:
    """BIC [len_K][len_S] of vhem_cluster outputs grid[k][s] (Z, L_elbo1, hemopt):
    log(Nv Kb T) ((K-1) + K ((S-1) + S (S-1) + 2 S dim)) - 2 log_ests [/ T]."""
    return _vhem_criterion(grid, K, S, dim, div_T, "bic")


def vhem_aic(grid, K, S, dim: int, div_T: int = 0) -> np.ndarray:
    """AIC [len_K][len_S]: 2 (K S (S + 2 dim) - 1) - 2 log_ests [/ T]."""
    return _vhem_criterion(grid, K, S, dim, div_T, "aic")


# ----------------------------------------------------------------------------
# vbh3m_remove_empty.m
# ----------------------------------------------------------------------------
def fit_to_h3m(fit) -> dict:
    """A VBHEM fit as the struct vbh3m_remove_empty.m reads: hmm (a list of group HMMs
    with prior, trans, pdf, N, N1, M and varpar alpha = eta, epsilon, beta = lambda, v,
    m, W), omega, Z, L_elbo, Nj, label (0-based), groups, group_size."""
    from .cluster import form_groups
    post, syn, Nj, point, _ = _fit_fields(fit)
    res = fit["result"] if isinstance(fit, dict) else fit
    K, S, d = post.m.shape
    hmms = []
    for j in range(K):
        cov = np.asarray(point["covars"][j])
        hmms.append(dict(
            prior=np.array(point["prior"][j]), trans=np.array(point["A"][j]),
            pdf=[dict(mean=np.array(point["centres"][j, s]),
                      cov=np.array(cov[s]) if cov.ndim == 3 else np.diag(cov[s])) for s in range(S)],
            N=np.array(syn["Nj_rho"][j]), N1=np.array(syn["Nj_rho1"][j]),
            M=np.array(syn["Nj_rho2rho"][j]),
            varpar=dict(alpha=np.array(post.eta[j]), epsilon=np.array(post.epsilon[j]),
                        beta=np.array(post.lam[j]), v=np.array(post.v[j]), m=np.array(post.m[j]),
                        W=np.array(post.W[j]))))
    Z = res.hatZ.cpu().numpy() if isinstance(res.hatZ, torch.Tensor) else np.asarray(res.hatZ)
    Le = res.L_elbo.cpu().numpy() if isinstance(res.L_elbo, torch.Tensor) else np.asarray(res.L_elbo)
    label = np.argmax(Z, axis=1)
    groups, group_size = form_groups(label, K)
    return dict(hmm=hmms, omega=np.array(point["omega"]), Z=Z, L_elbo=Le, Nj=np.array(Nj),
                label=label, groups=groups, group_size=group_size, K=K)


def vbh3m_remove_empty(model: dict, thresh: float = 1.0, sortclusters: str = "f"):
    """vbh3m_remove_empty.m: clusters with Nj (NL when present) < thresh are dropped,
    omega renormalised, Z, L_elbo, Nj, the labels, groups and group_size remapped; then
    every group HMM loses its states with N < 1e-3 (vbhmm_remove_empty) and is reordered
    by vbhmm_standardize(., sortclusters).  ``model``: :func:`fit_to_h3m`'s dict.
    Returns (model_out, emptyinds) with 0-based indices."""
    from .vbhmm_em import vbhmm_remove_empty, vbhmm_standardize
    key = "NL" if "NL" in model else "Nj"
    N = np.asarray(model[key], dtype=np.float64).reshape(-1)
    check = N < thresh
    zinds, nz = np.flatnonzero(check), np.flatnonzero(~check)
    out = dict(model)
    if zinds.size:
        out["hmm"] = [model["hmm"][j] for j in nz]
        om = np.asarray(model["omega"], dtype=np.float64)[nz]
        out["omega"] = om / om.sum()
        out["Z"] = np.asarray(model["Z"])[:, nz]
        out[key] = N[nz]
        out["L_elbo"] = np.asarray(model["L_elbo"])[:, nz]
        old = np.asarray(model["label"])
        lab = old.copy()          # (:47-49: labels of removed clusters keep their old number)
        for new, j in enumerate(nz):
            lab[old == j] = new
        out["label"] = lab
        out["groups"] = [model["groups"][j] for j in nz]
        out["group_size"] = np.asarray(model["group_size"])[nz]
        out["K"] = int(nz.size)
    hm = []
    for h in out["hmm"]:
        had_gamma = "gamma" in h
        g = vbhmm_remove_empty(h if had_gamma else dict(h, gamma=[]), 1e-3)
        g = vbhmm_standardize(g, sortclusters)
        if not had_gamma:
            g = {k: v for k, v in g.items() if k != "gamma"}
        hm.append(g)
    out["hmm"] = hm
    return out, zinds
