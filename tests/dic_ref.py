"""Plain-loop restatement of the reference's model-selection criteria, written from the
reference text (never from vbhem_amd/dic.py), and the loaders the DIC tests share.

* :func:`my_dic` -- src/compare_mtds/dic/myDIC.m, issyn = 0, statement by statement, on
  a struct laid out like the reference's h3m (:func:`fit_struct` builds it from a fit).
  The likelihood part takes the per-pair matrix L_elbo [Kb][K] as an argument, so any
  engine (the oracle, the host check build, the GPU) can supply it.
* :func:`vhem_bic` / :func:`vhem_aic` -- Synthetic_experiment/evaluate_vbhem_jounarl.m:159-235.
* :func:`vbh3m_remove_empty` -- src/vbhem/vbh3m_remove_empty.m with
  src/hmm/vbhmm_remove_empty.m and the 'f' order of vbhmm_standardize.m.
* :func:`oracle_pairs`, :func:`mix`, :func:`load_diccheck`, :func:`host_pairs`,
  :func:`device_loglik` -- L and LL of a packed grid of models from the oracle, from loops,
  from the host build of csrc/vbhmm_dic_pair.h and from the library on the GPU.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
from scipy.special import digamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICCHECK_PATH = os.path.join(ROOT, "tests", "diccheck", "libdiccheck.so")


# ----------------------------------------------------------------------------
# myDIC.m
# ----------------------------------------------------------------------------
def logtrick(col):
    """logtrick.m on one column: max first, then the sum in index order."""
    mv = max(col)
    acc = 0.0
    for x in col:
        acc += math.exp(x - mv)
    return mv + math.log(acc)


def fit_struct(res, hyp=None) -> dict:
    """The fields myDIC.m reads, named as the reference names them, from an EM result
    (post, syn, Nj, point): h3m.K, .alpha, .omega, .Nj, .learn_hyps.vbopt.lambda0 and per
    group HMM .N1, .M, .N, .prior, .trans, .pdf{k}.mean / .cov, .varpar.alpha (= eta),
    .epsilon, .beta (= lambda), .W, .v."""
    post, syn, point = res.post, res.syn, res.point
    K, S, d = post.m.shape
    hmm = []
    for i in range(K):
        W = [post.W[i, k] if post.W[i, k].ndim == 2 else np.diag(post.W[i, k]) for k in range(S)]
        cov = [point["covars"][i, k] if np.ndim(point["covars"][i, k]) == 2
               else np.diag(point["covars"][i, k]) for k in range(S)]
        hmm.append(dict(N1=syn["Nj_rho1"][i], M=syn["Nj_rho2rho"][i], N=syn["Nj_rho"][i],
                        prior=point["prior"][i], trans=point["A"][i],
                        pdf=[dict(mean=point["centres"][i, k], cov=cov[k]) for k in range(S)],
                        varpar=dict(alpha=post.eta[i], epsilon=post.epsilon[i], beta=post.lam[i],
                                    W=W, v=post.v[i])))
    out = dict(K=K, alpha=post.alpha, omega=point["omega"], Nj=res.Nj, hmm=hmm)
    if hyp is not None:
        out["learn_hyps"] = dict(vbopt=dict(lambda0=hyp["vbopt"]["lambda0"]))
    return out


def penalty(h3m: dict) -> float:
    """myDIC.m:25-96, 156."""
    K = h3m["K"]
    gamma0 = h3m["learn_hyps"]["vbopt"]["lambda0"]          # :25 (fails when absent)
    dim = len(h3m["hmm"][0]["pdf"][0]["mean"])
    alpha = h3m["alpha"]
    psiAlphaHat = digamma(sum(alpha))
    term_omega = 0.0
    for j in range(K):                                       # :37-40
        term_omega += h3m["Nj"][j] * (math.log(h3m["omega"][j]) - (digamma(alpha[j]) - psiAlphaHat))
    term_pi = 0.0
    for i in range(K):                                       # :45-54
        h = h3m["hmm"][i]
        etai = h["varpar"]["alpha"]
        psiEtaHat = digamma(sum(etai))
        for k in range(len(etai)):
            term_pi += h["N1"][k] * (math.log(h["prior"][k]) - (digamma(etai[k]) - psiEtaHat))
    term_eps = 0.0
    for i in range(K):                                       # :58-70
        h = h3m["hmm"][i]
        eps = h["varpar"]["epsilon"]
        for k in range(eps.shape[0]):
            psiEpsHat = digamma(sum(eps[k]))
            for l in range(eps.shape[1]):
                term_eps += h["M"][k][l] * (math.log(h["trans"][k][l]) - (digamma(eps[k][l]) - psiEpsHat))
    term_mu = 0.0
    for i in range(K):                                       # :73-78
        for g in h3m["hmm"][i]["varpar"]["beta"]:
            term_mu += gamma0 / g
    term_mu = -0.5 * term_mu
    term_W = 0.0
    for i in range(K):                                       # :82-96
        h = h3m["hmm"][i]
        for k in range(len(h["prior"])):
            Wk, vk = h["varpar"]["W"][k], h["varpar"]["v"][k]
            t1 = 0.0
            for q in range(1, dim + 1):
                t1 += digamma(0.5 * (vk + 1) - 0.5 * q)
            logLambdaTilde = t1 + dim * math.log(2) + math.log(np.linalg.det(Wk))
            logLambdahat = math.log(np.linalg.det(vk * Wk))
            term_W += 0.5 * h["N"][k] * (logLambdahat - logLambdaTilde)
    return 2 * (term_omega + term_pi + term_eps + term_mu + term_W)


def my_dic(h3m: dict, L_elbo, T: int, dt: int = 0):
    """myDIC.m:156-177 with L_elbo [Kb][K] given: (P_d, DIC).  The weights are
    hmms_to_h3m(h3m.hmm).omega = 1 / K (:160, :169), Ni = sum(Nj) / Kb (:21)."""
    P_d = penalty(h3m)
    K = h3m["K"]
    Kb = len(L_elbo)
    Ni = sum(h3m["Nj"]) / Kb
    omega2 = [1.0 / K] * K
    new_LL = 0.0
    for i in range(Kb):
        new_LL += logtrick([math.log(omega2[j]) + Ni * L_elbo[i][j] for j in range(K)])
    if dt:
        return P_d, 2 * P_d - 2 * new_LL / T
    return P_d, 2 * P_d - 2 * new_LL


# ----------------------------------------------------------------------------
# VHEM BIC / AIC
# ----------------------------------------------------------------------------
def _log_ests(cell, Kb, Nv):
    Z, L1 = cell["Z"], cell["L_elbo1"]
    K = len(Z[0])
    omega = [sum(Z[i][j] for i in range(Kb)) / Kb for j in range(K)]
    tot = 0.0
    for i in range(Kb):
        for j in range(K):
            tot += Z[i][j] * (math.log(omega[j]) - math.log(Z[i][j] + 1e-50) + Nv * L1[i][j])
    return tot


def vhem_bic(grid, K, S, dim, div_T=0):
    """evaluate_vbhem_jounarl.m:159-199."""
    Nv, T = grid[0][0]["hemopt"]["Nv"], grid[0][0]["hemopt"]["tau"]
    out = [[0.0] * len(S) for _ in K]
    for k, kk in enumerate(K):
        for s, ss in enumerate(S):
            Kb = len(grid[k][s]["Z"])
            N_bic = Nv * Kb * T
            Num_pars = (kk - 1) + kk * ((ss - 1) + ss * (ss - 1) + ss * 2 * dim)
            le = _log_ests(grid[k][s], Kb, Nv)
            out[k][s] = math.log(N_bic) * Num_pars - 2 * le / T if div_T else math.log(N_bic) * Num_pars - 2 * le
    return out


def vhem_aic(grid, K, S, dim, div_T=0):
    """evaluate_vbhem_jounarl.m:202-235."""
    Nv, T = grid[0][0]["hemopt"]["Nv"], grid[0][0]["hemopt"]["tau"]
    out = [[0.0] * len(S) for _ in K]
    for k, kk in enumerate(K):
        for s, ss in enumerate(S):
            Kb = len(grid[k][s]["Z"])
            Num_pars = kk * ss * (ss + 2 * dim) - 1
            le = _log_ests(grid[k][s], Kb, Nv)
            out[k][s] = 2 * Num_pars - 2 * le / T if div_T else 2 * Num_pars - 2 * le
    return out


# ----------------------------------------------------------------------------
# vbh3m_remove_empty.m
# ----------------------------------------------------------------------------
def _hmm_remove_empty(h, thresh):
    """vbhmm_remove_empty.m:33-97 (no groups, no gamma)."""
    nz = [k for k in range(len(h["N"])) if not h["N"][k] < thresh]
    if len(nz) == len(h["N"]):
        return h
    vp = h["varpar"]
    o = dict(h)
    o["varpar"] = dict(alpha=[vp["alpha"][k] for k in nz],
                       epsilon=[[vp["epsilon"][k][l] for l in nz] for k in nz],
                       beta=[vp["beta"][k] for k in nz], v=[vp["v"][k] for k in nz],
                       m=[vp["m"][k] for k in nz], W=[vp["W"][k] for k in nz])
    o["M"] = [[h["M"][k][l] for l in nz] for k in nz]
    o["N1"] = [h["N1"][k] for k in nz]
    o["N"] = [h["N"][k] for k in nz]
    sa = sum(o["varpar"]["alpha"])
    o["prior"] = [a / sa for a in o["varpar"]["alpha"]]
    o["trans"] = [[e / sum(row) for e in row] for row in o["varpar"]["epsilon"]]
    o["pdf"] = [h["pdf"][k] for k in nz]
    return o


def _fixation_order(h):
    """vbhmm_standardize.m 'f': the prior's argmax, then each row's argmax among the
    states not visited yet."""
    A = [list(r) for r in h["trans"]]
    n = len(h["prior"])
    order = []
    for t in range(n):
        row = list(h["prior"]) if t == 0 else A[order[-1]]
        cur = max(range(n), key=lambda k: (row[k], -k))
        order.append(cur)
        for r in A:
            r[cur] = -1.0
    return order


def vbh3m_remove_empty(h3m, thresh=1.0):
    """vbh3m_remove_empty.m:15-83 with sortclusters = 'f'.  Returns (h3mo, emptyinds,
    per-HMM kept original state indices in their final order) -- 0-based."""
    N = h3m["NL"] if "NL" in h3m else h3m["Nj"]
    zinds = [j for j in range(len(N)) if N[j] < thresh]
    nz = [j for j in range(len(N)) if not N[j] < thresh]
    o = dict(h3m)
    if zinds:
        o["hmm"] = [h3m["hmm"][j] for j in nz]
        om = [h3m["omega"][j] for j in nz]
        o["omega"] = [x / sum(om) for x in om]
        o["Z"] = [[row[j] for j in nz] for row in h3m["Z"]]
        o["Nj"] = [N[j] for j in nz]
        o["L_elbo"] = [[row[j] for j in nz] for row in h3m["L_elbo"]]
        lab = list(h3m["label"])
        for new, j in enumerate(nz):
            for i in range(len(lab)):
                if h3m["label"][i] == j:
                    lab[i] = new
        o["label"] = lab
        o["groups"] = [h3m["groups"][j] for j in nz]
        o["group_size"] = [h3m["group_size"][j] for j in nz]
    kept = []
    hm = []
    for h in o["hmm"]:
        idx = [k for k in range(len(h["N"])) if not h["N"][k] < 1e-3]
        g = _hmm_remove_empty(h, 1e-3)
        order = _fixation_order(g)
        kept.append([idx[k] for k in order])
        hm.append(g)
    o["hmm"] = hm
    return o, zinds, kept


# ----------------------------------------------------------------------------
# engines for L and LL of a packed grid (vbhem_amd.dic.pack_models layout)
# ----------------------------------------------------------------------------
def oracle_pairs(vo, base: dict, models, T: int) -> np.ndarray:
    """L [N][C]: every cluster against the oracle's VHEM E-step (diag, smooth = 1) run on
    its first n states, as test_vhem_gateway_mixed_cluster_sizes does."""
    cols = []
    for mo in models:
        K = np.asarray(mo["prior"]).shape[0]
        ns = mo.get("nstates", [np.asarray(mo["prior"]).shape[1]] * K)
        for j in range(K):
            n = int(ns[j])
            rj = dict(A=np.ascontiguousarray(np.asarray(mo["A"])[j:j + 1, :n, :n]),
                      prior=np.ascontiguousarray(np.asarray(mo["prior"])[j:j + 1, :n]),
                      centres=np.ascontiguousarray(np.asarray(mo["centres"])[j:j + 1, :n]),
                      covars=np.ascontiguousarray(np.asarray(mo["covars"])[j:j + 1, :n]))
            cols.append(vo.c_vhem_estep_pairs(base, rj, T, 1.0)["LL_elbo"][:, 0])
    return np.stack(cols, axis=1)


def mix(L, model_off, logw, scale):
    """LL [G] = sum_i logtrick_c(logw[c] + scale[g] L[i][c]) in loops."""
    out = []
    for g in range(len(model_off) - 1):
        tot = 0.0
        for i in range(len(L)):
            tot += logtrick([logw[c] + scale[g] * L[i][c] for c in range(model_off[g], model_off[g + 1])])
        out.append(tot)
    return np.array(out)


_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def load_diccheck():
    if not os.path.exists(DICCHECK_PATH):
        subprocess.run(["make", "-C", ROOT, "diccheck"], check=True, stdout=subprocess.DEVNULL)
    import torch  # noqa: F401  (the HIP runtime torch loaded is the one the library binds to)
    lib = ctypes.CDLL(DICCHECK_PATH)
    lib.diccheck_pairs_host.restype = ctypes.c_int
    lib.diccheck_pairs_host.argtypes = [ctypes.c_int] * 3 + [_ip] + [_dp] * 4 + [ctypes.c_int] * 2 + [_ip] + \
        [_dp] * 5 + [ctypes.c_int] * 2 + [_dp, _ip]
    lib.diccheck_mix_host.restype = None
    lib.diccheck_mix_host.argtypes = [ctypes.c_int] * 3 + [_ip, _dp, _dp, _dp, _dp]
    lib.diccheck_workspace_bytes.restype = ctypes.c_size_t
    lib.diccheck_workspace_bytes.argtypes = [ctypes.c_int] * 9
    lib.diccheck_loglik_device.restype = ctypes.c_int
    lib.diccheck_loglik_device.argtypes = [ctypes.c_int] * 4 + [_ip] + [_dp] * 4 + [ctypes.c_int] * 4 + \
        [_ip, _ip] + [_dp] * 7 + [ctypes.c_int, _dp, _dp]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def host_pairs(lib, base: dict, pk: dict, T: int, exact_only: bool = False):
    """(L [N][C], pairs recomputed in reference order) from pair_serial on the host."""
    N, SB = base["prior"].shape
    d = base["centres"].shape[2]
    ns, pr, A, cen, cov = _i(base["nstates"]), _d(base["prior"]), _d(base["A"]), _d(base["centres"]), \
        _d(base["covars"])
    nr, lA, lP, m, P, c = _i(pk["nstates_r"]), _d(pk["logA"]), _d(pk["logPi"]), _d(pk["m"]), _d(pk["P"]), \
        _d(pk["c"])
    L = np.zeros((N, pk["C"]))
    rec = ctypes.c_int(0)
    rc = lib.diccheck_pairs_host(N, SB, d, _p(ns, _ip), _p(pr, _dp), _p(A, _dp), _p(cen, _dp), _p(cov, _dp),
                                 pk["C"], pk["S"], _p(nr, _ip), _p(lA, _dp), _p(lP, _dp), _p(m, _dp),
                                 _p(P, _dp), _p(c, _dp), int(T), int(exact_only), _p(L, _dp), ctypes.byref(rec))
    assert rc == 0, rc
    return L, rec.value


def host_mix(lib, L, pk: dict) -> np.ndarray:
    L = _d(L)
    off, lw, sc = _i(pk["model_off"]), _d(pk["logw"]), _d(pk["scale"])
    LL = np.zeros(pk["G"])
    lib.diccheck_mix_host(L.shape[0], pk["C"], pk["G"], _p(off, _ip), _p(lw, _dp), _p(sc, _dp), _p(L, _dp),
                          _p(LL, _dp))
    return LL


def device_loglik(lib, base: dict, pk: dict, T: int, want_pairs: bool = True, covmode: int = 0):
    """(status, LL [G], L [N][C] or None) from vbhmm_dic_loglik on device 0."""
    N, SB = base["prior"].shape
    d = base["centres"].shape[2]
    ns, pr, A, cen, cov = _i(base["nstates"]), _d(base["prior"]), _d(base["A"]), _d(base["centres"]), \
        _d(base["covars"])
    off, nr, lw, sc = _i(pk["model_off"]), _i(pk["nstates_r"]), _d(pk["logw"]), _d(pk["scale"])
    lA, lP, m, P, c = _d(pk["logA"]), _d(pk["logPi"]), _d(pk["m"]), _d(pk["P"]), _d(pk["c"])
    LL = np.full(pk["G"], np.nan)
    L = np.full((N, pk["C"]), np.nan) if want_pairs else None
    rc = lib.diccheck_loglik_device(N, SB, d, covmode, _p(ns, _ip), _p(pr, _dp), _p(A, _dp), _p(cen, _dp),
                                    _p(cov, _dp), pk["G"], pk["C"], pk["S"], pk["max_model_clusters"],
                                    _p(off, _ip), _p(nr, _ip), _p(lw, _dp), _p(sc, _dp), _p(lA, _dp),
                                    _p(lP, _dp), _p(m, _dp), _p(P, _dp), _p(c, _dp), int(T), _p(LL, _dp),
                                    _p(L, _dp) if want_pairs else None)
    return rc, LL, L
