"""Numpy loop restatement of the reference's probability product kernel -- the judge
of tests/test_ppk.py and tests/test_ppk_gpu.py -- written from the formulas of
src/compare_mtds/ppk/elkernel.m, bhatt.m and ppk_sc.m:17-22 in their loop order:

  C = cov + pad on every entry (a vector cov is a diagonal matrix first),
  C += 1e-5 trace(C) I;
  bhatt (literal): iC1 = inv(C1), iC2 = inv(C2), Cd = inv(iC1 + iC2),
      Md = iC1 mu1 + iC2 mu2,
      2^(d/2) det(C1)^(-1/4) det(C2)^(-1/4) sqrt(det(Cd))
      exp(-(mu1' iC1 mu1 + mu2' iC2 mu2 - Md' Cd Md) / 4);
  bhatt (difference form, what the library computes): C1 + C2 = R'R, y = R' \\ (mu1 - mu2),
      exp(d/2 ln 2 + logdet(C1)/4 + logdet(C2)/4 - sum log diag R - |y|^2 / 4);
  T == 1: K = sum_ij p_i r_j pot_ij;  else sep = sum_ij (p_i r_j)^rho pot_ij
      (A_i.^rho)' (B_j.^rho), then T - 1 times sep = sum_ij sep_ij pot_ij (A_i' B_j).^rho,
      K = sum(sep o pot).

Also the shared cases, their cached Grams and the loader of the host check build.
"""
import ctypes
import functools
import os

import numpy as np
from scipy.linalg import solve_triangular

import score_ref as sr

RHO, PAD, T_DEFAULT = 0.5, 0.45, 10


# ----------------------------------------------------------------------------
# restatement
# ----------------------------------------------------------------------------
def reg_cov(cov, d, pad=PAD):
    c = np.asarray(cov, dtype=np.float64)
    C = (c.reshape(d, d) if c.size == d * d and (c.ndim == 2 or d == 1) else np.diag(c.reshape(-1))) + pad
    return C + 1e-5 * np.trace(C) * np.eye(d)


def bhatt_literal(mu1, mu2, C1, C2):
    """bhatt.m's expression, C1 and C2 already regularised."""
    n = len(mu1)
    iC1, iC2 = np.linalg.inv(C1), np.linalg.inv(C2)
    Cd = np.linalg.inv(iC1 + iC2)
    Md = iC1 @ mu1 + iC2 @ mu2
    rho = 0.5
    normalizer = (2 * np.pi) ** ((1 - 2 * rho) * (n / 2)) * rho ** (-n / 2)
    normalizer = normalizer * np.linalg.det(C1) ** (-rho / 2) * np.linalg.det(C2) ** (-rho / 2) \
        * np.sqrt(np.linalg.det(Cd))
    with np.errstate(under="ignore"):
        return normalizer * np.exp((-rho / 2) * (mu1 @ iC1 @ mu1 + mu2 @ iC2 @ mu2 - Md @ Cd @ Md))


def bhatt_diff(mu1, mu2, C1, C2):
    """The same affinity in the difference form."""
    n = len(mu1)
    R = np.linalg.cholesky(C1 + C2).T
    y = solve_triangular(R.T, mu1 - mu2, lower=True)
    ld = lambda C: 2.0 * np.sum(np.log(np.diag(np.linalg.cholesky(C))))
    with np.errstate(under="ignore"):
        return np.exp(n / 2 * np.log(2.0) + ld(C1) / 4 + ld(C2) / 4 - np.sum(np.log(np.diag(R))) - y @ y / 4)


def pot_matrix(h1, h2, pad=PAD, bhatt=bhatt_diff):
    M, N = len(h1["pdf"]), len(h2["pdf"])
    d = len(np.reshape(h1["pdf"][0]["mean"], -1))
    C1 = [reg_cov(p["cov"], d, pad) for p in h1["pdf"]]
    C2 = [reg_cov(p["cov"], d, pad) for p in h2["pdf"]]
    pot = np.zeros((M, N))
    for i in range(M):
        for j in range(N):
            pot[i, j] = bhatt(np.reshape(h1["pdf"][i]["mean"], -1).astype(np.float64),
                              np.reshape(h2["pdf"][j]["mean"], -1).astype(np.float64), C1[i], C2[j])
    return pot


def pow_rho(x, rho):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(x == 0, 0.0, x ** rho)


def elkernel(h1, h2, T=T_DEFAULT, rho=RHO, pad=PAD, bhatt=bhatt_diff):
    p1, p2 = np.reshape(h1["prior"], -1), np.reshape(h2["prior"], -1)
    A1, A2 = np.asarray(h1["trans"], dtype=np.float64), np.asarray(h2["trans"], dtype=np.float64)
    M, N = len(p1), len(p2)
    pot = pot_matrix(h1, h2, pad, bhatt)
    with np.errstate(under="ignore"):
        if T == 1:
            K = 0.0
            for i in range(M):
                for j in range(N):
                    K = K + p1[i] * p2[j] * pot[i, j]
            return K
        sep1 = np.zeros((M, N))
        for i in range(M):
            for j in range(N):
                sep1 = sep1 + pow_rho(p1[i] * p2[j], rho) * pot[i, j] * np.outer(pow_rho(A1[i], rho),
                                                                                 pow_rho(A2[j], rho))
        for _ in range(2, T + 1):
            sep2 = np.zeros((M, N))
            for i in range(M):
                for j in range(N):
                    sep2 = sep2 + sep1[i, j] * pot[i, j] * pow_rho(np.outer(A1[i], A2[j]), rho)
            sep1 = sep2
        return float(np.sum(sep1 * pot))


def gram(ha, hb=None, T=T_DEFAULT, rho=RHO, pad=PAD, bhatt=bhatt_diff):
    """ppk_sc.m:17-22: every pair, no symmetry used."""
    hb = ha if hb is None else hb
    return np.array([[elkernel(a, b, T, rho, pad, bhatt) for b in hb] for a in ha])


# ----------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------
def ragged_counts(K, H):
    return ([K, max(1, K // 2), max(1, K - 1)] * ((H + 2) // 3))[:H]


@functools.lru_cache(maxsize=None)
def make_set(K, d, diag, H=3, seed=0, spread=4.0, scale=1.0, centre=0.0):
    """H HMMs of ragged state counts (the largest K), as score_ref.make_case draws them."""
    rng = np.random.default_rng(4000 * K + 10 * d + int(diag) + 7919 * seed + 17 * H)
    return [sr.make_hmm(rng, k, d, diag, spread, scale, centre) for k in ragged_counts(K, H)]


@functools.lru_cache(maxsize=None)
def reference(K, d, diag, H=3, seed=0, T=T_DEFAULT, rho=RHO):
    return gram(make_set(K, d, diag, H, seed), None, T, rho)


def shifted(hmms, shift):
    return [dict(prior=h["prior"], trans=h["trans"],
                 pdf=[dict(mean=np.asarray(p["mean"]) + shift, cov=p["cov"]) for p in h["pdf"]]) for h in hmms]


@functools.lru_cache(maxsize=None)
def grid_set(K=5, d=3, diag=False, H=4):
    """HMMs whose means are multiples of 2^-16, so that a shift by 2^12 is exact."""
    out = []
    for h in make_set(K, d, diag, H, seed=3):
        out.append(dict(prior=h["prior"], trans=h["trans"],
                        pdf=[dict(mean=np.round(np.asarray(p["mean"]) * 65536.0) / 65536.0, cov=p["cov"])
                             for p in h["pdf"]]))
    return out


@functools.lru_cache(maxsize=None)
def families(K, d, F, n, seed=0, diag=False):
    """F prototypes (make_hmm with centre 10 f), n copies each with the means jittered
    by N(0, 0.2): (hmms, family of each)."""
    rng = np.random.default_rng(100 * K + 10 * d + F + 1000 * seed)
    hmms, fam = [], []
    for f in range(F):
        proto = sr.make_hmm(rng, K, d, diag, centre=10.0 * f)
        for _ in range(n):
            hmms.append(dict(prior=proto["prior"], trans=proto["trans"],
                             pdf=[dict(mean=p["mean"] + rng.normal(0, 0.2, d), cov=p["cov"])
                                  for p in proto["pdf"]]))
            fam.append(f)
    return hmms, np.array(fam)


@functools.lru_cache(maxsize=None)
def families_gram(K, d, F, n, seed=0):
    return gram(families(K, d, F, n, seed)[0])


def one_label_per_family(label, fam):
    F = len(set(fam.tolist()))
    return all(len(set(label[fam == f].tolist())) == 1 for f in range(F)) and len(set(label.tolist())) == F


# ----------------------------------------------------------------------------
# the host build of the pair routines (tests/ppkcheck/libppkcheck.so)
# ----------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPKCHECK_PATH = os.path.join(ROOT, "tests", "ppkcheck", "libppkcheck.so")
MODE_RECT, MODE_SYM, MODE_DIAG = 0, 1, 2


def load_ppkcheck():
    if not os.path.exists(PPKCHECK_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "ppkcheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(PPKCHECK_PATH)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    args = [ci, ci, cd, cd, ci, ci] + [ci, ci] + [vp] * 5 + [ci, ci] + [vp] * 5 + [vp]
    lib.ppkcheck_host.argtypes = args
    lib.ppkcheck_host.restype = ctypes.c_longlong
    lib.ppkcheck_device.argtypes = args
    lib.ppkcheck_device.restype = ctypes.c_int
    return lib


def run_ppkcheck(lib, pa, pb=None, T=T_DEFAULT, rho=RHO, pad=PAD, mode=None, device=False):
    """(status, Gram) of the packed sets (score.pack_hmms) through the host loop (or the
    kernels).  pb None: the symmetric mode of pa (or ``mode`` = MODE_DIAG)."""
    if mode is None:
        mode = MODE_SYM if pb is None else MODE_RECT
    pb = pa if pb is None else pb
    assert pa["covmode"] == pb["covmode"] and pa["mean"].shape[2] == pb["mean"].shape[2]
    d = pa["mean"].shape[2]
    Ha, KMa = pa["prior"].shape
    Hb, KMb = pb["prior"].shape
    out = np.full((Ha,) if mode == MODE_DIAG else (Ha, Hb), 7.0)
    keep = [np.ascontiguousarray(p[k]) for p in (pa, pb) for k in ("nstates", "prior", "trans", "mean", "cov")]
    fn = lib.ppkcheck_device if device else lib.ppkcheck_host
    rc = fn(d, int(pa["covmode"]), rho, pad, T, mode, Ha, KMa, *[a.ctypes.data for a in keep[:5]],
            Hb, KMb, *[a.ctypes.data for a in keep[5:]], out.ctypes.data)
    return int(rc), out
