"""PPK spectral clustering of HMMs: the probability product kernel Gram matrix on
the GPU, then spectral clustering of it.

The reference's src/compare_mtds/ppk: ppk_sc.m, elkernel.m, bhatt.m and
SpectralClustering.m -- the third method (beside VHEM and CCFD) that the paper's
synthetic experiment clusters the subject HMMs with.

:class:`PpkSet` is a set of H point HMMs prepared for the kernel and resident on
the device (include/vbhmm_ppk.h); :func:`ppk_matrix` fills the Gram matrix between
two such sets (or of one set with itself) in one launch;
:func:`spectral_clustering` and :func:`ppk_sc_from_gram` are host code on the
Gram matrix; :func:`ppk_sc` is ppk_sc.m end to end.  Indices are 0-based.  The
Gram matrix has no CPU path: the HIP library must load.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch

from . import _capi
from .h3m import BaseSet, kmeans_pp
from .score import PreparedSet, _as_list

F64 = torch.float64
MODE_RECT, MODE_SYM, MODE_DIAG = 0, 1, 2  # include/vbhmm_ppk.h
KMEANS_MAX_ITER = 200                     # SpectralClustering.m:89-90


class PpkSet(PreparedSet):
    """H point HMMs prepared for the probability product kernel (regularised
    covariances ``cov + pad`` on every entry plus ``1e-5 trace I``, their
    log-determinants, ``prior ** rho``, ``trans ** rho``) and resident on ``device``.
    ``hmms``: a list of HMM dicts (``prior``, ``trans``, ``pdf[{mean, cov}]``; ragged
    state counts; one dimension), or a packed :class:`BaseSet`, whose device arrays
    are read where they are.  At most 16 states and 8 dimensions.  A regularised
    covariance that is not positive definite raises :class:`_capi.VbhemError` naming
    the HMM and the state."""

    def __init__(self, hmms, rho: float = 0.5, pad: float = 0.45, device="cuda"):
        self._load(hmms, device)
        self.rho, self.pad = float(rho), float(pad)
        self._alloc_prepared(self.lib.vbhmm_ppk_prepared_bytes)
        _capi.check(self.lib.vbhmm_ppk_prepare(ctypes.byref(self._desc), self.rho, self.pad,
                                               _capi.ptr(self.prepared), self.prepared.numel() * 8,
                                               self._stream()),
                    "vbhmm_ppk_prepare")


def _gram(a: PpkSet, b: PpkSet, T: int, mode: int) -> torch.Tensor:
    shape = (a.H,) if mode == MODE_DIAG else (a.H, b.H)
    out = torch.empty(shape, dtype=F64, device=a.device)
    _capi.check(a.lib.vbhmm_ppk_gram(ctypes.byref(a.desc()), _capi.ptr(a.prepared), ctypes.byref(b.desc()),
                                     _capi.ptr(b.prepared), int(T), mode, _capi.ptr(out), a._stream()),
                "vbhmm_ppk_gram")
    return out


def ppk_matrix(a: PpkSet, b: Optional[PpkSet] = None, T: int = 10, normalize: bool = False) -> torch.Tensor:
    """The Gram matrix ``K[i][j] = elkernel(a_i, b_j, T, rho)``, ``[Ha][Hb]`` (device,
    fp64), one launch.  ``b=None``: the set with itself -- only the pairs i <= j are
    computed and the result is bitwise symmetric.  ``normalize`` divides by
    ``sqrt(K(a_i, a_i) K(b_j, b_j))``; the default is the reference's raw kernel,
    which carries T + 1 affinity factors and is not bounded by 1."""
    if b is not None:
        if (b.rho, b.pad) != (a.rho, a.pad) or b.prepared.device != a.prepared.device:
            raise ValueError("the two sets must be prepared with the same rho and pad on one device")
    K = _gram(a, a, T, MODE_SYM) if b is None else _gram(a, b, T, MODE_RECT)
    if normalize:
        da = _gram(a, a, T, MODE_DIAG)
        db = da if b is None else _gram(b, b, T, MODE_DIAG)
        K = K / torch.sqrt(da[:, None] * db[None, :])
    return K


def spectral_clustering(A, k: int, type: int = 3, seed=None):
    """SpectralClustering.m on the affinity matrix ``A`` [n][n]: (labels [n] 0-based,
    centres [k][k], U [n][k]).  Degrees are ``sum(A, 2)``, zeros replaced by eps.
    type 1: the raw matrix; 2: ``D^-1 A``; 3: ``D^-1/2 A D^-1/2`` with the rows of U
    normalised to unit length (NaN -> 0).  U holds the k eigenvectors of largest
    |eigenvalue|: for types 1 and 3 of the symmetrised matrix (``eigh``); for type 2
    of the non-symmetric ``D^-1 A`` (``eig``), which is symmetrised and solved again
    only if they come out complex (SpectralClustering.m:64-70).  The rows of U are
    then clustered by :func:`h3m.kmeans_pp` on ``default_rng(seed)`` with 200
    iterations, the stand-in for MATLAB's kmeans('start', 'cluster'): parity
    unpinned."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("A must be a square matrix")
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError("need 1 <= k <= number of rows")
    if type not in (1, 2, 3):
        raise ValueError("type must be 1 (raw), 2 (D^-1 A) or 3 (D^-1/2 A D^-1/2)")
    degs = A.sum(axis=1)
    L = A
    if type != 1:
        degs = np.where(degs == 0, np.finfo(np.float64).eps, degs)
    with np.errstate(all="ignore"):
        if type == 2:
            L = A / degs[:, None]
        elif type == 3:
            s = 1.0 / np.sqrt(degs)
            L = s[:, None] * A * s[None, :]

    def top(w, V):
        order = np.argsort(-np.abs(w), kind="stable")[:k]
        return V[:, order]

    def sym_top(M):
        w, V = np.linalg.eigh((M + M.T) / 2)
        return top(w, V)

    if type == 2:
        w, V = np.linalg.eig(L)
        U = top(w, V)
        U = sym_top(L) if np.iscomplexobj(U) and np.abs(U.imag).sum() != 0 else np.real(U)
    else:
        U = sym_top(L)
    if type == 3:
        with np.errstate(all="ignore"):
            U = U / np.sqrt((U ** 2).sum(axis=1, keepdims=True))
        U = np.where(np.isnan(U), 0.0, U)
    U = np.ascontiguousarray(U)
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    centres = kmeans_pp(U, k, rng, max_iter=KMEANS_MAX_ITER)
    labels = np.argmin(((U[None, :, :] - centres[:, None, :]) ** 2).sum(2), axis=0).astype(np.int64)
    return labels, centres, U


def _hmm_list(hmms) -> List[dict]:
    if not isinstance(hmms, BaseSet):
        return _as_list(hmms)
    b = hmms.numpy()
    return [dict(prior=b["prior"][i, :K], trans=b["A"][i, :K, :K],
                 pdf=[dict(mean=b["centres"][i, s], cov=b["covars"][i, s]) for s in range(K)])
            for i, K in enumerate(b["nstates"])]


def ppk_sc_from_gram(hmms, A, K: int, seed=None) -> dict:
    """ppk_sc.m:25-66 on a Gram matrix ``A`` that is already there: spectral
    clustering of type 3, then ``label`` [N] (0-based), ``group`` (K index arrays),
    ``group_size`` [K], ``weight`` = group_size / N, ``Z`` [N][K] (one-hot),
    ``ind_center`` [K] (per cluster the member whose row of U is nearest the cluster's
    centre, the first on ties; -1 for an empty cluster), ``hmms`` (the centre HMMs;
    None for an empty cluster), ``A`` and ``U``."""
    hl = _hmm_list(hmms)
    A = np.asarray(A, dtype=np.float64)
    N = len(hl)
    if A.shape != (N, N):
        raise ValueError("A must be [N][N] for the N HMMs")
    label, centres, U = spectral_clustering(A, K, 3, seed)
    K = int(K)
    Z = np.zeros((N, K))
    Z[np.arange(N), label] = 1.0
    group = [np.nonzero(label == k)[0] for k in range(K)]
    ind = np.full(K, -1, dtype=np.int64)
    for k, g in enumerate(group):
        if len(g):
            dist = np.sqrt(((U[g] - centres[k]) ** 2).sum(axis=1))
            ind[k] = g[int(np.argmin(dist))]
    size = np.array([len(g) for g in group], dtype=np.int64)
    return dict(label=label, group=group, group_size=size, weight=size / N, Z=Z, ind_center=ind,
                hmms=[hl[i] if i >= 0 else None for i in ind], A=A, U=U)


def ppk_sc(hmms, K: int, seed=None, T: int = 10, rho: float = 0.5, device="cuda") -> dict:
    """ppk_sc.m: the Gram matrix of the HMMs under the probability product kernel
    (on the GPU, symmetric mode, the reference's raw kernel), then
    :func:`ppk_sc_from_gram`."""
    A = ppk_matrix(PpkSet(hmms, rho=rho, device=device), None, T).cpu().numpy()
    return ppk_sc_from_gram(hmms, A, K, seed)
