"""CCFD clustering of HMMs: density peaks on the symmetrised KL distance.

The reference's src/compare_mtds/ccfd/myccfd.m and CCFD.m, the fourth method that
Synthetic_experiment/exprmt1_demo.m compares (beside VBHEM, VHEM and PPK-SC):

  :func:`distance_matrix`   D[i][j] = 0.5 (KL(i, j) + KL(j, i)) of myccfd.m:14-30 on the
                            GPU (include/vbhmm_ccfd.h), without the [H][N_total]
                            log-likelihood matrix that ``score.kld_matrix`` stores
  :func:`CCFD`              one density-peak clustering at a cut-off (CCFD.m)
  :func:`myccfd_from_dist`  the search over the cut-off of myccfd.m:42-114
  :func:`myccfd`            both

The O(N^2) sweeps over D (local density, nearest denser point, border density) go
through an engine: :class:`DeviceEngine` runs the HIP kernels on a matrix resident on
the GPU and brings only length-N vectors to the host; :class:`NumpyEngine` serves a
host array.  The O(N) rest of CCFD.m runs on the host in fp64, every sum one addition
after the other in index order.  D is taken to be symmetric (as the reference's own
is); only rows are read.

Indices, centres and labels are 0-based; a halo member is marked -1 where the
reference writes 0.  Failures raise :class:`NoSingularPoints`.
"""
from __future__ import annotations

import ctypes
import sys
from typing import Optional

import numpy as np
import torch

F64 = torch.float64
REALMAX = sys.float_info.max
_UNSET = -2  # a point without a label yet (the reference's -1)


class NoSingularPoints(RuntimeError):
    """CCFD.m's error('NO SINGULAR POINTS'), and the places where MATLAB would stop on
    an index error: a top-ranked point that is no centre, a point left without a
    neighbour, a search whose chosen candidate never succeeded."""


# ----------------------------------------------------------------------------
# engines: the sweeps over D
# ----------------------------------------------------------------------------
def _check_shape(shape):
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError(f"the distance matrix must be square, not {tuple(shape)}")
    if shape[0] < 2:
        raise ValueError("CCFD needs at least 2 points")


class NumpyEngine:
    """The sweeps in numpy over a host matrix."""

    def __init__(self, D):
        self.D = np.ascontiguousarray(D.detach().cpu().numpy() if isinstance(D, torch.Tensor) else D,
                                      dtype=np.float64)
        _check_shape(self.D.shape)
        self.N = self.D.shape[0]

    def finite(self) -> bool:
        return bool(np.isfinite(self.D).all())

    def stats(self):
        """(min(pur), max(pur), maxd): over the entries above the diagonal, and
        max(max(dist)) over the whole matrix."""
        iu = np.triu_indices(self.N, 1)
        pur = self.D[iu]
        return float(pur.min()), float(pur.max()), float(self.D.max())

    def rho(self, dcs) -> np.ndarray:
        diag = np.diagonal(self.D)
        return np.stack([(self.D < dc).sum(axis=1) - (diag < dc) for dc in dcs]).astype(np.int64)

    def delta(self, ranks, maxd):
        N = self.N
        delta, nneigh = np.empty((len(ranks), N)), np.empty((len(ranks), N), dtype=np.int64)
        above = np.tri(N, N, -1, dtype=bool)  # in rank space: column rank < row rank
        for c, rank in enumerate(ranks):
            order = np.argsort(rank)
            P = np.where(above, self.D[np.ix_(order, order)], np.inf)
            at = np.argmin(P, axis=1)  # the first minimum: the lowest rank among equals
            best = P[np.arange(N), at]
            take = best < maxd
            take[0] = False
            delta[c, order] = np.where(take, best, maxd)
            nneigh[c, order] = np.where(take, order[at], -1)
            delta[c, order[0]] = -1.0
        return delta, nneigh

    def border(self, dc, cl, rho) -> np.ndarray:
        hit = (cl[:, None] != cl[None, :]) & (self.D <= dc)
        aver = (rho[:, None].astype(np.float64) + rho[None, :].astype(np.float64)) / 2.0
        return np.where(hit, aver, 0.0).max(axis=1)

    def columns(self, idx) -> np.ndarray:
        return np.ascontiguousarray(self.D[:, np.asarray(idx, dtype=np.int64)])

    def dist(self):
        return self.D


class DeviceEngine:
    """The sweeps as HIP kernels over a matrix resident on a GPU (one workgroup per row;
    include/vbhmm_ccfd.h).  ``rowmin`` / ``rowmax``: the per-row extrema over j > i when
    :func:`distance_matrix`'s kernel already produced them."""

    def __init__(self, D: torch.Tensor, rowmin: Optional[torch.Tensor] = None,
                 rowmax: Optional[torch.Tensor] = None):
        from . import _capi
        if D.device.type != "cuda":
            raise ValueError("DeviceEngine needs a matrix on a GPU")
        _check_shape(D.shape)
        self._capi, self.lib = _capi, _capi.lib()
        self.D = D.to(F64).contiguous()
        self.N, self.device = int(D.shape[0]), D.device
        self._rowmin, self._rowmax = rowmin, rowmax

    def _stream(self):
        return self._capi.stream(self.device)

    def _int(self, a) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def finite(self) -> bool:
        return bool(torch.isfinite(self.D).all())

    def stats(self):
        ptr, check = self._capi.ptr, self._capi.check
        if self._rowmin is None:
            self._rowmin = torch.empty((self.N,), dtype=F64, device=self.device)
            self._rowmax = torch.empty((self.N,), dtype=F64, device=self.device)
            with torch.cuda.device(self.device):
                check(self.lib.vbhmm_ccfd_rowstats(ptr(self.D), self.N, ptr(self._rowmin), ptr(self._rowmax),
                                                   self._stream()), "vbhmm_ccfd_rowstats")
        mn, mx = self._rowmin.cpu().numpy()[:-1], self._rowmax.cpu().numpy()[:-1]
        diag = float(torch.diagonal(self.D).max())
        return float(mn.min()), float(mx.max()), max(float(mx.max()), diag)

    def rho(self, dcs) -> np.ndarray:
        ptr, check = self._capi.ptr, self._capi.check
        C = len(dcs)
        out = torch.empty((C, self.N), dtype=torch.int32, device=self.device)
        cut = (ctypes.c_double * C)(*[float(v) for v in dcs])
        with torch.cuda.device(self.device):
            check(self.lib.vbhmm_ccfd_rho(ptr(self.D), self.N, cut, C, ptr(out), self._stream()), "vbhmm_ccfd_rho")
        return out.cpu().numpy().astype(np.int64)

    def delta(self, ranks, maxd):
        ptr, check = self._capi.ptr, self._capi.check
        C = len(ranks)
        rk = self._int(np.stack(ranks))
        delta = torch.empty((C, self.N), dtype=F64, device=self.device)
        nneigh = torch.empty((C, self.N), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.vbhmm_ccfd_delta(ptr(self.D), self.N, ptr(rk), C, float(maxd), ptr(delta), ptr(nneigh),
                                            self._stream()), "vbhmm_ccfd_delta")
        return delta.cpu().numpy(), nneigh.cpu().numpy().astype(np.int64)

    def border(self, dc, cl, rho) -> np.ndarray:
        ptr, check = self._capi.ptr, self._capi.check
        cl_d, rho_d = self._int(cl), self._int(rho)
        out = torch.empty((self.N,), dtype=F64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.vbhmm_ccfd_border(ptr(self.D), self.N, float(dc), ptr(cl_d), ptr(rho_d), ptr(out),
                                             self._stream()), "vbhmm_ccfd_border")
        return out.cpu().numpy()

    def columns(self, idx) -> np.ndarray:
        at = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.device)
        return self.D.index_select(1, at).cpu().numpy()

    def dist(self):
        return self.D


def make_engine(D, device=None):
    """The engine of a matrix: a tensor on a GPU (or a host array with a ``cuda`` device)
    gets the kernels, anything else numpy."""
    if isinstance(D, (NumpyEngine, DeviceEngine)):
        return D
    if device is not None and torch.device(device).type == "cuda":
        D = D if isinstance(D, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(D, dtype=np.float64))
        return DeviceEngine(D.to(device))
    if isinstance(D, torch.Tensor) and D.device.type == "cuda" and device is None:
        return DeviceEngine(D)
    return NumpyEngine(D)


# ----------------------------------------------------------------------------
# CCFD.m: the O(N) part, on the host
# ----------------------------------------------------------------------------
def _seqsum(a) -> float:
    """One addition after the other, in index order."""
    a = np.asarray(a, dtype=np.float64)
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def rank_of(rho) -> np.ndarray:
    """The position of every point in the stable descending sort of rho (CCFD.m:48)."""
    order = np.argsort(-np.asarray(rho, dtype=np.int64), kind="stable")
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank


def _finish(engine, dc, rho, rank, delta, nneigh, slope, want_halo):
    """CCFD.m:61-256 from the swept vectors of one cut-off."""
    N = engine.N
    order = np.argsort(rank)
    delta = np.array(delta, dtype=np.float64)
    delta[order[0]] = delta.max()  # :61, the placeholder -1 still among the candidates
    rho_f = rho.astype(np.float64)
    gamma = rho_f * delta
    threshold = 2 * (_seqsum(gamma) / N)
    kept = gamma[~(gamma > threshold)]
    if kept.size < 1:
        raise NoSingularPoints("NO SINGULAR POINTS (the trim kept no point)")
    mgamma = _seqsum(kept) / kept.size
    covgamma = _seqsum((kept - mgamma) ** 2) / (kept.size - 1) if kept.size > 1 else 0.0
    five = 5 * np.sqrt(covgamma)
    singid = np.concatenate([np.nonzero(gamma > mgamma + five)[0], np.nonzero(gamma < mgamma - five)[0]])
    if singid.size < 1:
        raise NoSingularPoints("NO SINGULAR POINTS")
    with np.errstate(all="ignore"):
        spread = delta.max() - delta.min()
        den = np.float64((rho_f.max() - rho_f.min()) + rho_f.min())
        k_star1 = (slope * spread + delta.min()) / den
        k_star2 = ((1 / slope) * spread + delta.min()) / den
        is_centre = (rho_f[singid] / delta[singid] < 1 / k_star2) & (delta[singid] / rho_f[singid] < k_star1)
    icl = singid[is_centre].astype(np.int64)
    K = len(icl)
    if K < 1:
        raise NoSingularPoints("NO SINGULAR POINTS (no singular point passed the centre test)")
    cl = np.full(N, _UNSET, dtype=np.int64)
    cl[icl] = np.arange(K)
    for i in order:
        if cl[i] == _UNSET:
            if nneigh[i] < 0:
                raise NoSingularPoints(f"point {int(i)} is no centre and has no denser neighbour below the "
                                       "largest distance")
            cl[i] = cl[nneigh[i]]
    halo = cl.copy()
    if want_halo and K > 1:
        bord = np.zeros(K)
        np.maximum.at(bord, cl, engine.border(dc, cl, rho))
        halo[rho_f < bord[cl]] = -1
    cols = engine.columns(icl)  # [N][K]: all of D that the fitness reads
    fit1 = 0.0
    for j in range(K):
        fit1 = fit1 + _seqsum(cols[cl == j, j]) / N  # the divisor is N, not the cluster's size (:236)
    fit1 = fit1 / K
    fit2 = 0.0
    if K > 1:
        between = cols[icl, :]  # [K][K], dist(icl[a], icl[b])
        tmp = np.triu(between, 1)
        tmp = tmp + tmp.T
        fit2 = _seqsum(tmp.T.reshape(-1)) / K / (K - 1)
    with np.errstate(all="ignore"):
        fitness = float(np.float64(fit2) / np.float64(fit1))
    return dict(fitness=fitness, dc=float(dc), icl=icl, cl=cl, rho=rho.astype(np.int64), delta=delta,
                nneigh=np.asarray(nneigh, dtype=np.int64), halo=halo)


def _run_candidates(engine, stats, dcs, slope, want_halo) -> list:
    """CCFD at up to three cut-offs from one read of D per sweep: a result dict per
    cut-off, or the NoSingularPoints it raised."""
    rho = engine.rho(dcs)
    ranks = [rank_of(r) for r in rho]
    delta, nneigh = engine.delta(ranks, stats[2])
    out = []
    for c, dc in enumerate(dcs):
        try:
            out.append(_finish(engine, dc, rho[c], ranks[c], delta[c], nneigh[c], slope, want_halo))
        except NoSingularPoints as e:
            out.append(e)
    return out


def _prepare(D, device=None):
    engine = make_engine(D, device)
    if not engine.finite():
        raise ValueError("the distance matrix holds a NaN or an infinity")
    return engine, engine.stats()


def _cutoff(stats, percent) -> float:
    return stats[0] + (stats[1] - stats[0]) * percent / 100


def CCFD(D, percent, slope=3, dc=None, device=None) -> dict:
    """CCFD.m at one cut-off: ``dc``, or min(pur) + (max(pur) - min(pur)) percent / 100
    over the entries above D's diagonal.  Returns fitness, dc, icl (the centres), cl
    (labels), rho, delta, nneigh (-1: none), halo (-1: in the halo)."""
    engine, stats = _prepare(D, device)
    res = _run_candidates(engine, stats, [_cutoff(stats, percent) if dc is None else float(dc)], slope, True)[0]
    if isinstance(res, NoSingularPoints):
        raise res
    return res


def myccfd_from_dist(D, hmms=None, slope=3, device=None) -> dict:
    """The search of myccfd.m:42-77 over the cut-off and the final call, on a finished
    distance matrix (a tensor on a GPU: the kernels; a host array: numpy).  Returns
    ``ccfd_result`` (fitness, percent, dc, icl, cl, rho, delta, NCLUST, halo, dist, k),
    ``hmms`` (the centres' HMMs, when ``hmms`` is given), ``label``, ``groups``, ``weight``."""
    engine, stats = _prepare(D, device)
    percent, r, cofr = 10.0, 3.0, (-1, 0, 1)
    slots = [None, None, None]  # persist across rounds, as dc(i), icl{i}, cl{i} do
    fitidx = 2
    while r > 0:
        got = _run_candidates(engine, stats, [_cutoff(stats, percent + r * c) for c in cofr], slope, False)
        fitness = []
        for i, res in enumerate(got):
            if isinstance(res, NoSingularPoints):
                fitness.append(-REALMAX)
            else:
                fitness.append(res["fitness"])
                slots[i] = res
        best = max(fitness)
        fitidx = 2 if all(f == best for f in fitness) else fitness.index(best)
        percent = percent + r * cofr[fitidx]
        r = r - 0.5
    if slots[fitidx] is None:
        raise NoSingularPoints("the search's chosen candidate never succeeded")
    star = _run_candidates(engine, stats, [slots[fitidx]["dc"]], slope, True)[0]
    if isinstance(star, NoSingularPoints):
        raise star
    icl, label = slots[fitidx]["icl"], slots[fitidx]["cl"]
    K = len(icl)
    groups = [np.nonzero(label == i)[0] for i in range(K)]
    size = np.array([len(g) for g in groups], dtype=np.float64)
    result = dict(fitness=star["fitness"], percent=percent, dc=star["dc"], icl=icl, cl=label, rho=star["rho"],
                  delta=star["delta"], NCLUST=K, halo=star["halo"], dist=engine.dist(), k=slope)
    return dict(ccfd_result=result, hmms=None if hmms is None else [hmms[int(i)] for i in icl], label=label,
                groups=groups, weight=size / size.sum())


# ----------------------------------------------------------------------------
# the distance
# ----------------------------------------------------------------------------
def _distance_batch(hset, sb, counts):
    """(D [H][H], rowmin [H], rowmax [H]) on the device from a prepared HmmSet, a
    SequenceBatch of all subjects' trials one subject after the other, and the number
    of trials of every subject."""
    from . import _capi
    dv, H = hset.device, hset.H
    if len(counts) != H or int(np.sum(counts)) != sb.N:
        raise ValueError("trials_by_subject needs one list of sequences per HMM")
    seg = np.zeros(H + 1, dtype=np.int32)
    seg[1:] = np.cumsum(counts)
    seg_d = torch.from_numpy(seg).to(dv)
    lib = hset.lib
    nb = int(lib.vbhmm_ccfd_distance_workspace_bytes(H, sb.N))
    ws = torch.empty((max(nb, 16) // 8,), dtype=F64, device=dv)
    D = torch.empty((H, H), dtype=F64, device=dv)
    rowmin, rowmax = torch.empty((H,), dtype=F64, device=dv), torch.empty((H,), dtype=F64, device=dv)
    sd = sb.desc()
    with torch.cuda.device(dv):
        _capi.check(lib.vbhmm_ccfd_distance(ctypes.byref(hset.desc()), _capi.ptr(hset.prepared), ctypes.byref(sd),
                                            _capi.ptr(seg_d), _capi.ptr(ws), ws.numel() * 8, _capi.ptr(D),
                                            _capi.ptr(rowmin), _capi.ptr(rowmax), hset._stream()),
                    "vbhmm_ccfd_distance")
    return D, rowmin, rowmax


def _distance(hmms, trials_by_subject, device="cuda"):
    from .score import HmmSet, _as_list
    from .vbhmm import SequenceBatch
    hset = hmms if isinstance(hmms, HmmSet) else HmmSet(hmms, device)
    groups = [_as_list(g) for g in trials_by_subject]
    if len(groups) != hset.H:
        raise ValueError("trials_by_subject needs one list of sequences per HMM")
    sb = SequenceBatch([s for g in groups for s in g], hset.dim, hset.device)
    return _distance_batch(hset, sb, [len(g) for g in groups])


def distance_matrix(hmms, trials_by_subject, device="cuda") -> torch.Tensor:
    """``D[i][j] = D[j][i] = 0.5 (KL(i, j) + KL(j, i))``, ``D[i][i] = 0``, ``[H][H]`` fp64 on
    the device; KL(i, j) = the mean over subject i's trials of ll_i / T - ll_j / T
    (vbhmm_kld with 'n').  ``hmms``: a list of HMM dicts or a :class:`score.HmmSet`;
    ``trials_by_subject[i]``: the sequences of HMM i.  A subject without trials, or an
    empty trial, gives NaN.  Memory: H^2 + N_total doubles, never H * N_total."""
    return _distance(hmms, trials_by_subject, device)[0]


def myccfd(hmms, trials_by_subject, slope=3, device="cuda") -> dict:
    """myccfd.m: the distance on the GPU, then the search on the matrix where it lies."""
    D, rowmin, rowmax = _distance(hmms, trials_by_subject, device)
    from .score import HmmSet
    return myccfd_from_dist(DeviceEngine(D, rowmin, rowmax), None if isinstance(hmms, HmmSet) else list(hmms), slope)
