"""Scoring sequences under HMMs on the GPU: log-likelihood, Viterbi path, KL.

What a user runs once HMMs are learned (``vbhmm_em``) or clustered
(``cluster``): the reference's src/hmm/vbhmm_ll.m, vbhmm_map_state.m,
vbhmm_kld.m, vbhmm_random_sample.m and vbhmm_prob_state.m.

:class:`HmmSet` is a set of H point HMMs prepared and resident on the device
(include/vbhmm_score.h); :func:`ll_matrix` scores N sequences under all of
them in one launch (``[H][N]``), :func:`viterbi` decodes them, and
:func:`mean_ll` / :func:`kld_matrix` reduce such a matrix per subject.  The
reference-named wrappers take and return host data.  State indices are 0-based
everywhere (the reference's are 1-based).  There is no CPU path: the HIP
library must load.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _capi
from .h3m import COV_DIAG, COV_FULL, BaseSet
from .vbhmm import SequenceBatch

F64 = torch.float64
MAX_STATES, MAX_DIM = 16, 8


# ----------------------------------------------------------------------------
# HMM dicts (prior, trans, pdf[{mean, cov}])
# ----------------------------------------------------------------------------
def _hmm_arrays(hmm: dict):
    """(prior [K], trans [K][K], mean [K][d], covs: K arrays, [d] (diagonal) or [d][d])."""
    prior = np.asarray(hmm["prior"], dtype=np.float64).reshape(-1)
    K = prior.shape[0]
    trans = np.asarray(hmm["trans"], dtype=np.float64).reshape(K, K)
    pdf = list(hmm["pdf"])
    if len(pdf) != K:
        raise ValueError(f"hmm has {K} prior entries but {len(pdf)} emission densities")
    mean = np.stack([np.asarray(p["mean"], dtype=np.float64).reshape(-1) for p in pdf])
    d = mean.shape[1]
    covs = []
    for p in pdf:
        c = np.asarray(p["cov"], dtype=np.float64)
        if c.size == d * d and (c.ndim == 2 or d == 1):
            c = c.reshape(d, d)
        elif c.size == d:
            c = c.reshape(d)  # a vector is a diagonal covariance (mvnpdf)
        else:
            raise ValueError(f"cov of shape {c.shape} does not fit a {d}-dimensional mean")
        covs.append(c)
    return prior, trans, mean, covs


def group_hmms(post) -> List[dict]:
    """The group HMMs of a clustering result (``res["result"].post``, a
    :class:`h3m.Posterior`) as point-HMM dicts, by convert_h3mrtoh3mb.m:9-72 and
    form_outputH3M.m:35-41: prior = eta / sum(eta), trans = epsilon rows normalised
    (an all-zero row stays zero), mean = m, cov = sym(W^-1) / (v - d - 1)
    (/ v when v <= d + 1); a diagonal W gives a vector cov."""
    eta, eps = np.asarray(post.eta, dtype=np.float64), np.asarray(post.epsilon, dtype=np.float64)
    v, m, W = (np.asarray(a, dtype=np.float64) for a in (post.v, post.m, post.W))
    K, S, d = m.shape
    out = []
    for j in range(K):
        scale = eps[j].sum(axis=1, keepdims=True)
        pdf = []
        for k in range(S):
            den = v[j, k] - d - 1 if v[j, k] > d + 1 else v[j, k]
            if W.ndim == 4:
                tC = np.linalg.inv(W[j, k]) / den
                cov = (tC + tC.T) / 2
            else:
                cov = (1.0 / W[j, k]) / den
            pdf.append(dict(mean=m[j, k].copy(), cov=cov))
        out.append(dict(prior=eta[j] / eta[j].sum(), trans=eps[j] / np.where(scale == 0, 1.0, scale),
                        pdf=pdf))
    return out


def _as_list(data) -> list:
    return list(data) if isinstance(data, (list, tuple)) else [data]


class PreparedSet:
    """What :class:`HmmSet` and :class:`ppk.PpkSet` share: H point HMMs as the five
    device arrays of include/vbhmm_score.h, their descriptor, and a prepared buffer
    sized by the subclass's ``*_prepared_bytes``.  The subclass fills the buffer."""

    def _load(self, hmms, device):
        """``hmms`` (HMM dicts or a :class:`BaseSet`) onto ``device``; the descriptor."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} lives on a GPU (HIP); there is no CPU path")
        self.lib = _capi.lib()
        dv = self.device
        if isinstance(hmms, BaseSet):
            b = hmms.to(dv)
            self.nstates = b.nstates.to(torch.int32).contiguous()
            self.prior, self.trans = b.prior.to(F64).contiguous(), b.A.to(F64).contiguous()
            self.mean, self.cov = b.centres.to(F64).contiguous(), b.covars.to(F64).contiguous()
            self.covmode = int(b.covmode)
        else:
            packed = pack_hmms(_as_list(hmms))
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dv)
            self.nstates, self.prior, self.trans = t(packed["nstates"]), t(packed["prior"]), t(packed["trans"])
            self.mean, self.cov, self.covmode = t(packed["mean"]), t(packed["cov"]), packed["covmode"]
        self.H, self.KM, self.dim = (int(s) for s in self.mean.shape)
        self._desc = _capi.ScoreHmmsT(self.H, self.KM, self.dim, self.covmode, _capi.ptr(self.nstates),
                                      _capi.ptr(self.prior), _capi.ptr(self.trans),
                                      _capi.ptr(self.mean), _capi.ptr(self.cov))

    def _alloc_prepared(self, prepared_bytes):
        nb = int(prepared_bytes(ctypes.byref(self._desc)))
        self.prepared = torch.empty((max(nb, 8) // 8,), dtype=F64, device=self.device)

    def _stream(self):
        return _capi.stream(self.device)

    def desc(self) -> "_capi.ScoreHmmsT":
        return self._desc


class HmmSet(PreparedSet):
    """H point HMMs, prepared (Cholesky factors inverted, log-normalisers) and
    resident on ``device``.  ``hmms``: a list of HMM dicts (``prior``, ``trans``,
    ``pdf[{mean, cov}]``; ragged state counts; all of one dimension), or a packed
    :class:`BaseSet`, whose device arrays are read where they are.  At most 16
    states and 8 dimensions.  A covariance that is not positive definite raises
    :class:`_capi.VbhemError` naming the HMM and the state."""

    def __init__(self, hmms, device="cuda"):
        self._load(hmms, device)
        if self.KM > MAX_STATES or self.dim > MAX_DIM:
            raise ValueError(f"at most {MAX_STATES} states and {MAX_DIM} dimensions are supported")
        self._alloc_prepared(self.lib.vbhmm_score_prepared_bytes)
        _capi.check(self.lib.vbhmm_score_prepare(ctypes.byref(self._desc), _capi.ptr(self.prepared),
                                                 self.prepared.numel() * 8, self._stream()),
                    "vbhmm_score_prepare")


def pack_hmms(hmms: List[dict]) -> dict:
    """HMM dicts as the padded host arrays of include/vbhmm_score.h: nstates [H],
    prior [H][KM], trans [H][KM][KM], mean [H][KM][d], cov [H][KM][d][d] (any
    covariance a matrix) or [H][KM][d] (all diagonal), covmode."""
    arrs = [_hmm_arrays(h) for h in hmms]
    if not arrs:
        raise ValueError("no HMMs")
    H, KM, d = len(arrs), max(a[0].shape[0] for a in arrs), arrs[0][2].shape[1]
    if any(a[2].shape[1] != d for a in arrs):
        raise ValueError("the HMMs of a set must have one dimension")
    full = any(c.ndim == 2 for a in arrs for c in a[3])
    nstates = np.array([a[0].shape[0] for a in arrs], dtype=np.int32)
    prior, trans, mean = np.zeros((H, KM)), np.zeros((H, KM, KM)), np.zeros((H, KM, d))
    cov = np.zeros((H, KM, d, d)) if full else np.zeros((H, KM, d))
    for h, (p, A, m, cs) in enumerate(arrs):
        K = p.shape[0]
        prior[h, :K], trans[h, :K, :K], mean[h, :K] = p, A, m
        for k, c in enumerate(cs):
            cov[h, k] = (np.diag(c) if c.ndim == 1 else c) if full else c
    return dict(nstates=nstates, prior=prior, trans=trans, mean=mean, cov=cov,
                covmode=COV_FULL if full else COV_DIAG)


def _batch(hset: HmmSet, data) -> SequenceBatch:
    if isinstance(data, SequenceBatch):
        if data.dim != hset.dim or data.x.device != hset.prepared.device:
            raise ValueError("the batch must have the HMMs' dimension and device")
        return data
    return SequenceBatch(_as_list(data), hset.dim, hset.device)


def _lengths(batch: SequenceBatch) -> torch.Tensor:
    return (batch.offsets[1:] - batch.offsets[:-1]).to(F64)


def ll_matrix(hset: HmmSet, batch, normalize: bool = True) -> torch.Tensor:
    """Log-likelihood of every sequence under every HMM, ``[H][N]`` (device, fp64),
    one launch.  ``normalize`` divides by the sequence lengths (vbhmm_ll's 'n':
    an empty sequence gives NaN; 0 without)."""
    sb = _batch(hset, batch)
    out = torch.empty((hset.H, sb.N), dtype=F64, device=hset.device)
    sd = sb.desc()
    _capi.check(hset.lib.vbhmm_score_ll(ctypes.byref(hset.desc()), _capi.ptr(hset.prepared),
                                        ctypes.byref(sd), _capi.ptr(out), hset._stream()),
                "vbhmm_score_ll")
    return out / _lengths(sb)[None, :] if normalize else out


def viterbi(hset: HmmSet, batch):
    """(path [H][sum T] int32, loglik [H][N]): the most probable 0-based state path
    of every sequence under every HMM (sequence n at path[h, offsets[n]:offsets[n+1]])
    and the scaled recursion's -sum log(scale)."""
    sb = _batch(hset, batch)
    total = int(sb.x.shape[0])
    path = torch.zeros((hset.H, total), dtype=torch.int32, device=hset.device)
    ll = torch.empty((hset.H, sb.N), dtype=F64, device=hset.device)
    nb = int(hset.lib.vbhmm_score_workspace_bytes(ctypes.byref(hset.desc()), total))
    ws = _capi.workspace(nb, hset.device, align=16)
    sd = sb.desc()
    _capi.check(hset.lib.vbhmm_score_viterbi(ctypes.byref(hset.desc()), _capi.ptr(hset.prepared),
                                             ctypes.byref(sd), total, _capi.ptr(path), _capi.ptr(ll),
                                             _capi.ptr(ws), ws.numel(), hset._stream()),
                "vbhmm_score_viterbi")
    return path, ll


def _segment_mean(v: torch.Tensor, counts: Sequence[int]) -> torch.Tensor:
    """Mean of v [H][N] over consecutive column segments of ``counts`` -> [H][S]
    (an empty segment gives NaN).  A padded gather and a masked sum: the order is
    fixed and a NaN or infinity stays in its own segment."""
    cnt = torch.as_tensor(np.asarray(counts, dtype=np.int64), device=v.device)
    S, L = cnt.numel(), max(int(max(counts, default=0)), 1)
    start = torch.cumsum(cnt, 0) - cnt
    j = torch.arange(L, device=v.device)
    mask = j[None, :] < cnt[:, None]
    idx = torch.where(mask, start[:, None] + j[None, :], torch.zeros_like(mask, dtype=torch.int64))
    if v.shape[1] == 0:
        return torch.full((v.shape[0], S), float("nan"), dtype=v.dtype, device=v.device)
    vals = torch.where(mask[None], v[:, idx], torch.zeros((), dtype=v.dtype, device=v.device))
    return vals.sum(-1) / cnt.to(v.dtype)[None, :]


def mean_ll(hset: HmmSet, data_by_subject, normalize: bool = True) -> torch.Tensor:
    """``[H][subjects]``: each subject's mean log-likelihood (over its sequences)
    under each HMM -- the assignment of subjects to group HMMs (argmax over H)."""
    groups = [_as_list(g) for g in data_by_subject]
    ll = ll_matrix(hset, [s for g in groups for s in g], normalize)
    return _segment_mean(ll, [len(g) for g in groups])


def kld_matrix(hmms, data_by_hmm, normalize: bool = True, device="cuda") -> torch.Tensor:
    """``D[i][j] = mean_n(ll_i(data_i) - ll_j(data_i))`` (vbhmm_kld for every pair),
    ``[H][H]``, from one ll_matrix launch over the concatenated data.  ``hmms``: a
    list of HMM dicts or an :class:`HmmSet`; ``data_by_hmm[i]``: the sequences of HMM i."""
    hset = hmms if isinstance(hmms, HmmSet) else HmmSet(hmms, device)
    groups = [_as_list(g) for g in data_by_hmm]
    if len(groups) != hset.H:
        raise ValueError("data_by_hmm needs one list of sequences per HMM")
    counts = [len(g) for g in groups]
    ll = ll_matrix(hset, [s for g in groups for s in g], normalize)
    owner = torch.repeat_interleave(torch.arange(hset.H, device=ll.device),
                                    torch.as_tensor(counts, device=ll.device))
    own = ll[owner, torch.arange(ll.shape[1], device=ll.device)]
    return _segment_mean(own[None, :] - ll, counts).T.contiguous()


def kld_jobs(hset: HmmSet, batch, lists, jobs) -> torch.Tensor:
    """Many vbhmm_kld values in one fused call (include/vbhmm_kld.h), ``[P]`` fp64 on the
    device: for job p = ``jobs[p]`` = (a, b, list),
    ``kl[p] = mean over n in lists[list] of (ll_a(n) / T_n - ll_b(n) / T_n)``.
    ``lists``: a list of int sequences, indices into ``batch`` (sequences or a
    :class:`SequenceBatch`) in any order, repeats allowed; ``jobs``: ``[P][3]`` ints.  An
    empty list or an empty sequence in it gives NaN.  No ``[H][N]`` matrix is built:
    work and memory follow the sum of the jobs' list lengths.  An index out of range
    raises :class:`_capi.VbhemError` naming it, before anything runs on the device."""
    sb = _batch(hset, batch)
    jb = np.ascontiguousarray(np.asarray(jobs, dtype=np.int64).reshape(-1, 3))
    ls = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
    flat = np.concatenate(ls) if ls else np.zeros(0, dtype=np.int64)
    for a in (jb, flat):
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("kld_jobs: an index does not fit 32 bits")
    jb, items = jb.astype(np.int32), np.ascontiguousarray(flat.astype(np.int32))
    off = np.zeros(len(ls) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(l) for l in ls])
    P = int(jb.shape[0])
    out = torch.empty((P,), dtype=F64, device=hset.device)
    lib = hset.lib
    nb = int(lib.vbhmm_kld_jobs_workspace_bytes(len(ls), off.ctypes.data, P, jb.ctypes.data))
    ws = _capi.workspace(nb, hset.device, align=16)
    sd = sb.desc()
    with torch.cuda.device(hset.device):
        _capi.check(lib.vbhmm_kld_jobs(ctypes.byref(hset.desc()), _capi.ptr(hset.prepared), ctypes.byref(sd),
                                       len(ls), off.ctypes.data, items.ctypes.data if items.size else None, P,
                                       jb.ctypes.data, _capi.ptr(ws), ws.numel(), _capi.ptr(out),
                                       hset._stream()),
                    "vbhmm_kld_jobs")
    return out


# ----------------------------------------------------------------------------
# reference-named wrappers (host data in and out)
# ----------------------------------------------------------------------------
def vbhmm_ll(hmm: dict, data, opt: str = "n", device="cuda"):
    """vbhmm_ll.m: (loglik [N], errors [N]) of the sequences ``data`` (a list of
    [T x d] arrays, or one) under ``hmm``; opt 'n' (default) normalises by the
    lengths, '' does not.  errors = isinf(loglik)."""
    hset = HmmSet([hmm], device)
    ll = ll_matrix(hset, _as_list(data), "n" in opt)[0].cpu().numpy()
    return ll, np.isinf(ll)


def vbhmm_map_state(hmm: dict, data, device="cuda") -> List[np.ndarray]:
    """vbhmm_map_state.m: the most probable state sequence of every sequence, as
    int arrays of 0-based state indices (the reference returns 1-based ROIs)."""
    hset = HmmSet([hmm], device)
    seqs = _as_list(data)
    path, _ = viterbi(hset, seqs)
    p = path[0].cpu().numpy()
    lens = [int(np.asarray(a).reshape(-1, hset.dim).shape[0]) for a in seqs]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [p[off[n]:off[n + 1]].astype(np.int64) for n in range(len(seqs))]


def vbhmm_kld(hmm1: dict, hmm2: dict, data1, opt: str = "n", seed=None, device="cuda"):
    """vbhmm_kld.m: (kld, ll1, ll2, data1), kld = mean(ll1 - ll2).  ``data1``: the
    sequences of hmm1, or [N, T]: sample N sequences of length T from hmm1
    (vbhmm_random_sample with ``seed``)."""
    if not isinstance(data1, (list, tuple)) or (len(data1) == 2 and all(np.ndim(v) == 0 for v in data1)):
        nt = np.asarray(data1).reshape(-1)  # not a list of sequences: [N, T] (vbhmm_kld.m:36-40)
        if nt.size != 2:
            raise ValueError("data1 must be a list of sequences or [N, T]")
        _, data1 = vbhmm_random_sample(hmm1, int(nt[1]), int(nt[0]), seed)
    ll = ll_matrix(HmmSet([hmm1, hmm2], device), list(data1), "n" in opt).cpu().numpy()
    ll1, ll2 = ll[0], ll[1]
    return float(np.mean(ll1 - ll2)), ll1, ll2, data1


def multirnd(cumprob, f) -> int:
    """vbhmm_random_sample.m:76-79 with the uniform given: the 0-based index
    sum(f > cumprob) (f equal to a cumulative boundary stays below it)."""
    return int(np.sum(f > np.asarray(cumprob, dtype=np.float64)))


def vbhmm_random_sample(hmm: dict, T, N: int, seed=None):
    """vbhmm_random_sample.m: (h, data), N hidden-state sequences (0-based) and
    their observations.  T: a length, or a vector with T[j] = P(length = j + 1).
    Draws come from numpy's ``default_rng(seed)`` in the reference's order (per
    sequence: the length, then the states; then per state the emissions of every
    sequence, randn(n, d) L' + mean with L the lower Cholesky factor); MATLAB's
    random stream is not reproduced."""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    prior, trans, mean, covs = _hmm_arrays(hmm)
    K, d = mean.shape
    cumprior, cumtrans = np.cumsum(prior), np.cumsum(trans, axis=1)
    cumT = None if np.ndim(T) == 0 else np.cumsum(np.asarray(T, dtype=np.float64).reshape(-1))
    h = []
    for _ in range(int(N)):
        myT = int(T) if cumT is None else multirnd(cumT, rng.random()) + 1
        hh = np.zeros(myT, dtype=np.int64)
        if myT > 0:
            hh[0] = multirnd(cumprior, rng.random())
        for t in range(1, myT):
            hh[t] = multirnd(cumtrans[hh[t - 1]], rng.random())
        h.append(hh)
    data = [np.zeros((len(hh), d)) for hh in h]
    for j in range(K):
        c = covs[j]
        L = np.linalg.cholesky(np.diag(c) if c.ndim == 1 else c)
        for n, hh in enumerate(h):
            ii = np.nonzero(hh == j)[0]
            data[n][ii] = rng.standard_normal((len(ii), d)) @ L.T + mean[j]
    return h, data


def vbhmm_prob_state(hmm: dict, stateseq):
    """vbhmm_prob_state.m: the probability of a hidden-state sequence (0-based
    indices), prior[s_0] * prod_t trans[s_{t-1}][s_t]; a list of sequences gives
    an array."""
    prior = np.asarray(hmm["prior"], dtype=np.float64).reshape(-1)
    trans = np.asarray(hmm["trans"], dtype=np.float64).reshape(len(prior), len(prior))
    single = not (isinstance(stateseq, (list, tuple)) and len(stateseq) > 0
                  and np.ndim(stateseq[0]) > 0)
    out = []
    for X in ([stateseq] if single else stateseq):
        X = np.asarray(X, dtype=np.int64).reshape(-1)
        pr = prior[X[0]]
        for t in range(1, len(X)):
            pr = pr * trans[X[t - 1], X[t]]
        out.append(pr)
    return float(out[0]) if single else np.array(out)
