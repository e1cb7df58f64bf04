"""Clustering scores of the reference's synthetic experiments
(Synthetic_experiment/evaluate_vbhem_jounarl.m:86-122, syn_evluate.m): the Rand
indices of src/compare_mtds/eva/valid_RandIndex.m and the purity of
src/compare_mtds/eva/Purity.m, restated for numpy label vectors (any integer
labels; the reference's are 1-based).

The rest of that evaluation:

  :func:`dunn_index`       compute_hmms_dist.m / compute_inter_Centhmms_dist.m and the
                           ``cpt_dist`` branches: every KL of the index in one fused
                           ``score.kld_jobs`` call on the GPU
  :func:`mixture_loglik`   the PPK log-likelihood of :27-57
  :func:`sc_aic`, :func:`sc_bic`   the 'scaic' / 'scbic' criteria of :237-296
  :func:`evaluate_run`     one iteration of evaluate_vbhem_jounarl.m for one method
  :func:`summarize`        its means and standard deviations over runs (:580-652)

Labels, groups and centre indices are 0-based.  A CCFD halo member (marked -1 in
``ccfd_result["halo"]``) enters RI and purity with the cluster label it has in ``cl``
(``result["label"]``), not with the halo mark: the reference scores ``CCFD_i.label``,
which myccfd.m fills from ``cl``."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def contingency(c1, c2) -> np.ndarray:
    """valid_RandIndex.m:44-55: counts of (c1 label, c2 label) pairs."""
    a = np.unique(np.asarray(c1), return_inverse=True)[1].ravel()
    b = np.unique(np.asarray(c2), return_inverse=True)[1].ravel()
    C = np.zeros((a.max() + 1 if a.size else 0, b.max() + 1 if b.size else 0))
    np.add.at(C, (a, b), 1.0)
    return C


def rand_index(c1, c2):
    """(RI, AR, MI, HI) of valid_RandIndex(c1, c2) (:18-42): the Rand index, the
    Hubert-Arabie adjusted Rand index, Mirkin's and Hubert's indices."""
    c1 = np.asarray(c1).ravel()
    c2 = np.asarray(c2).ravel()
    if c1.size != c2.size or c1.size < 2:
        raise ValueError("rand_index: two label vectors of the same length >= 2")
    C = contingency(c1, c2)
    n = C.sum()
    nis = (C.sum(axis=1) ** 2).sum()
    njs = (C.sum(axis=0) ** 2).sum()
    t1 = n * (n - 1) / 2.0
    t2 = (C ** 2).sum()
    t3 = 0.5 * (nis + njs)
    nc = (n * (n ** 2 + 1) - (n + 1) * nis - (n + 1) * njs + 2 * (nis * njs) / n) / (2 * (n - 1))
    A = t1 + t2 - t3
    D = -t2 + t3
    AR = 0.0 if t1 == nc else (A - nc) / (t1 - nc)
    return A / t1, AR, D / t1, (A - D) / t1


def purity(labels, clusters) -> float:
    """Purity.m:7-19: the fraction of items whose cluster's majority label is theirs."""
    labels = np.asarray(labels).ravel()
    clusters = np.asarray(clusters).ravel()
    if labels.size != clusters.size:
        raise ValueError("purity: label vectors of different lengths")
    overlap = 0
    for k in np.unique(clusters):
        _, cnt = np.unique(labels[clusters == k], return_counts=True)
        overlap += int(cnt.max())
    return overlap / labels.size


# ----------------------------------------------------------------------------
# the Dunn index
# ----------------------------------------------------------------------------
def dunn_index(centres, hmms, data_by_subject, groups, pooled: str = "members", centre_subjects=None,
               device="cuda") -> dict:
    """The Dunn index of a clustering of subject HMMs (higher is better):

      intra[j][i] = 0.5 (KL(c_j, h_i | cendata_j) + KL(h_i, c_j | data_i))   (compute_hmms_dist.m:57-62)
      inter[i][j] = 0.5 (KL(c_i, c_j | cendata_i) + KL(c_j, c_i | cendata_j)), i < j
                                                              (compute_inter_Centhmms_dist.m:42-53)
      DI = min(inter_vct) / max_j max(intra[j])

    with KL(a, b | data) = vbhmm_kld(a, b, data) (normalised by the lengths).  ``centres``:
    K centre HMM dicts (None: no centre); ``hmms``: the H subject HMMs; ``data_by_subject[i]``:
    subject i's trials; ``groups[j]``: the subjects of cluster j.  ``pooled="members"``:
    cendata_j is all members' trials in group order (the reference's 'vb', 'vh', 'dic');
    ``"centre"``: the trials of subject ``centre_subjects[j]`` ('sc' with ind_center, 'ccfd'
    with icl).  Clusters that are empty or have no centre are dropped first; one remaining
    centre gives DI = 0.0 (evaluate_vbhem_jounarl.m:324-325); a zero denominator follows
    IEEE division.  Centres and members go into one HmmSet, all trials into one
    SequenceBatch, and the whole index is one ``score.kld_jobs`` call.

    Returns ``intra`` (per kept cluster an array over its members), ``inter`` [K][K]
    (filled above the diagonal), ``inter_vct`` (in (i, j > i) order), ``DI`` and ``kept``
    (the indices of the clusters that stayed)."""
    from . import score
    from .vbhmm import SequenceBatch
    if pooled not in ("members", "centre"):
        raise ValueError("pooled must be 'members' or 'centre'")
    if len(centres) != len(groups):
        raise ValueError("dunn_index needs one group per centre")
    if pooled == "centre" and (centre_subjects is None or len(centre_subjects) != len(centres)):
        raise ValueError("pooled='centre' needs one centre subject per centre")
    H = len(hmms)
    if len(data_by_subject) != H:
        raise ValueError("data_by_subject needs one list of trials per subject HMM")
    grp = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
    kept = [j for j, g in enumerate(grp) if len(g) and centres[j] is not None]
    if not kept:
        raise ValueError("dunn_index: no cluster with members and a centre")
    K = len(kept)
    if K == 1:
        return dict(intra=[], inter=np.zeros((1, 1)), inter_vct=np.zeros(0), DI=0.0, kept=kept)
    if any(g.min() < 0 or g.max() >= H for g in (grp[j] for j in kept)):
        raise ValueError("dunn_index: a group member is not a subject")
    trials = [score._as_list(d) for d in data_by_subject]
    first = np.zeros(H + 1, dtype=np.int64)
    first[1:] = np.cumsum([len(t) for t in trials])
    hset = score.HmmSet([centres[j] for j in kept] + list(hmms), device)
    sb = SequenceBatch([s for t in trials for s in t], hset.dim, hset.device)
    cs = None if pooled == "members" else [int(centre_subjects[j]) for j in kept]
    if cs is not None and any(not 0 <= i < H for i in cs):
        raise ValueError("dunn_index: a centre subject is not a subject")
    lists, jobs = dunn_jobs([grp[j] for j in kept], first, cs)
    kl = score.kld_jobs(hset, sb, lists, jobs).cpu().numpy()
    return dict(dunn_reduce(kl, [grp[j] for j in kept]), kept=kept)


def dunn_jobs(groups, first, centre_subjects=None):
    """The (lists, jobs) of ``score.kld_jobs`` for the index of K clusters: HMM c < K is
    centre c, HMM K + i subject i; subject i's trials are the sequences
    first[i] .. first[i + 1] - 1 (list i).  cendata_c is the list of subject
    ``centre_subjects[c]``, or (None) a further list of all members' trials in group order.
    Jobs: per cluster and member the pair (c, K + i | cendata_c), (K + i, c | data_i), then
    per (a, b > a) the pair (a, b | cendata_a), (b, a | cendata_b)."""
    K, H = len(groups), len(first) - 1
    lists = [np.arange(first[i], first[i + 1]) for i in range(H)]
    cen = []
    for c, g in enumerate(groups):
        if centre_subjects is None:
            lists.append(np.concatenate([lists[i] for i in g]))
            cen.append(len(lists) - 1)
        else:
            cen.append(int(centre_subjects[c]))
    jobs = []
    for c, g in enumerate(groups):
        for i in g:
            jobs.append((c, K + int(i), cen[c]))
            jobs.append((K + int(i), c, int(i)))
    for a in range(K):
        for b in range(a + 1, K):
            jobs.append((a, b, cen[a]))
            jobs.append((b, a, cen[b]))
    return lists, jobs


def dunn_reduce(kl, groups) -> dict:
    """intra, inter, inter_vct and DI from the values of :func:`dunn_jobs`' jobs."""
    K = len(groups)
    kl = np.asarray(kl, dtype=np.float64)
    half = 0.5 * (kl[0::2] + kl[1::2])
    intra, at = [], 0
    for g in groups:
        intra.append(half[at:at + len(g)].copy())
        at += len(g)
    inter_vct = half[at:].copy()
    inter = np.zeros((K, K))
    inter[np.triu_indices(K, 1)] = inter_vct
    with np.errstate(divide="ignore", invalid="ignore"):
        DI = float(np.float64(inter_vct.min()) / np.float64(max(m.max() for m in intra)))
    return dict(intra=intra, inter=inter, inter_vct=inter_vct, DI=DI)


# ----------------------------------------------------------------------------
# the PPK criteria
# ----------------------------------------------------------------------------
def mixture_loglik(hmms, weight, data_by_subject, device="cuda") -> float:
    """evaluate_vbhem_jounarl.m:44-52: ``sum_n logsumexp_k(log w_k + ll_k(n))`` over all
    trials of all subjects, ll normalised by the length (vbhmm_ll's default 'n').  An HMM
    that carries the counts pruning needs (``N`` and ``varpar``) first loses its states
    with N < 1e-3 (vbhmm_remove_empty(h, 0, 1e-3)); a plain point HMM is scored as it is.
    A centre that is None (an empty PPK cluster) is left out with its weight."""
    from scipy.special import logsumexp
    from . import score
    w = np.asarray(weight, dtype=np.float64).reshape(-1)
    if len(hmms) != w.size:
        raise ValueError("mixture_loglik needs one weight per HMM")
    use = [k for k, h in enumerate(hmms) if h is not None]
    hs = []
    for k in use:
        h = hmms[k]
        if "N" in h and "varpar" in h:
            from .vbhmm_em import vbhmm_remove_empty
            h = vbhmm_remove_empty(h if "gamma" in h else dict(h, gamma=[]), 1e-3)
        hs.append(h)
    seqs = [s for d in data_by_subject for s in score._as_list(d)]
    ll = score.ll_matrix(score.HmmSet(hs, device), seqs, True).cpu().numpy()      # [K][N_total]
    with np.errstate(divide="ignore"):
        return float(np.sum(logsumexp(np.log(w[use])[:, None] + ll, axis=0)))


def sc_num_pars(K: int, S: int, dim: int) -> int:
    """evaluate_vbhem_jounarl.m:251 / :283."""
    return (K - 1) + K * ((S - 1) + S * (S - 1) + S * 2 * dim)


def _sc_criterion(ppk_ll, K, S, dim, T, div_T, weight):
    Ks, Ss = [int(k) for k in np.atleast_1d(K)], [int(s) for s in np.atleast_1d(S)]
    LL = np.asarray(ppk_ll, dtype=np.float64).reshape(len(Ks), len(Ss))
    out = np.zeros((len(Ks), len(Ss)))
    for k, kk in enumerate(Ks):
        for s, ss in enumerate(Ss):
            out[k, s] = -2 * (LL[k, s] / T if div_T else LL[k, s]) + weight * sc_num_pars(kk, ss, dim)
    return out


def sc_aic(ppk_ll, K, S, dim: int, T: float, div_T: int = 0) -> np.ndarray:
    """'scaic' (:237-264), [len_K][len_S]: -2 PPK_LL [/ T] + 2 Num_pars.  ``T``: the mean
    length of the subjects' first trials (:244)."""
    return _sc_criterion(ppk_ll, K, S, dim, T, div_T, 2.0)


def sc_bic(ppk_ll, K, S, dim: int, n_bic: float, T: float, div_T: int = 0) -> np.ndarray:
    """'scbic' (:266-296), [len_K][len_S]: -2 PPK_LL [/ T] + log(n_bic) Num_pars.
    ``n_bic``: the number of observations of all trials (:272-274)."""
    return _sc_criterion(ppk_ll, K, S, dim, T, div_T, float(np.log(n_bic)))


# ----------------------------------------------------------------------------
# one iteration of evaluate_vbhem_jounarl.m, and the summary over runs
# ----------------------------------------------------------------------------
METHODS = ("vb", "vhem", "ccfd", "dic", "vhbic", "vhaic", "scaic", "scbic")


def fix_negative_criterion(crit) -> np.ndarray:
    """:437-448 ('vhaic' / 'vhbic'): where the grid holds exactly one negative entry, that
    entry becomes +inf; any other grid is left as it is."""
    crit = np.array(crit, dtype=np.float64)
    if int((crit < 0).sum()) == 1:
        crit[crit < 0] = np.inf
    return crit


def _k_flags(K_select, num_hmm):
    return dict(is_K_right=float(K_select == num_hmm), is_K_big=float(K_select > num_hmm),
                is_K_less=float(K_select < num_hmm))


def _s_flags(S_select, num_sta):
    S_select = np.asarray(S_select)
    n = S_select.size
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(is_S_right=float(np.float64((S_select == num_sta).sum()) / n),
                    is_S_big=float(np.float64((S_select > num_sta).sum()) / n),
                    is_S_less=float(np.float64((S_select < num_sta).sum()) / n))


def _vhem_cell(cell, true_label, num_hmm, num_sta, with_S, dist):
    """One vhem_cluster output: (:363-405), also what 'vhaic' / 'vhbic' read (:471-492)."""
    size = np.asarray(cell["group_size"])
    nonempty = np.flatnonzero(size != 0)
    out = dict(RI=rand_index(true_label, cell["label"])[0], purity=purity(true_label, cell["label"]),
               K_select=int(nonempty.size))
    out.update(_k_flags(out["K_select"], num_hmm))
    if with_S:
        out["S_select"] = np.array([int((np.asarray(cell["hmms"][j]["stats"]["emit_vcounts"]) > 1e-3).sum())
                                    for j in nonempty])
        out.update(_s_flags(out["S_select"], num_sta))
    if dist is not None:
        out["DI"] = dist([cell["hmms"][j] for j in nonempty], [cell["groups"][j] for j in nonempty], "members", None)
    return out


def evaluate_run(method: str, result, true_label, num_hmm: int, num_sta: int, criterion=None, S=None,
                 hmms=None, data=None, cpt_dist: bool = False, device="cuda") -> dict:
    """One iteration of evaluate_vbhem_jounarl.m for one method.  ``result``:

      'vb'     a fit after ``dic.vbh3m_remove_empty`` (its dict, or the pair it returns)
      'vhem'   a [k][s] grid of ``vhem.vhem_cluster`` outputs; every output is the mean
               over the grid (:413-431), K_select the grid of counts
      'ccfd'   ``ccfd.myccfd``'s dict
      'dic', 'vhbic', 'vhaic', 'scaic', 'scbic'
               ``criterion`` [len_K][len_S] and the [k][s] grid of results it was computed
               from ('dic': ``dic.fit_to_h3m`` dicts, pruned here as :519-521 does; 'vh*':
               vhem_cluster outputs; 'sc*': ``ppk.ppk_sc`` outputs); the cell at the
               criterion's minimum is scored.  For 'vhaic' / 'vhbic' a negative entry is
               first replaced by +inf where the grid holds exactly one (:437-448).

    Returns RI, purity, K_select, is_K_right / is_K_big / is_K_less; S_select and the
    is_S_* fractions for 'vb' always and for the grid methods when the grid has more than
    one S (``S``, or the grid's second extent), never for 'ccfd'; ``DI`` when ``cpt_dist``
    and ``hmms`` (the subject HMMs) and ``data`` (their trials) are given; the selected
    cell as ``select`` = (k, s) for the criterion methods.  A CCFD halo member counts with
    its cluster label from ``cl``."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}")
    true_label = np.asarray(true_label).ravel()
    dist = None
    if cpt_dist:
        if hmms is None or data is None:
            raise ValueError("cpt_dist needs the subject HMMs and their data")

        def dist(centres, groups, pooled, centre_subjects):
            return dunn_index(centres, hmms, data, groups, pooled, centre_subjects, device)["DI"]

    def vb_like(model):
        out = dict(RI=rand_index(true_label, model["label"])[0], purity=purity(true_label, model["label"]),
                   K_select=len(np.asarray(model["omega"]).reshape(-1)),
                   S_select=np.array([len(np.asarray(h["prior"]).reshape(-1)) for h in model["hmm"]]))
        out.update(_k_flags(out["K_select"], num_hmm))
        if dist is not None:
            out["DI"] = dist(list(model["hmm"]), model["groups"], "members", None)
        return out

    if method == "vb":
        out = vb_like(result[0] if isinstance(result, tuple) else result)
        out.update(_s_flags(out["S_select"], num_sta))
        return out
    if method == "ccfd":
        icl = np.asarray(result["ccfd_result"]["icl"]).reshape(-1)
        out = dict(RI=rand_index(true_label, result["label"])[0], purity=purity(true_label, result["label"]),
                   K_select=int(icl.size))
        out.update(_k_flags(out["K_select"], num_hmm))
        if dist is not None:
            out["DI"] = dist(list(result["hmms"]), result["groups"], "centre", icl)
        return out

    len_K, len_S = len(result), len(result[0])
    if S is not None:
        len_S = len(np.atleast_1d(S))
    with_S = len_S > 1
    if method == "vhem":
        cells = [_vhem_cell(c, true_label, num_hmm, num_sta, with_S, dist) for row in result for c in row]
        keys = ["RI", "purity", "is_K_right", "is_K_big", "is_K_less"] + (["DI"] if dist is not None else [])
        keys += ["is_S_right", "is_S_big", "is_S_less"] if with_S else []
        out = {k: float(np.mean([c[k] for c in cells])) for k in keys}
        out["K_select"] = np.array([c["K_select"] for c in cells]).reshape(len_K, -1)
        if with_S:
            out["S_select"] = [[c["S_select"] for c in cells[r * len(result[0]):(r + 1) * len(result[0])]]
                               for r in range(len_K)]
        return out

    if criterion is None:
        raise ValueError(f"method '{method}' needs its criterion grid")
    crit = np.array(criterion, dtype=np.float64)
    if crit.shape != (len_K, len(result[0])):
        raise ValueError("the criterion grid and the grid of results differ in shape")
    if method in ("vhaic", "vhbic"):
        crit = fix_negative_criterion(crit)
    k, s = (int(v) for v in np.unravel_index(int(np.argmin(crit)), crit.shape))
    cell = result[k][s]
    if method in ("vhaic", "vhbic"):
        out = _vhem_cell(cell, true_label, num_hmm, num_sta, True, dist)
    elif method in ("scaic", "scbic"):
        have = [j for j, h in enumerate(cell["hmms"]) if h is not None]
        out = dict(RI=rand_index(true_label, cell["label"])[0], purity=purity(true_label, cell["label"]),
                   K_select=len(np.asarray(cell["group_size"]).reshape(-1)),
                   S_select=np.array([len(np.asarray(cell["hmms"][j]["prior"]).reshape(-1)) for j in have]))
        out.update(_k_flags(out["K_select"], num_hmm))
        if dist is not None:
            out["DI"] = dist(list(cell["hmms"]), cell["group"], "centre", cell["ind_center"])
    else:
        from .dic import vbh3m_remove_empty
        out = vb_like(vbh3m_remove_empty(cell)[0])
    if with_S:
        out.update(_s_flags(out["S_select"], num_sta))
    else:
        for key in ("is_S_right", "is_S_big", "is_S_less"):
            out.pop(key, None)
    out["select"] = (k, s)
    out["criterion"] = crit
    return out


SUMMARY_KEYS = ("RI", "purity", "DI", "is_K_right", "is_K_big", "is_K_less", "is_S_right", "is_S_big", "is_S_less")


def summarize(runs: Sequence[dict]) -> dict:
    """:580-652 over the dicts of :func:`evaluate_run`: per output present in every run the
    vector over the runs, ``mean_<name>`` and ``std_<name>`` (N - 1 in the divisor, as
    MATLAB's std; 0 for a single run), and ``K_is`` / ``S_is``, the runs' selections."""
    runs = list(runs)
    if not runs:
        raise ValueError("summarize needs at least one run")
    out = {}
    for key in SUMMARY_KEYS:
        if all(key in r for r in runs):
            v = np.array([float(r[key]) for r in runs])
            out[key] = v
            out["mean_" + key] = float(v.mean())
            out["std_" + key] = float(v.std(ddof=1)) if v.size > 1 else 0.0
    out["K_is"] = [r["K_select"] for r in runs]
    if all("S_select" in r for r in runs):
        out["S_is"] = [r["S_select"] for r in runs]
    return out
