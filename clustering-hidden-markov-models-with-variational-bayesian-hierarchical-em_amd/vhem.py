"""VHEM clustering of HMMs (src/compare_mtds/hem: vhem_cluster.m and vhem_h3m/).

The classic emhmm clustering call: point-estimate HMMs are clustered into K group
HMMs of S states by the variational hierarchical EM of Coviello et al.  One EM
iteration is one launch of the fused VHEM E-step (``EStepEngine.fused_vhem``:
recursions, responsibilities, weights and the gated statistic sums on the device);
everything here is the O(K S d^2) host math around it (with hemopt['em_engine'] =
'device' the EM loop of a chunk of trials runs on the GPU instead, vhem_em_run_trials,
and only the trials that need a degenerate fix come back to this host loop):

* :func:`hmms_to_h3m` / :func:`h3m_to_hmms` -- hmms_to_h3m.m, h3m_to_hmms.m
* :func:`hem_mstep` -- hem_mstep_component.m:123-166 from the packed statistics
* :func:`hem_fix_degenerate_component` / :func:`hem_fix_degenerate_hmm`
* :func:`hem_h3m_c_step` / :func:`hem_h3m_c_trials` -- hem_h3m_c_step.m, hem_h3m_c.m
* :func:`initialize_hem_h3m_c` -- initialize_hem_h3m_c.m ('base', 'baseem', 'gmmNew',
  'gmmNew2')
* :func:`vhem_cluster` -- vhem_cluster.m

A reduced mixture (h3m_r) is a dict: omega [K], prior [K,S], A [K,S,S], centres
[K,S,d], covars [K,S,d,d] (full) | [K,S,d] (diag), LogL, and after an M-step
emit_vcounts [K,S].  Indices are 0-based.  Every ``rand`` of the reference comes from
a numpy Generator (trial t: seed + t), so parity of the random draws is unpinned.
"""
from __future__ import annotations

import warnings
from typing import List, Optional

import numpy as np
import torch

from . import host
from .cluster import form_groups, unique_ll
from .h3m import (COV_DIAG, COV_FULL, BaseSet, gmm_mix_hier_em, hmms_to_h3m_hem, make_a_prior,
                  make_gmm_weights)

INITMODES = ("base", "baseem", "gmmNew", "gmmNew2")
MAX_BATCH_CLUSTERS = 256  # clusters per batched-trials launch (as cluster.vbhem_h3m_c)


# ----------------------------------------------------------------------------
# options (vhem_cluster.m:107-187)
# ----------------------------------------------------------------------------
def default_hemopt(K: int, S: int, **over) -> dict:
    """hemopt with the defaults of vhem_cluster.m:107-187; ``seed`` is required."""
    opt = dict(K=int(K), N=int(S), verbose=0, remove_empty=1, trials=100, reg_cov=0.001,
               termmode="L", termvalue=1e-5, max_iter=100, min_iter=1, sortclusters="f",
               initmode="auto", tau=10, seed=None, Nv=100, inf_norm="nt", smooth=1.0,
               keep_suboptimal_hmms=0, computeStats=0, covar_type="full", M=1,
               em_engine="host")
    initopt = dict(iter=30, trials=4, mode="")
    initopt.update(over.pop("initopt", {}) or {})
    unknown = set(over) - set(opt)
    if unknown:
        raise ValueError(f"unknown hemopt fields: {sorted(unknown)}")
    opt.update(over)
    if not initopt["mode"]:
        initopt["mode"] = {"baseem": "u", "gmmNew": "r0", "gmmNew2": "u0"}.get(opt["initmode"], "")
    opt["initopt"] = initopt
    if opt["seed"] is None:
        raise ValueError("hemopt['seed'] needs to be set to make reproducible results")
    if opt["computeStats"]:
        raise ValueError("computeStats (mu2 / MANOVA) is not supported")
    if opt["M"] != 1:
        raise ValueError("GMM emissions with M > 1 are not supported")
    if opt["termmode"] != "L":
        raise ValueError("termmode must be 'L'")
    if opt["covar_type"] not in ("full", "diag"):
        raise ValueError("covar_type must be 'full' or 'diag'")
    if opt["initmode"] != "auto" and opt["initmode"] not in INITMODES:
        raise ValueError(f"initmode {opt['initmode']!r}: 'auto' or one of {INITMODES}")
    if opt["em_engine"] not in ("host", "device"):
        raise ValueError(f"em_engine {opt['em_engine']!r}: 'host' or 'device'")
    inf_norm_value(opt["inf_norm"], 1, 1, 1)
    return opt


def inf_norm_value(mode: str, T: int, Nv: float, Kb: int) -> float:
    """hem_h3m_c_step.m:110-119."""
    if mode == "":
        return 1.0
    if mode == "n":
        return float(Nv) / Kb
    if mode in ("tn", "nt"):
        return float(T) * float(Nv) / Kb
    if mode == "t":
        return float(T)
    raise ValueError(f"unknown inf_norm {mode!r}")


# ----------------------------------------------------------------------------
# conversions
# ----------------------------------------------------------------------------
def hmms_to_h3m(hmms: List[Optional[dict]], covmode="full") -> BaseSet:
    """hmms_to_h3m.m: point prior / trans / pdf{}.mean, cov; an empty entry (None)
    becomes a one-state dummy with omega = 0; omega is normalised."""
    cm = {"full": COV_FULL, "diag": COV_DIAG}.get(covmode, covmode)
    return hmms_to_h3m_hem(hmms, cm, use_post=False)


def copy_h3m(h: dict) -> dict:
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in h.items()}


def h3m_to_hmms(h3m: dict, covmode: int) -> dict:
    """h3m_to_hmms.m: the group HMMs, label = argmax_j Z (0-based), groups, group_size,
    Z, LogL, LogLs, L_elbo1 and per-HMM stats.emit_vcounts."""
    K = len(h3m["omega"])
    ns = h3m.get("nstates")
    hmms = []
    for j in range(K):
        S = int(ns[j]) if ns is not None else h3m["prior"].shape[1]
        cov = h3m["covars"][j, :S]
        hm = dict(prior=np.array(h3m["prior"][j, :S]), trans=np.array(h3m["A"][j, :S, :S]),
                  pdf=[dict(mean=np.array(h3m["centres"][j, s]),
                            cov=np.diag(cov[s]) if covmode == COV_DIAG else np.array(cov[s]))
                       for s in range(S)])
        if "emit_vcounts" in h3m:
            hm["stats"] = dict(emit_vcounts=np.array(h3m["emit_vcounts"][j]))
        hmms.append(hm)
    Z = np.asarray(h3m["Z"])
    label = np.argmax(Z, axis=1)
    groups, group_size = form_groups(label, K)
    out = dict(Z=Z, LogLs=h3m["LogLs"], LogL=h3m["LogL"], label=label, groups=groups,
               group_size=group_size, hmms=hmms, omega=np.array(h3m["omega"]))
    if "L_elbo1" in h3m:
        out["L_elbo1"] = h3m["L_elbo1"]
    return out


# ----------------------------------------------------------------------------
# M-step and the degenerate fixes
# ----------------------------------------------------------------------------
def hem_mstep(st: dict, Kb: int, tau: int, reg_cov: float, covmode: int) -> dict:
    """hem_mstep_component.m:123-166 for every cluster, and omega_new = Nj / Kb
    (hem_h3m_c_step.m:430).  ``st`` = host.unpack_stats of the VHEM fused E-step:
    N1 = new_prior, M = new_A, Nr = new_Gweight, Y = new_Gmu, SC = new_GMu."""
    new_prior, new_A = st["N1"], st["M"]
    K, S = new_prior.shape
    d = st["Y"].shape[-1]
    if S == 1:                                     # :124 (xi = 0 for one state)
        new_A = np.full((K, 1, 1), 1e-12)
    if tau == 1:                                   # :129
        new_A = np.repeat(1e-12 * np.eye(S)[None], K, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        prior = new_prior / new_prior.sum(1, keepdims=True)
        A = new_A / new_A.sum(2, keepdims=True)
        vcounts = new_A.sum(1) + new_prior         # :138
        w = st["Nr"]
        cen = st["Y"] / w[..., None]
        if covmode == COV_DIAG:
            Sigma = st["SC"] - 2 * (st["Y"] * cen) + (cen ** 2) * w[..., None]
            cov = Sigma / w[..., None] + reg_cov
        else:
            tmp = st["Y"][..., :, None] * cen[..., None, :]
            tmp2 = w[..., None, None] * (cen[..., :, None] * cen[..., None, :])
            Sigma = st["SC"] - tmp - np.swapaxes(tmp, -1, -2) + tmp2
            cov = Sigma / w[..., None, None] + reg_cov * np.eye(d)
    return dict(omega=st["Nj"] / Kb, prior=prior, A=A, centres=cen, covars=cov,
                emit_vcounts=vcounts)


def hem_fix_degenerate_component(h: dict, iz: int, N: int, draw) -> None:
    """hem_fix_degenerate_component.m (in place): cluster iz (omega = 0) becomes a
    perturbed copy of the heaviest one; N = the first base HMM's state count;
    ``draw(shape)`` = rand(shape)."""
    hi = int(np.argmax(h["omega"]))
    h["omega"][[iz, hi]] = h["omega"][hi] / 2
    h["omega"] = h["omega"] / h["omega"].sum()
    for k in ("centres", "covars", "emit_vcounts"):
        if k in h:
            h[k][iz] = h[k][hi]
    prior = h["prior"][hi] + (0.1 / N) * draw(h["prior"][hi].shape)
    A0 = h["A"][hi]
    A = (0.1 / N) * draw(A0.shape)
    A[A0 == 0] = 0
    h["prior"][iz] = prior / prior.sum()
    h["A"][iz] = A / A.sum(1, keepdims=True)


def hem_fix_degenerate_hmm(h: dict, j: int, iz: int, draw) -> None:
    """hem_fix_degenerate_hmm.m (in place): state iz of cluster j (no counts) splits
    the state with the most counts."""
    hi = int(np.argmax(h["emit_vcounts"][j]))
    prior, A = h["prior"][j], h["A"][j]
    prior[[iz, hi]] = prior[hi] / 2
    h["prior"][j] = prior / prior.sum()
    A[iz, :] = A[hi, :]
    half = A[:, hi] / 2
    A[:, iz] = half
    A[:, hi] = half
    h["covars"][j, iz] = h["covars"][j, hi]
    c = np.array(h["centres"][j, hi])
    h["centres"][j, iz] = c + (0.01 * draw(c.shape)) * c


def _apply_fixes(h: dict, N: int, draw) -> None:
    """hem_h3m_c_step.m:461-478."""
    for iz in np.flatnonzero(h["omega"] == 0):
        hem_fix_degenerate_component(h, int(iz), N, draw)
    for j in range(len(h["omega"])):
        for iz in np.flatnonzero(h["emit_vcounts"][j] == 0):
            hem_fix_degenerate_hmm(h, j, int(iz), draw)


# ----------------------------------------------------------------------------
# EM (hem_h3m_c_step.m), R trials in lockstep
# ----------------------------------------------------------------------------
def _stack(hs: List[dict], covmode: int) -> dict:
    red = {k: np.concatenate([h[k] for h in hs], axis=0) for k in ("A", "prior", "centres", "covars")}
    return host.vhem_cluster_constants(red, covmode)


def device_em_supported(base: BaseSet, K: int, S: int, R: int, opt: dict) -> bool:
    """Whether a chunk of R trials of K clusters lies inside the shapes of the device EM
    engine (vhem_em_run_trials): those of the batched E-step with d <= 16, and a
    ``min_iter`` that lets every trial end within max_iter + 2 E-steps."""
    max_iter, min_iter = int(opt["max_iter"]), int(opt.get("min_iter", 0))
    return (1 <= S <= 16 and base.SB <= S and 1 <= base.d <= 16 and R >= 1 and R * K <= 256
            and max_iter >= 0 and 0 <= min_iter <= max_iter + 1)


def _hem_h3m_c_trials_device(h3ms: List[dict], engine, opt: dict, rngs) -> List[dict]:
    """hem_h3m_c_trials with the loop on the device (vhem_em_run_trials); the trials it
    flags are rerun by the host engine."""
    import ctypes

    from . import _capi
    from .estep import EStepEngine
    if not isinstance(engine, EStepEngine):
        raise ValueError("em_engine='device' needs a device EStepEngine")
    R = len(h3ms)
    base = engine.base
    covmode, Kb, d = base.covmode, base.N, base.d
    K, S = h3ms[0]["prior"].shape
    if engine.K != R * K:
        raise ValueError("the trials must share one shape, K = engine.K / trials")
    T, Nv = int(opt["tau"]), opt["Nv"]
    reg = float(opt.get("reg_cov", 0.0))
    inf_norm = inf_norm_value(opt["inf_norm"], T, Nv, Kb)
    max_iter = int(opt["max_iter"])
    omegaB = base.omega.to(torch.float64).contiguous()
    Ni = ((float(Nv) * omegaB) * float(Kb)).contiguous()              # :61
    add = reg * np.eye(d) if covmode == COV_FULL else reg             # :98-108
    arr = {k: np.ascontiguousarray(np.stack([np.asarray(h[k], dtype=np.float64) for h in h3ms]))
           for k in ("omega", "prior", "A", "centres")}
    arr["covars"] = np.ascontiguousarray(
        np.stack([np.asarray(h["covars"], dtype=np.float64) + add for h in h3ms]))
    arr["emit_vcounts"] = np.zeros((R, K, S))
    want = dict(omega=(R, K), prior=(R, K, S), A=(R, K, S, S), centres=(R, K, S, d),
                covars=(R, K, S, d, d) if covmode == COV_FULL else (R, K, S, d))
    for k, shp in want.items():
        if arr[k].shape != shp:
            raise ValueError(f"the trials' {k} must have shape {shp[1:]}")
    mix = _capi.VhemMixTrialsT(K, S, d, covmode, *(arr[k].ctypes.data for k in (
        "omega", "prior", "A", "centres", "covars", "emit_vcounts")))
    copt = _capi.VhemEmOptT(inf_norm, float(opt["smooth"]), reg, float(opt["termvalue"]), T,
                            max_iter, int(opt.get("min_iter", 0)))
    lib = _capi.lib()
    nb = int(lib.vhem_em_trials_workspace_bytes(ctypes.byref(engine._bt), K, S, R, T))
    if nb == 0:
        raise _capi.VbhemError(
            f"vhem_em_trials_workspace_bytes: unsupported shape (R={R}, K={K}, S={S}, d={d}, "
            f"Sb={base.SB}): needs R*K <= 256, Sb <= S <= 16, d <= 16")
    ws = getattr(engine, "_em_ws", None)
    if ws is None or ws.numel() < nb:
        ws = engine._em_ws = torch.empty((nb,), dtype=torch.uint8, device=engine.device)
    SL = host.stats_len(K, S, d, covmode)
    LogLs = np.zeros((R, max_iter + 2))
    num_iter, fb, fb_iter = (np.zeros(R, dtype=np.int32) for _ in range(3))
    LogL, stats = np.zeros(R), np.zeros((R, SL))
    rc = lib.vhem_em_run_trials(ctypes.byref(engine._bt), _capi.ptr(Ni), _capi.ptr(omegaB), R, T,
                                ctypes.byref(copt), ctypes.byref(mix), LogLs.ctypes.data,
                                num_iter.ctypes.data, LogL.ctypes.data, fb.ctypes.data,
                                fb_iter.ctypes.data, stats.ctypes.data, _capi.ptr(engine.hatZ),
                                _capi.ptr(engine.LL), _capi.ptr(ws), ws.numel(), engine._stream())
    _capi.check(rc, "vhem_em_run_trials")
    flagged = [r for r in range(R) if fb[r]]
    Z = engine.hatZ.cpu().numpy()
    Lel = engine.LL.cpu().numpy()
    hs: List[Optional[dict]] = [None] * R
    for r in range(R):
        if fb[r]:
            continue
        n, cols = int(num_iter[r]), slice(r * K, (r + 1) * K)
        hs[r] = dict(omega=arr["omega"][r].copy(), prior=arr["prior"][r].copy(), A=arr["A"][r].copy(),
                     centres=arr["centres"][r].copy(), covars=arr["covars"][r].copy(),
                     emit_vcounts=arr["emit_vcounts"][r].copy(), LogL=float(LogL[r]),
                     LogLs=[float(x) for x in LogLs[r, :n + 1]], Z=Z[:, cols].copy(),
                     L_elbo1=Lel[:, cols] / inf_norm, num_iter=n)
    if flagged:
        # the degenerate fixes draw from the trial's own Generator: the unchanged host
        # loop, from the initial mixtures, on a fresh engine of that many trials
        eng = EStepEngine(base, len(flagged) * K, S, T, device=engine.device, trials=len(flagged))
        redo = hem_h3m_c_trials([h3ms[r] for r in flagged], eng, opt, [rngs[r] for r in flagged])
        for r, h in zip(flagged, redo):
            hs[r] = h
    for h in hs:
        h["fallback_trials"] = list(flagged)
    return hs


def hem_h3m_c_trials(h3ms: List[dict], engine, opt: dict, rngs=None,
                     em_engine: str = "host") -> List[dict]:
    """hem_h3m_c_step.m for R initialisations at once: one batched fused E-step per
    iteration (vhem_estep_fused_trials); a trial that has stopped keeps its final
    state while its clusters ride along (as em.vbhem_h3m_c_trials).  ``rngs``: one
    numpy Generator per trial for the degenerate fixes' rand.  Returns the R final
    mixtures with Z, LogL, LogLs, L_elbo1, num_iter.

    em_engine: ``"host"`` (the default) runs the stopping rule, the M-step and the next
    E-step constants of every trial in numpy between two launches.  ``"device"`` keeps
    the loop on the GPU (vhem_em_run_trials: a device :class:`EStepEngine`, R K <= 256,
    Sb <= S <= 16, d <= 16, min_iter <= max_iter + 1; :func:`device_em_supported`).  The
    device draws no random number: a trial that needs a degenerate fix, or turns
    non-finite, is frozen there and flagged, and is then rerun by the host loop from its
    initial mixture with its own untouched Generator, so every trial's result is the
    host engine's.  Every dict returned by the device engine carries
    ``fallback_trials``: the indices (into ``h3ms``) of the trials that were rerun."""
    if em_engine not in ("host", "device"):
        raise ValueError(f"em_engine {em_engine!r}: 'host' or 'device'")
    R = len(h3ms)
    if engine.trials != R:
        raise ValueError("engine.trials must equal len(h3ms)")
    if em_engine == "device":
        rngs = rngs if rngs is not None else [np.random.default_rng(0) for _ in range(R)]
        return _hem_h3m_c_trials_device(h3ms, engine, opt, rngs)
    base = engine.base
    covmode = base.covmode
    Kb, d = base.N, base.d
    K, S = h3ms[0]["prior"].shape
    T, Nv = int(opt["tau"]), opt["Nv"]
    reg = float(opt.get("reg_cov", 0.0))
    inf_norm = inf_norm_value(opt["inf_norm"], T, Nv, Kb)
    smooth = float(opt["smooth"])
    omegaB = base.omega.to(torch.float64)
    Ni = (float(Nv) * omegaB) * float(Kb)          # :61
    Nb1 = int(base.nstates[0])
    SL = host.stats_len(K, S, d, covmode)
    rngs = rngs if rngs is not None else [np.random.default_rng(0) for _ in range(R)]
    hs = []
    for h in h3ms:                                  # :98-108
        h = copy_h3m(h)
        h["covars"] = h["covars"] + (reg * np.eye(d) if covmode == COV_FULL else reg)
        h["LogLs"] = []
        h.setdefault("LogL", -np.inf)
        hs.append(h)
    num_iter = [0] * R
    done = [False] * R
    while not all(done):
        engine.set_clusters(_stack(hs, covmode))
        with np.errstate(divide="ignore"):
            engine.set_log_omega(np.concatenate([np.log(h["omega"]) for h in hs]))
        vec = engine.fused_vhem(Ni, omegaB, inf_norm, smooth)
        vec = vec.cpu().numpy() if isinstance(vec, torch.Tensor) else np.asarray(vec)
        for r in range(R):
            if done[r]:
                continue
            h = hs[r]
            st = host.unpack_stats(vec[r * SL:(r + 1) * SL], K, S, d, covmode)
            new_LL = st["Lt1"]                      # LogL = sum_i LSE (:308)
            old_LL = h["LogL"]
            h["LogL"] = new_LL
            h["LogLs"].append(new_LL)
            with np.errstate(invalid="ignore", divide="ignore"):
                change = (new_LL - old_LL) / abs(old_LL) if num_iter[r] > 1 else np.inf
            if change < 0:
                warnings.warn("The change in log likelihood is negative!!!")
            stop = bool(change < opt["termvalue"]) or num_iter[r] > opt["max_iter"]
            if stop and num_iter[r] >= opt.get("min_iter", 0):
                done[r] = True
                cols = slice(r * K, (r + 1) * K)
                h["Z"] = engine.hatZ[:, cols].cpu().numpy().copy()
                h["L_elbo1"] = engine.LL[:, cols].cpu().numpy() / inf_norm
                h["num_iter"] = num_iter[r]
                continue
            num_iter[r] += 1
            new = hem_mstep(st, Kb, T, reg, covmode)
            new["LogL"], new["LogLs"] = h["LogL"], h["LogLs"]
            _apply_fixes(new, Nb1, rngs[r].random)
            hs[r] = new
    return hs


def hem_h3m_c_step(h3m_r: dict, engine, opt: dict, rng=None) -> dict:
    """hem_h3m_c_step.m for one initialisation."""
    return hem_h3m_c_trials([h3m_r], engine, opt, None if rng is None else [rng])[0]


# ----------------------------------------------------------------------------
# initialisations (initialize_hem_h3m_c.m)
# ----------------------------------------------------------------------------
def _base_states(bn: dict):
    ns = bn["nstates"]
    idx = [(i, s) for i in range(len(ns)) for s in range(int(ns[i]))]
    return idx, np.stack([bn["centres"][i, s] for i, s in idx]), np.stack([bn["covars"][i, s] for i, s in idx])


def initialize_hem_h3m_c(base: BaseSet, opt: dict, rng: np.random.Generator) -> dict:
    """initialize_hem_h3m_c.m for opt['initmode'] in 'base' (:142-152), 'baseem'
    (:111-139), 'gmmNew' / 'gmmNew2' (:276-493)."""
    bn = base.numpy()
    Kb, d, covmode = base.N, base.d, base.covmode
    Kr, N = int(opt["K"]), int(opt["N"])
    mode = opt["initmode"]
    iom = opt["initopt"]["mode"]
    full = covmode == COV_FULL
    cshape = (Kr, N, d, d) if full else (Kr, N, d)
    prior = np.zeros((Kr, N))
    A = np.zeros((Kr, N, N))
    cen = np.zeros((Kr, N, d))
    cov = np.zeros(cshape)
    if mode == "base":
        idx = rng.permutation(Kb)[:Kr]
        if np.any(bn["nstates"][idx] != N) or base.SB != N:
            raise ValueError("initmode 'base' needs base HMMs of S states")
        prior, A, cen, cov = (np.array(bn[k][idx]) for k in ("prior", "A", "centres", "covars"))
        omega = np.full(Kr, 1.0 / Kr)
    elif mode == "baseem":
        if not np.any(bn["omega"] != 0):
            raise ValueError("every base HMM has weight 0")
        for j in range(Kr):
            n = 0
            while n < N:
                rb = int(rng.integers(0, Kb))
                if bn["omega"][rb] == 0:            # v0.74: skip HMMs with weight 0
                    continue
                rg = int(rng.integers(0, int(bn["nstates"][rb])))
                cen[j, n], cov[j, n] = bn["centres"][rb, rg], bn["covars"][rb, rg]
                n += 1
            prior[j], A[j] = make_a_prior(N, iom, rng)
        omega = np.full(Kr, 1.0 / Kr)
    elif mode in ("gmmNew", "gmmNew2"):
        idx, pc, pv = _base_states(bn)
        # (:327 the base states' weights feed gmms.alpha only; trainMix has equal priors)
        for i in range(Kb):
            n = int(bn["nstates"][i])
            make_gmm_weights(bn["prior"][i, :n], bn["A"][i, :n, :n], iom)
        if mode == "gmmNew2":
            tmpK = N * Kr
            use = rng.permutation(tmpK).reshape((N, Kr)).T      # reshape(randperm, Kr, N)
        else:
            tmpK = N
            use = np.tile(np.arange(N), (Kr, 1))
        _, gc, gv, lp = gmm_mix_hier_em(pc, pv, full, tmpK, opt["Nv"] * Kb,
                                        int(opt["initopt"]["iter"]), rng)
        if "m" in iom:
            # (:360-411) base HMM -> group by summed log-posterior, base state -> group ROI
            newA = np.zeros((Kr, N, N))
            newp = np.zeros((Kr, N))
            col = {ib: c for c, ib in enumerate(idx)}
            for i in range(Kb):
                n = int(bn["nstates"][i])
                ll = np.stack([lp[:, col[(i, s)]] for s in range(n)], axis=1)   # [tmpK][n]
                myj = int(np.argmax([ll[use[j]].sum() for j in range(Kr)]))
                mp = np.argmax(ll[use[myj]], axis=0)
                for k in range(n):
                    newp[myj, mp[k]] += bn["prior"][i, k]
                    for l in range(n):
                        newA[myj, mp[k], mp[l]] += bn["A"][i, k, l]
            with np.errstate(invalid="ignore", divide="ignore"):
                newp = newp / newp.sum(1, keepdims=True)
                newA = newA / newA.sum(2, keepdims=True)
        for j in range(Kr):
            cen[j], cov[j] = gc[use[j]], gv[use[j]]
            rng.random(N)                           # (:472 the emissions' priors, M = 1)
            if "m" in iom:
                prior[j], A[j] = newp[j], newA[j]
            else:
                prior[j], A[j] = make_a_prior(N, iom, rng)
        omega = rng.random(Kr)
        omega = omega / omega.sum()
    else:
        raise ValueError(f"initmode {mode!r} is not supported")
    return dict(omega=omega, prior=prior, A=A, centres=np.array(cen), covars=np.array(cov),
                LogL=-np.inf)


def _init_base(base: BaseSet, rng: np.random.Generator) -> BaseSet:
    """hem_h3m_c.m:263-275: initialise from a random run of 400 consecutive base HMMs."""
    if base.N <= 400:
        return base
    i0 = int(rng.integers(0, base.N - 400))
    sub = base.shard(i0, i0 + 400)
    return BaseSet(sub.nstates, sub.prior, sub.A, sub.centres, sub.covars,
                   sub.omega / sub.omega.sum(), sub.covmode)


def planted_hmms(n_per: int = 20, seed: int = 0, noise: float = 0.1):
    """The exprmt1 recipe (Synthetic_experiment/exprmt1_sampledata.m:20-43) as point
    HMMs: two ground-truth HMMs that differ in their transitions only, ``n_per``
    subject HMMs each (subject i belongs to ground truth i mod 2), means perturbed by
    N(0, noise^2) and the transition rows and priors by a Dirichlet draw around the
    truth.  Returns (hmms, labels)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt_A = np.array([[[0.6, 0.4], [0.4, 0.6]], [[0.4, 0.6], [0.6, 0.4]]])
    gt_mu = np.array([[0.0, 0.0], [3.0, 3.0]])
    hmms, labels = [], []
    for i in range(2 * n_per):
        g = i % 2
        A = np.stack([rng.dirichlet(1.0 + 250.0 * gt_A[g, s]) for s in range(2)])
        prior = rng.dirichlet(1.0 + 25.0 * np.array([0.5, 0.5]))
        hmms.append(dict(prior=prior, trans=A,
                         pdf=[dict(mean=gt_mu[s] + noise * rng.standard_normal(2), cov=np.eye(2))
                              for s in range(2)]))
        labels.append(g)
    return hmms, np.array(labels)


# ----------------------------------------------------------------------------
# trials and the driver
# ----------------------------------------------------------------------------
def _device_engine(device):
    from .estep import EStepEngine
    dev = torch.device(device)
    return lambda base, K, S, T, trials=1: EStepEngine(base, K, S, T, device=dev, trials=trials)


def hem_h3m_c(base: BaseSet, opt: dict, device="cuda", engine_factory=None,
              inits: Optional[List[dict]] = None) -> dict:
    """hem_h3m_c.m ('base', 'baseem', 'gmmNew', 'gmmNew2'): ``trials`` EM runs, trial t
    seeded seed + t, batched in launches of at most MAX_BATCH_CLUSTERS clusters; the
    best LogL wins (MATLAB's max skips NaN).  opt['em_engine'] = 'device' keeps the EM
    loop of every chunk inside the device engine's shapes on the GPU
    (:func:`hem_h3m_c_trials`); any other chunk takes the host engine, with either
    setting.  K == Kb returns the base mixture
    (:19-25).  Every trial NaN raises ValueError (the reference's redo ladder,
    :304-320, is reduced to that).  ``inits``: the trials' initial mixtures (skips the
    initialisation)."""
    K, S = int(opt["K"]), int(opt["N"])
    Kb = base.N
    if K == Kb or K == 0 or Kb == 0:
        bn = base.numpy()
        return dict(omega=bn["omega"], prior=bn["prior"], A=bn["A"], centres=bn["centres"],
                    covars=bn["covars"], nstates=bn["nstates"], LogL=0.0, LogLs=[0.0],
                    Z=np.eye(K))
    R = int(opt["trials"]) if inits is None else len(inits)
    rngs = [np.random.Generator(np.random.PCG64(int(opt["seed"]) + t)) for t in range(1, R + 1)]
    if inits is None:
        inits = [initialize_hem_h3m_c(_init_base(base, rngs[t]), opt, rngs[t]) for t in range(R)]
    make = engine_factory or _device_engine(device)
    outs: List[dict] = []
    per = max(1, MAX_BATCH_CLUSTERS // K) if (S <= 16 and base.SB <= S) else 1
    from .estep import EStepEngine
    want_device = opt.get("em_engine", "host") == "device"
    for r0 in range(0, R, per):
        chunk = inits[r0:r0 + per]
        eng = make(base, len(chunk) * K, S, int(opt["tau"]), trials=len(chunk))
        on_device = (want_device and isinstance(eng, EStepEngine)
                     and device_em_supported(base, K, S, len(chunk), opt))
        outs.extend(hem_h3m_c_trials(chunk, eng, opt, rngs[r0:r0 + per],
                                     em_engine="device" if on_device else "host"))
        del eng
    all_LL = np.array([o["LogL"] for o in outs], dtype=float)
    ok = np.isfinite(all_LL) | (all_LL == np.inf)
    if not ok.any():
        raise ValueError("every VHEM trial ended with a NaN or -inf log-likelihood")
    best = int(np.nanargmax(np.where(np.isnan(all_LL), -np.inf, all_LL)))
    out = dict(outs[best])
    out["t_best"] = best
    out["trials_LL"] = all_LL
    if opt.get("keep_suboptimal_hmms", 0):
        uniq = unique_ll(all_LL, 2 * opt["termvalue"] * 10)
        out["suboptimal_h3ms"] = [outs[q] for q in uniq]
    return out


def vhem_cluster(hmms: list, K: int, S: Optional[int] = None, hemopt: Optional[dict] = None,
                 device="cuda", engine_factory=None) -> dict:
    """vhem_cluster.m: cluster point-estimate HMMs (dicts with prior, trans,
    pdf[{mean, cov}]; None = empty) into K group HMMs of S states
    (default: ceil(median) of the inputs' state counts).  hemopt['seed'] is required.
    initmode 'auto' runs 'baseem' / 'u', 'gmmNew' / 'r0' and 'gmmNew2' / 'u0'; the
    best LogL wins.  Returns the h3m_to_hmms dict (+ hemopt, initmode)."""
    hemopt = dict(hemopt or {})
    if hemopt.get("remove_empty", 1):
        from .vbhmm_em import vbhmm_remove_empty
        hmms = [vbhmm_remove_empty(h, 1e-3) if (h is not None and "N" in h and "varpar" in h) else h
                for h in hmms]
    if S is None:
        S = int(np.ceil(np.median([len(h["prior"]) for h in hmms if h is not None])))
    opt = default_hemopt(K, S, **hemopt)
    covmode = COV_FULL if opt["covar_type"] == "full" else COV_DIAG
    base = hmms_to_h3m(hmms, covmode)
    if opt["initmode"] != "auto":
        h3m = hem_h3m_c(base, opt, device, engine_factory)
        used = opt["initmode"]
    else:
        modes, iopts = ["baseem", "gmmNew", "gmmNew2"], ["u", "r0", "u0"]
        runs = [hem_h3m_c(base, dict(opt, initmode=m, initopt=dict(opt["initopt"], mode=io)),
                          device, engine_factory) for m, io in zip(modes, iopts)]
        lls = np.array([r["LogL"] for r in runs], dtype=float)
        ind = int(np.nanargmax(lls))
        h3m, used = runs[ind], modes[ind]
    out = h3m_to_hmms(h3m, covmode)
    if opt["sortclusters"]:
        from .vbhmm_em import vbhmm_standardize
        std = []
        for g in out["hmms"]:
            g2 = dict(g)
            stats = g2.pop("stats", None)
            if stats is not None:
                g2["N"] = stats["emit_vcounts"]     # carried through the permutation
            s = vbhmm_standardize(g2, opt["sortclusters"])
            if stats is not None:
                s["stats"] = dict(emit_vcounts=s.pop("N"))
            std.append(s)
        out["hmms"] = std
    if opt.get("keep_suboptimal_hmms", 0) and "suboptimal_h3ms" in h3m:
        out["suboptimal_hmms"] = [h3m_to_hmms(s, covmode) for s in h3m["suboptimal_h3ms"]]
    if "trials_LL" in h3m:
        out["trials_LL"] = h3m["trials_LL"]
    out["hemopt"] = opt
    out["initmode"] = used
    return out
