"""numpy restatement of the reference's VHEM clustering step, written from the MATLAB
(src/compare_mtds/hem/vhem_h3m/hem_h3m_c_step.m, hem_mstep_component.m,
hem_fix_degenerate_component.m, hem_fix_degenerate_hmm.m, ../hmms_to_h3m.m), with
loops where the MATLAB has loops.  The per-pair quantities (hem_hmm_bwd_fwd_mex) come
from the oracle (vbhem_oracle.c_vhem_estep_pairs).  The checker of tests/test_vhem*.py;
it imports nothing from the package.

Base mixture: the packed numpy dict of BaseSet.numpy() (nstates, prior, A, centres,
covars, omega, covmode).  Reduced mixture: dict(omega [K], prior [K][S], A [K][S][S],
centres [K][S][d], covars [K][S][d][d] | [K][S][d], LogL).
"""
import copy

import numpy as np

import vbhem_oracle as vo

COV_DIAG, COV_FULL = 0, 1


def inf_norm_of(mode, T, Nv, Kb):
    """hem_h3m_c_step.m:110-119."""
    return {"": 1.0, "n": Nv / Kb, "tn": T * Nv / Kb, "nt": T * Nv / Kb, "t": float(T)}[mode]


def logtrick_rows(lA):
    """logtrick(lA')' (hem_h3m_c_step.m:521-535): log sum exp of every row."""
    out = np.zeros(lA.shape[0])
    for i in range(lA.shape[0]):
        mv = np.max(lA[i])
        out[i] = mv + np.log(np.sum(np.exp(lA[i] - mv)))
    return out


def hmms_to_h3m(hmms, covmode):
    """hmms_to_h3m.m -> packed base dict."""
    K = len(hmms)
    nin = next(len(h["pdf"][0]["mean"]) for h in hmms if h is not None)
    SB = max(len(h["prior"]) if h is not None else 1 for h in hmms)
    out = dict(nstates=np.ones(K, dtype=np.int32), prior=np.zeros((K, SB)), A=np.zeros((K, SB, SB)),
               centres=np.zeros((K, SB, nin)),
               covars=np.zeros((K, SB, nin, nin) if covmode == COV_FULL else (K, SB, nin)),
               omega=np.ones(K), covmode=covmode)
    for j, h in enumerate(hmms):
        if h is not None:
            s = len(h["prior"])
            out["nstates"][j] = s
            out["prior"][j, :s] = h["prior"]
            out["A"][j, :s, :s] = h["trans"]
            for i in range(s):
                out["centres"][j, i] = h["pdf"][i]["mean"]
                c = np.asarray(h["pdf"][i]["cov"], dtype=float)
                out["covars"][j, i] = c if covmode == COV_FULL else np.diag(c)
        else:
            out["prior"][j, 0] = 1.0
            out["A"][j, 0, 0] = 1.0
            out["covars"][j, 0] = np.eye(nin) if covmode == COV_FULL else np.ones(nin)
            out["omega"][j] = 0.0
    out["omega"] = out["omega"] / np.sum(out["omega"])
    return out


def estep(base, h3m_r, opt):
    """hem_h3m_c_step.m:185-314: pairs, L_elbo / inf_norm, log_Z, Z, LogL."""
    Kb = base["prior"].shape[0]
    T = opt["tau"]
    red = {k: h3m_r[k] for k in ("A", "prior", "centres", "covars")}
    pairs = vo.c_vhem_estep_pairs(base, red, T, opt["smooth"])
    N_i = opt["Nv"] * base["omega"] * Kb                                  # :61
    inf_norm = inf_norm_of(opt["inf_norm"], T, opt["Nv"], Kb)
    L_elbo = pairs["LL_elbo"] / inf_norm                                   # :293
    with np.errstate(divide="ignore"):
        log_Z = np.log(h3m_r["omega"])[None, :] + N_i[:, None] * L_elbo    # :294
    lt = logtrick_rows(log_Z)
    Z = np.exp(log_Z - lt[:, None])                                        # :297
    return dict(pairs=pairs, L_elbo=L_elbo, log_Z=log_Z, Z=Z, LogL=float(np.sum(lt)), N_i=N_i)


def mstep_sums(base, es, j):
    """hem_mstep_component.m:84-121 for reduced component j: the sums over the bases
    with Zomega(i) > 0."""
    pairs, Z = es["pairs"], es["Z"]
    Kb = Z.shape[0]
    Zj = Z[:, j] * base["omega"]                                           # c_step:443
    S = pairs["sum_nu_1"].shape[2]
    new_prior = np.zeros(S)
    new_A = np.zeros((S, S))
    new_Gweight = np.zeros(S)
    new_Gmu = np.zeros(pairs["emit_mu"].shape[2:])
    new_GMu = np.zeros(pairs["emit_Mu"].shape[2:])
    for i in range(Kb):
        if Zj[i] > 0:
            new_prior = new_prior + Zj[i] * pairs["sum_nu_1"][i, j]
            new_A = new_A + Zj[i] * pairs["sum_xi"][i, j]
            for n in range(S):
                new_Gweight[n] = new_Gweight[n] + Zj[i] * pairs["emit_pr"][i, j, n]
                new_Gmu[n] = new_Gmu[n] + Zj[i] * pairs["emit_mu"][i, j, n]
                new_GMu[n] = new_GMu[n] + Zj[i] * pairs["emit_Mu"][i, j, n]
    return dict(new_prior=new_prior, new_A=new_A, new_Gweight=new_Gweight, new_Gmu=new_Gmu,
                new_GMu=new_GMu)


def mstep_finish(sums, tau, reg_cov, covmode):
    """hem_mstep_component.m:123-166."""
    new_prior, new_A = sums["new_prior"], sums["new_A"]
    S = new_prior.shape[0]
    dim = sums["new_Gmu"].shape[1]
    if S == 1:
        new_A = np.full((1, 1), 1e-12)
    if tau == 1:
        new_A = 1e-12 * np.eye(S)
    hmm = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        hmm["prior"] = new_prior / np.sum(new_prior)
        hmm["A"] = new_A / np.sum(new_A, axis=1)[:, None]
        hmm["emit_vcounts"] = np.sum(new_A, axis=0) + new_prior
        hmm["centres"] = np.zeros((S, dim))
        hmm["covars"] = np.zeros((S, dim, dim) if covmode == COV_FULL else (S, dim))
        for n in range(S):
            w = sums["new_Gweight"][n]
            c = sums["new_Gmu"][n] / w
            hmm["centres"][n] = c
            if covmode == COV_DIAG:
                Sigma = sums["new_GMu"][n] - 2 * (sums["new_Gmu"][n] * c) + (c ** 2) * w
                hmm["covars"][n] = Sigma / w + reg_cov
            else:
                tmp = np.outer(sums["new_Gmu"][n], c)
                tmp2 = w * np.outer(c, c)
                Sigma = sums["new_GMu"][n] - tmp - tmp.T + tmp2
                hmm["covars"][n] = Sigma / w + reg_cov * np.eye(dim)
    return hmm


def packed_stats(base, es, covmode):
    """The fused VHEM E-step's outputs from the restatement: Nj, N1, M, Nr, Y, SC (the
    host.unpack_stats names) and LogL."""
    K = es["Z"].shape[1]
    sums = [mstep_sums(base, es, j) for j in range(K)]
    return dict(Nj=np.sum(es["Z"], axis=0), N1=np.stack([s["new_prior"] for s in sums]),
                M=np.stack([s["new_A"] for s in sums]), Nr=np.stack([s["new_Gweight"] for s in sums]),
                Y=np.stack([s["new_Gmu"] for s in sums]), SC=np.stack([s["new_GMu"] for s in sums]),
                LogL=es["LogL"])


def fix_degenerate_component(h, iz, N, draw):
    """hem_fix_degenerate_component.m; draw(shape) = rand(shape)."""
    highest = int(np.argmax(h["omega"]))
    h["omega"][[iz, highest]] = h["omega"][highest] / 2
    h["omega"] = h["omega"] / np.sum(h["omega"])
    for k in ("centres", "covars", "emit_vcounts"):
        h[k][iz] = h[k][highest]
    prior = h["prior"][highest] + (.1 / N) * draw(h["prior"][highest].shape)
    A = h["A"][highest]
    f_zeros = A == 0
    A = (.1 / N) * draw(A.shape)
    A[f_zeros] = 0
    h["prior"][iz] = prior / np.sum(prior)
    h["A"][iz] = A / np.sum(A, axis=1)[:, None]


def fix_degenerate_hmm(h, j, iz, draw):
    """hem_fix_degenerate_hmm.m on reduced component j."""
    highest = int(np.argmax(h["emit_vcounts"][j]))
    h["prior"][j][[iz, highest]] = h["prior"][j][highest] / 2
    h["prior"][j] = h["prior"][j] / np.sum(h["prior"][j])
    h["A"][j][iz, :] = h["A"][j][highest, :]
    half = h["A"][j][:, highest] / 2
    h["A"][j][:, iz] = half
    h["A"][j][:, highest] = half
    h["covars"][j][iz] = h["covars"][j][highest]
    c = h["centres"][j][highest].copy()
    h["centres"][j][iz] = c + (0.01 * draw(c.shape)) * c


def c_step(h3m_r, base, opt, draw=None, estep_fn=estep):
    """hem_h3m_c_step.m.  Returns the final mixture with Z, LogL, LogLs, L_elbo1,
    num_iter and fixes (the number of degenerate fixes that fired)."""
    covmode = base["covmode"]
    Kb = base["prior"].shape[0]
    h = copy.deepcopy(h3m_r)
    Kr, Nr = h["prior"].shape
    dim = h["centres"].shape[2]
    N = int(base["nstates"][0])
    reg_cov = opt.get("reg_cov", 0)
    h["covars"] = h["covars"] + (reg_cov * np.eye(dim) if covmode == COV_FULL else reg_cov)
    h["LogLs"] = []
    num_iter = 0
    fixes = 0
    while True:
        es = estep_fn(base, h, opt)
        new_LL = es["LogL"]
        old_LL = h["LogL"]
        h["LogL"] = new_LL
        h["LogLs"].append(new_LL)
        h["Z"] = es["Z"]
        stop = False
        if num_iter > 1:
            with np.errstate(invalid="ignore", divide="ignore"):
                changeLL = (new_LL - old_LL) / abs(old_LL)
        else:
            changeLL = np.inf
        if changeLL < opt["termvalue"]:
            stop = True
        if num_iter > opt["max_iter"]:
            stop = True
        if stop and num_iter >= opt.get("min_iter", 0):
            break
        num_iter += 1
        new = dict(omega=np.sum(es["Z"], axis=0) / Kb, LogL=h["LogL"], LogLs=h["LogLs"], Z=h["Z"])
        comps = [mstep_finish(mstep_sums(base, es, j), opt["tau"], reg_cov, covmode)
                 for j in range(Kr)]
        for k in ("prior", "A", "centres", "covars", "emit_vcounts"):
            new[k] = np.stack([c[k] for c in comps])
        for iz in np.flatnonzero(new["omega"] == 0):
            fix_degenerate_component(new, int(iz), N, draw)
            fixes += 1
        for j in range(Kr):
            for iz in np.flatnonzero(new["emit_vcounts"][j] == 0):
                fix_degenerate_hmm(new, j, int(iz), draw)
                fixes += 1
        h = new
    h["L_elbo1"] = es["L_elbo"]
    h["num_iter"] = num_iter
    h["fixes"] = fixes
    return h
