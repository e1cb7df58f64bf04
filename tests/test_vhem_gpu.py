"""The fused VHEM E-step (vhem_estep_fused / _trials), the EM loop and vhem_cluster on
the GPU against the numpy restatement of the reference (tests/vhem_ref.py).

Every fused case has N = 200 bases (several chunks of >= 64 bases, a short last one),
one cluster with zero transitions (log A = -inf), one base with omega_b = 0 and, for
K >= 2, one cluster with omega_r = 0.  The clusters are near copies of each other with
a growing offset, so Z is spread: entries between 0 and 1e-8 exist (a 1e-8 gate would
show at the 1e-10 bound) and, with inf_norm = '' (Nv = 100), some underflow to 0."""
import functools

import numpy as np
import pytest
import torch

import vhem_ref as ref
from cases import make_case, make_reduced
from conftest import RTOL_NORTH_STAR, RTOL_PAIRS, elem_err, hatz_err, stat_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 200

# name: (S, Sb, d, cov, ragged, T, K, smooth, inf_norm)
CASES = {
    # S = 8, T = 10: the shape of fb_bwd4_kernel / fb_list4_kernel (the VHEM call takes its
    # first pass on fb_split_kernel's backward mode, the list pass on fb_list4_kernel)
    "bwd4_K16": (8, 8, 8, 1, True, 10, 16, 1.0, "nt"),
    "bwd4_K3": (8, 8, 8, 1, True, 10, 3, 2.5, ""),
    "bwd4_K65": (8, 8, 8, 1, True, 10, 65, 1.0, "n"),
    # S = 12: the shape of fb_bwd12_kernel / fb_list12_kernel (likewise)
    "bwd12_K4": (12, 12, 4, 1, False, 10, 4, 2.5, "t"),
    "bwd12_K1": (12, 12, 4, 1, False, 10, 1, 1.0, "nt"),
    # d = 2 diag: the short-K1 shape (K1 inside fb_bwd2_kernel for VBHEM; VHEM: emission GEMM)
    "k1_K4": (5, 5, 2, 0, False, 10, 4, 1.0, "nt"),
    "k1_K5": (5, 5, 2, 0, False, 10, 5, 2.5, "t"),      # masked lanes (G = 8)
    "k1_K16": (5, 5, 2, 0, False, 10, 16, 2.5, "n"),
    "k1_K65": (5, 5, 2, 0, False, 10, 65, 1.0, ""),     # K > 64: the loop path
    "small_K1": (3, 3, 2, 1, True, 7, 1, 2.5, "nt"),
    "small_K3": (3, 3, 2, 1, True, 7, 3, 1.0, "t"),
    "small_K4": (3, 3, 2, 1, True, 7, 4, 2.5, ""),
    "small_K16": (3, 3, 2, 1, True, 7, 16, 1.0, "n"),
    "small_K65": (3, 3, 2, 1, True, 7, 65, 2.5, "nt"),
    # Sb > S: fb_pairs_kernel (generic path, dense statistics)
    "pairs_K3": (2, 5, 2, 1, False, 4, 3, 2.5, "nt"),
    "pairs_K16": (2, 5, 2, 1, False, 4, 16, 1.0, ""),
    # state counts with padded rows in fb_split_kernel: the first pass's backward mode at
    # S = 7 (one lane per column), 9 and 13 (two lanes, odd S), the list pass on four lanes
    # at S = 9 (the last lane's rows all padded) and 13 (the names sort last: the seeds of
    # the cases above stay what they were)
    "split_S7": (7, 7, 2, 1, True, 10, 3, 2.5, "nt"),
    "split_S9": (9, 9, 3, 1, True, 10, 4, 1.0, "t"),
    "split_S13": (13, 11, 2, 0, False, 7, 3, 2.5, ""),
}
NV = 100


def near_reduced(K, S, d, cov, seed):
    """K reduced HMMs: cluster j = cluster 0 with its means moved by 0.03 j (+ 0.12 for
    odd j) along a fixed direction and its transition rows mixed with j's own; cluster 0 has zero
    transitions (cases.make_reduced)."""
    r0 = make_reduced(1, S, d, cov, seed=seed, zero_transition=True)
    rk = make_reduced(K, S, d, cov, seed=seed + 1)
    rng = np.random.default_rng(seed)
    dirn = rng.normal(size=(S, d))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    out = {k: np.repeat(r0[k], K, axis=0) for k in r0}
    for j in range(1, K):
        out["centres"][j] = r0["centres"][0] + (0.03 * j + 0.12 * (j % 2)) * dirn
        out["A"][j] = 0.8 * r0["A"][0] + 0.2 * rk["A"][j]
        out["prior"][j] = 0.8 * r0["prior"][0] + 0.2 * rk["prior"][j]
    return out


@functools.lru_cache(maxsize=None)
def fused_case(name):
    """(base dict, BaseSet, reduced mixture, options, the restatement's E-step and its
    packed statistics) -- computed once, shared by the tests, never modified."""
    return build_fused(CASES[name], 7000 + sorted(CASES).index(name))


def build_fused(shape, seed, N=N):
    """fused_case's recipe for a shape tuple laid out as CASES' values, on N > 7 bases."""
    S, Sb, d, cov, ragged, T, K, smooth, norm = shape
    cs = make_case(N, 2, S, Sb, d, cov, seed=seed, ragged=ragged, tau=T)
    base = cs["base"]
    om = np.ones(N)
    om[7] = 0.0                                    # a base with omega_b = 0
    base["omega"] = om / om.sum()
    # bases near the clusters: their means scattered around cluster 0's
    red = near_reduced(K, S, d, cov, seed)
    rng = np.random.default_rng(seed + 5)
    base["centres"] = (red["centres"][0][None, :Sb] if Sb <= S else
                       np.resize(red["centres"][0], (Sb, d))[None]) + \
        rng.normal(0.0, 0.3, base["centres"].shape)
    mask = np.arange(Sb)[None, :] < base["nstates"][:, None]
    base["centres"] = base["centres"] * mask[..., None]
    omega = rng.dirichlet(np.ones(K) * 5)
    if K >= 2:
        omega[K - 1] = 0.0                         # a cluster with omega_r = 0
        omega /= omega.sum()
    h = dict(red, omega=omega, LogL=-np.inf)
    opt = dict(tau=T, Nv=NV, inf_norm=norm, smooth=smooth)
    es = ref.estep(base, h, opt)
    return base, h, opt, es, ref.packed_stats(base, es, cov)


def gpu_engine(vb, base, K, S, T, trials=1):
    from vbhem_amd.estep import EStepEngine
    return EStepEngine(vb.BaseSet.from_numpy(base), K, S, T, device=DEV, trials=trials)


def run_fused(vb, eng, base, h, opt):
    """One fused VHEM call: (unpacked statistics, Z, raw vector)."""
    cov = base["covmode"]
    Kb = base["prior"].shape[0]
    eng.set_clusters(vb.host.vhem_cluster_constants(h, cov))
    with np.errstate(divide="ignore"):
        eng.set_log_omega(np.log(h["omega"]))
    ob = torch.as_tensor(base["omega"], device=DEV)
    Ni = (float(opt["Nv"]) * ob) * float(Kb)
    inn = ref.inf_norm_of(opt["inf_norm"], opt["tau"], opt["Nv"], Kb)
    vec = eng.fused_vhem(Ni, ob, inn, opt["smooth"]).cpu().numpy().copy()
    return vec, eng.hatZ.cpu().numpy().copy()


@pytest.fixture(params=["gated", "dense"])
def schedule(request, capi_lib):
    from vbhem_amd import _capi
    prev = _capi.set_fused_mode(_capi.FUSED_GATED if request.param == "gated" else _capi.FUSED_DENSE)
    yield request.param
    _capi.set_fused_mode(prev)


def check_fused(vb, name, vec, Z):
    check_fused_shape(vb, name, CASES[name], fused_case(name), vec, Z)


def check_fused_shape(vb, name, shape, case, vec, Z):
    """check_fused's bars on a build_fused case."""
    base, h, opt, es, want = case
    S, Sb, d, cov, ragged, T, K, smooth, norm = shape
    got = vb.host.unpack_stats(vec, K, S, d, cov)
    figs = {k: stat_err(got[k], want[k]) for k in ("N1", "M", "Nr", "Y", "SC")}
    figs["Nj"] = stat_err(got["Nj"], want["Nj"])
    figs["Z"] = hatz_err(Z, es["Z"])
    figs["rows"] = float(np.abs(Z.sum(1) - 1.0).max())
    figs["LogL"] = abs(got["Lt1"] - want["LogL"]) / abs(want["LogL"])
    print(name, {k: f"{v:.2e}" for k, v in figs.items()})
    assert not np.isnan(vec).any() and not np.isnan(Z).any()
    assert got["Lt7"] == 0.0
    for k in ("N1", "M", "Nr", "Y", "SC"):
        assert figs[k] <= RTOL_PAIRS, (k, figs[k])
    assert figs["Z"] <= 1e-10
    assert figs["rows"] <= 1e-14
    assert figs["LogL"] <= 1e-12
    assert figs["Nj"] <= 1e-12
    if K >= 2:
        assert np.all(Z[:, K - 1] == 0.0)          # omega_r = 0: exactly 0
        assert got["Nj"][K - 1] == 0.0 and np.all(got["N1"][K - 1] == 0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_vhem_matches_restatement(vb, vo, schedule, name):
    """Statistics stat_err <= RTOL_PAIRS, Z hatz_err <= 1e-10 with rows summing to 1
    within 1e-14, LogL 1e-12 relative, Nj 1e-12.

    lz = log omega + (N_i / inf_norm) L_elbo multiplies the recursion's rounding by
    N_i / inf_norm = 20 ('nt'), 200 ('n'), 100 ('') at N = 200, so the bounds on Z and
    Nj hold L_elbo to about one unit in its last place.  The VHEM call therefore takes
    L_elbo, in both schedules, from the recursion with the dense schedule's arithmetic
    (DESIGN.md section 4.11).  Measured on an MI355X, worst of the 32 runs: statistics
    7.0e-11, Z 2.0e-11, Nj 7.2e-13 (all bwd4_K65, inf_norm 'n'), rows 4.4e-16, LogL
    2.1e-16."""
    base, h, opt, es, want = fused_case(name)
    S, Sb, d, cov, ragged, T, K, smooth, norm = CASES[name]
    if name == "k1_K65":
        # inf_norm = '', Nv = 100: the > 0 gate really excludes pairs here -- zero and
        # non-zero off-winner entries in the restatement
        off = np.sort(es["Z"][:, :K - 1], axis=1)[:, :-1]
        assert (off == 0).any() and (off > 0).any()
    eng = gpu_engine(vb, base, K, S, T)
    vec, Z = run_fused(vb, eng, base, h, opt)
    if name.startswith("split_") and schedule == "gated":
        # the instances these cases are here for: fb_split_kernel<S, LPC, mode>, backward
        # (1) then list (2) mode
        from vbhem_amd import _capi
        assert (_capi.last_kernel(0), _capi.last_kernel(1)) == (
            "vbhem::fb_split_kernel<%d, %d, 1>" % (S, 1 if S <= 8 else 2),
            "vbhem::fb_split_kernel<%d, %d, 2>" % (S, 2 if S <= 8 else 4))
    check_fused(vb, name, vec, Z)


def test_omega_b_zero_contributes_nothing(vb, vo):
    """Dropping the omega_b = 0 base changes nothing but Nj and LogL (its Z row)."""
    name = "k1_K4"
    base, h, opt, es, want = fused_case(name)
    S, Sb, d, cov, ragged, T, K, smooth, norm = CASES[name]
    vec, _ = run_fused(vb, gpu_engine(vb, base, K, S, T), base, h, opt)
    keep = np.arange(N) != 7
    sub = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    eng = gpu_engine(vb, sub, K, S, T)
    eng.set_clusters(vb.host.vhem_cluster_constants(h, cov))
    with np.errstate(divide="ignore"):
        eng.set_log_omega(np.log(h["omega"]))
    ob = torch.as_tensor(sub["omega"], device=DEV)
    Ni = (float(NV) * ob) * float(N)               # N_i of the full set
    vec2 = eng.fused_vhem(Ni, ob, ref.inf_norm_of(norm, T, NV, N), smooth).cpu().numpy()
    a = vb.host.unpack_stats(vec, K, S, d, cov)
    b = vb.host.unpack_stats(vec2, K, S, d, cov)
    for k in ("N1", "M", "Nr", "Y", "SC"):
        assert stat_err(a[k], b[k]) <= 1e-13, k   # (the same terms, chunked differently)


@pytest.mark.parametrize("name", ["bwd4_K16", "k1_K65", "small_K3", "pairs_K3"])
def test_schedules_agree_and_calls_repeat(vb, vo, capi_lib, name):
    from vbhem_amd import _capi
    base, h, opt, es, want = fused_case(name)
    S, Sb, d, cov, ragged, T, K, smooth, norm = CASES[name]
    eng = gpu_engine(vb, base, K, S, T)
    out = {}
    prev = _capi.set_fused_mode(_capi.FUSED_GATED)
    try:
        for mode in (_capi.FUSED_GATED, _capi.FUSED_DENSE):
            _capi.set_fused_mode(mode)
            v1, Z1 = run_fused(vb, eng, base, h, opt)
            v2, Z2 = run_fused(vb, eng, base, h, opt)
            assert np.array_equal(v1, v2) and np.array_equal(Z1, Z2)   # bit-identical
            out[mode] = (vb.host.unpack_stats(v1, K, S, d, cov), Z1)
    finally:
        _capi.set_fused_mode(prev)
    g, dn = out[_capi.FUSED_GATED], out[_capi.FUSED_DENSE]
    # (the schedules take L_elbo from different recursion kernels: equal to rounding)
    assert hatz_err(g[1], dn[1]) <= 1e-10
    for k in ("Nj", "N1", "M", "Nr", "Y", "SC"):
        assert stat_err(g[0][k], dn[0][k]) <= 1e-10, k
    assert abs(g[0]["Lt1"] - dn[0]["Lt1"]) <= 1e-10 * abs(dn[0]["Lt1"])


@pytest.mark.parametrize("name", ["bwd4_K3", "k1_K5", "small_K4"])
def test_trials_equal_single_calls(vb, vo, name):
    """R = 3 different initialisations in one vhem_estep_fused_trials call equal three
    single calls bit for bit."""
    base, h, opt, es, want = fused_case(name)
    S, Sb, d, cov, ragged, T, K, smooth, norm = CASES[name]
    hs = []
    for r in range(3):
        rng = np.random.default_rng(50 + r)
        hr = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in h.items()}
        hr["centres"] = hr["centres"] + 0.05 * rng.normal(size=hr["centres"].shape)
        hr["omega"] = rng.dirichlet(np.ones(K))
        hs.append(hr)
    big = {k: np.concatenate([x[k] for x in hs]) for k in ("A", "prior", "centres", "covars", "omega")}
    vec, Z = run_fused(vb, gpu_engine(vb, base, 3 * K, S, T, trials=3), base, big, opt)
    SL = vec.size // 3
    one = gpu_engine(vb, base, K, S, T)
    for r in range(3):
        v1, Z1 = run_fused(vb, one, base, hs[r], opt)
        assert np.array_equal(v1, vec[r * SL:(r + 1) * SL]), r
        assert np.array_equal(Z1, Z[:, r * K:(r + 1) * K]), r


def test_trials_beyond_256_clusters(vb, vo):
    """R = 80 trials of K = 4 (320 clusters: past the VBHEM trials call's 256) in one
    call; the first, a middle and the last trial equal their single calls bit for bit."""
    base, h, opt, es, want = fused_case("small_K4")
    S, Sb, d, cov, ragged, T, K, smooth, norm = CASES["small_K4"]
    R = 80
    hs = []
    for r in range(R):
        rng = np.random.default_rng(900 + r)
        hr = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in h.items()}
        hr["centres"] = hr["centres"] + 0.05 * rng.normal(size=hr["centres"].shape)
        hr["omega"] = rng.dirichlet(np.ones(K))
        hs.append(hr)
    big = {k: np.concatenate([x[k] for x in hs]) for k in ("A", "prior", "centres", "covars", "omega")}
    vec, Z = run_fused(vb, gpu_engine(vb, base, R * K, S, T, trials=R), base, big, opt)
    SL = vec.size // R
    one = gpu_engine(vb, base, K, S, T)
    for r in (0, 41, R - 1):
        v1, Z1 = run_fused(vb, one, base, hs[r], opt)
        assert np.array_equal(v1, vec[r * SL:(r + 1) * SL]), r
        assert np.array_equal(Z1, Z[:, r * K:(r + 1) * K]), r


def test_folded_fallback(vb, vo, schedule):
    """Pairs whose factorised normaliser underflows take the exact fallback (folded into
    the responsibilities kernel in the gated schedule): cluster 0's transitions put
    their mass on sigma + 1 while its emissions favour state 0."""
    S, Sb, d, cov, T, K = 4, 4, 3, 0, 6, 3
    cs = make_case(70, K, S, Sb, d, cov, seed=99, tau=T)
    base = cs["base"]
    red = make_reduced(K, S, d, cov, seed=99)
    A = np.full((S, S), np.exp(-600.0))
    for r in range(S):
        A[r, (r + 1) % S] = 1.0
    red["A"][0] = A
    red["covars"][0, 1:] = np.exp(400.0)
    h = dict(red, omega=np.array([0.5, 0.3, 0.2]), LogL=-np.inf)
    opt = dict(tau=T, Nv=NV, inf_norm="nt", smooth=1.0)
    es = ref.estep(base, h, opt)
    want = ref.packed_stats(base, es, cov)
    eng = gpu_engine(vb, base, K, S, T)
    vec, Z = run_fused(vb, eng, base, h, opt)
    assert eng.fallback_count() > 0
    got = vb.host.unpack_stats(vec, K, S, d, cov)
    for k in ("Nj", "N1", "M", "Nr", "Y", "SC"):
        assert stat_err(got[k], want[k]) <= RTOL_PAIRS, k
    assert hatz_err(Z, es["Z"]) <= 1e-10
    assert abs(got["Lt1"] - want["LogL"]) <= 1e-12 * abs(want["LogL"])


@pytest.mark.parametrize("shape", [(8, 8, 8, 1, 10, 16), (5, 5, 2, 0, 10, 8)])
def test_vbhem_unchanged_by_vhem_calls(vb, vo, shape):
    """vbhem_estep_fused before and after a VHEM call on the same engine (the same
    workspace) is bit-identical to itself."""
    S, Sb, d, cov, T, K = shape
    cs = make_case(N, K, S, Sb, d, cov, seed=31, tau=T)
    from vbhem_amd.estep import EStepEngine
    eng = EStepEngine(cs["bs"], K, S, T, device=DEV)
    tN = torch.as_tensor(100.0 * N * cs["base"]["omega"], device=DEV)
    logOm = vb.host.log_omega_tilde(cs["post"]["alpha"])

    def vbhem():
        eng.set_clusters(cs["consts"])
        eng.set_log_omega(logOm)
        return eng.fused(tN).cpu().numpy().copy(), eng.hatZ.cpu().numpy().copy()

    a = vbhem()
    red = near_reduced(K, S, d, cov, 5)
    run_fused(vb, eng, cs["base"], dict(red, omega=np.full(K, 1.0 / K)),
              dict(tau=T, Nv=NV, inf_norm="nt", smooth=2.5))
    b = vbhem()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    want = vo.c_fused(cs["base"], cs["consts"], T, tN.cpu().numpy(), logOm)
    got = vb.host.unpack_stats(a[0], K, S, d, cov)
    for k in ("Nj", "N1", "M", "Nr", "Y", "SC"):
        assert stat_err(got[k], want[k]) < 1e-9, k


# -- EM loop ---------------------------------------------------------------------
def em_case(reg_cov, seed=12):
    cs = make_case(40, 3, 3, 3, 2, 1, seed=seed, ragged=True)
    h0 = make_reduced(3, 3, 2, 1, seed=seed)
    h0.update(omega=np.full(3, 1 / 3), LogL=-np.inf)
    opt = dict(tau=6, Nv=NV, inf_norm="nt", smooth=1.0, reg_cov=reg_cov, termvalue=1e-5,
               max_iter=100, min_iter=1)
    return cs, h0, opt


def test_em_loop_matches_restatement(vb, vo):
    from vbhem_amd import vhem
    cs, h0, opt = em_case(0.001)
    want = ref.c_step(h0, cs["base"], opt, draw=np.random.default_rng(5).random)
    got = vhem.hem_h3m_c_step(h0, gpu_engine(vb, cs["base"], 3, 3, 6), opt, np.random.default_rng(5))
    assert got["num_iter"] == want["num_iter"] and want["num_iter"] >= 2
    assert elem_err(got["LogLs"], want["LogLs"]) <= RTOL_NORTH_STAR
    for k in ("omega", "prior", "A", "centres", "covars"):
        assert elem_err(got[k], want[k], floor_rel=1e-8) <= RTOL_NORTH_STAR, k
    assert hatz_err(got["Z"], want["Z"]) <= RTOL_NORTH_STAR


MONOTONE_SEED = 12


def test_loglikelihood_is_monotone(vb, vo):
    """reg_cov = 0 and no degenerate fix (checked on the restatement): LogLs never
    decreases by more than floating-point slack (1e-10 relative)."""
    from vbhem_amd import vhem
    cs, h0, opt = em_case(0.0, MONOTONE_SEED)
    want = ref.c_step(h0, cs["base"], opt, draw=None)
    assert want["fixes"] == 0 and want["num_iter"] >= 3
    got = vhem.hem_h3m_c_step(h0, gpu_engine(vb, cs["base"], 3, 3, 6), opt)
    L = np.array(got["LogLs"])
    assert np.all(np.diff(L) >= -1e-10 * np.abs(L[:-1])), L


# -- end to end ---------------------------------------------------------------------
PLANTED_SEED, CLUSTER_SEED = 0, 3


def test_vhem_cluster_planted(vb):
    """exprmt1 recipe: two ground-truth HMMs, 20 subject HMMs each."""
    from vbhem_amd import evaluate, vhem
    hm, lab = vhem.planted_hmms(20, seed=PLANTED_SEED)
    out = vhem.vhem_cluster(hm, 2, 2, dict(seed=CLUSTER_SEED, trials=8), device=DEV)
    assert evaluate.rand_index(out["label"], lab)[0] == 1
    assert sorted(out["group_size"].tolist()) == [20, 20]
    assert np.abs(out["Z"].sum(1) - 1).max() <= 1e-14
    assert out["LogL"] == np.nanmax(out["trials_LL"])
    assert out["LogLs"][-1] == out["LogL"]
