"""DIC model selection without a GPU: the restatement of myDIC.m / the BIC and AIC
formulas / vbh3m_remove_empty.m (tests/dic_ref.py) pinned on closed forms, the host build
of the pair routine (csrc/vbhmm_dic_pair.h through tests/diccheck) against the oracle's
VHEM E-step, vbhem_amd/dic.py on a stand-in engine (the oracle's L) against the
restatement, and the workspace bound.

The shapes reach every instance of the GPU kernel, and a guard keeps it so.  The inputs of
the GPU tests' mixed-wave and many-tile cases are built here too, with the conditions under
which they can tell a wrong kernel from a right one."""
import math
import types

import numpy as np
import pytest

import dic_ref as dr
from cases import make_case, make_reduced
from conftest import RTOL_PAIRS, elem_err

EULER = 0.57721566490153286


@pytest.fixture(scope="module")
def dic(vb):
    from vbhem_amd import dic as mod
    return mod


@pytest.fixture(scope="module")
def check_lib():
    return dr.load_diccheck()


# ----------------------------------------------------------------------------
# shapes shared with tests/test_dic_gpu.py
# ----------------------------------------------------------------------------
# name -> (N, Sb, d, T, ragged bases, [cluster sizes of each model], zero transition)
SHAPES = {
    "T1": (5, 3, 2, 1, False, [[3, 3]], False),
    "T2": (5, 3, 2, 2, False, [[3, 3]], False),
    "S1": (4, 3, 2, 5, False, [[1, 1, 1]], False),
    "Sb1": (4, 1, 2, 5, False, [[3, 3]], False),
    "d1": (4, 3, 1, 5, False, [[3, 3]], False),
    "all16": (2, 16, 16, 6, False, [[16, 16]], False),
    "ragged_bases": (9, 4, 3, 7, True, [[4, 4, 4]], False),
    "mixed_sizes": (5, 3, 2, 5, True, [[2, 4, 3], [1, 5]], False),
    "zero_transition": (5, 3, 2, 6, False, [[3, 3]], True),
    # the kernel's (cluster-state bucket, base-state bucket) instances the shapes above miss
    "S8_Sb8": (9, 8, 3, 4, True, [[8, 5], [6]], False),        # (8, 8), mixed sizes
    "S5_Sb9": (5, 9, 2, 4, False, [[5, 7]], False),            # (8, 16)
    "S9_Sb3": (5, 3, 2, 4, False, [[9, 12, 16]], False),       # (16, 4), 3 clusters
    "S16_Sb5": (5, 5, 4, 3, True, [[16, 9]], False),           # (16, 8)
    "d16_S3": (4, 3, 16, 3, False, [[3, 3]], False),           # the longest block of the 4-bucket
    "K64": (3, 2, 2, 3, False, [[2] * 64], False),             # kMaxModelClusters in one model
    # (4, 8) and (4, 16): the edge sweep alone ran them, against the host build only
    "S3_Sb5": (5, 5, 2, 4, False, [[3, 2]], False),
    "S3_Sb9": (5, 9, 2, 4, False, [[3, 3]], False),
}

# The tile, wave and sub-tile sweep of tests/test_dic_gpu.py.  The kernel packs SBP = 4, 8 or
# 16 lanes per base (the bucket of SB): a wave holds 64 / SBP bases, a pass of the workgroup
# (a sub-tile) 256 / SBP, a tile 64.  N on both sides of each, per SB ...
EDGES = {3: [1, 15, 16, 17, 63, 64, 65, 129], 5: [1, 7, 8, 9, 31, 32, 33, 64, 65],
         9: [1, 3, 4, 5, 15, 16, 17, 64, 65]}
# ... and the largest cluster size of the models it runs with, one call per entry: the
# cluster-state buckets 4, 8 and 16.
EDGE_S = (3, 6, 11)


def state_bucket(s):
    """vbhmm_dic_pair.h's state_bucket, restated."""
    return 4 if s <= 4 else 8 if s <= 8 else 16


def build(name, seed=0):
    """(base dict, models) of a shape: make_case's diag base set, make_reduced's group
    HMMs padded to the largest size with each cluster's own count in nstates."""
    N, Sb, d, T, ragged, sizes, zt = SHAPES[name]
    base = make_case(N, 2, 3, Sb, d, 0, seed=70 + seed, ragged=ragged, tau=T)["base"]
    models = []
    for g, sz in enumerate(sizes):
        red = make_reduced(len(sz), max(sz), d, 0, seed=90 + seed + g, zero_transition=zt)
        for j, n in enumerate(sz):     # cluster j keeps its first n states, renormalised
            red["A"][j, :n, :n] /= red["A"][j, :n, :n].sum(-1, keepdims=True)
            red["prior"][j, :n] /= red["prior"][j, :n].sum()
        rng = np.random.default_rng(seed + g)
        om = rng.dirichlet(np.ones(len(sz)))
        models.append(dict(red, nstates=np.array(sz), omega=om, scale=float(rng.uniform(0.5, 3.0))))
    return base, models, T


def oracle_LL(vo, base, models, pk, T):
    L = dr.oracle_pairs(vo, base, models, T)
    return L, dr.mix(L, pk["model_off"], pk["logw"], pk["scale"])


def one_sign(L, pk):
    """The sign condition under which a sum inherits its terms' relative bound: every
    subject's mixture LSE of every model has the same sign."""
    terms = []
    for g in range(pk["G"]):
        c0, c1 = pk["model_off"][g], pk["model_off"][g + 1]
        for i in range(L.shape[0]):
            terms.append(dr.logtrick([pk["logw"][c] + pk["scale"][g] * L[i][c] for c in range(c0, c1)]))
    t = np.array(terms)
    return bool((t < 0).all() or (t > 0).all())


def test_shapes_reach_every_bucket_pair():
    """dic_kernel<SP, SBP> has nine instances, SP the bucket of the largest cluster size of
    a call and SBP the bucket of SB.  SHAPES on its own and the edge sweep on its own reach
    all nine, a model of SHAPES has kMaxModelClusters clusters, and a ragged base set has
    a base that owns all SB states."""
    nine = {(a, b) for a in (4, 8, 16) for b in (4, 8, 16)}
    got = {(state_bucket(max(max(sz) for sz in sh[5])), state_bucket(sh[1])) for sh in SHAPES.values()}
    assert got == nine, sorted(nine - got)
    assert {(state_bucket(S), state_bucket(Sb)) for S in EDGE_S for Sb in EDGES} == nine
    assert max(len(sz) for sh in SHAPES.values() for sz in sh[5]) == 64
    for name, sh in SHAPES.items():
        if sh[4]:
            assert build(name)[0]["nstates"].max() == sh[1], name


# ----------------------------------------------------------------------------
# closed forms pin the restatement and the pair routine
# ----------------------------------------------------------------------------
def test_one_state_pair_is_T_times_E(dic, check_lib, vo):
    """K = S = Sb = d = 1: every log-sum-exp has one term, logA = logPi = 0, so
    L = T E with E = -1/2 (ln 2 pi + ln s2 + (sb2 + (mu - m)^2) / s2)."""
    T, mu, sb2, m, s2 = 7, 1.25, 0.75, -0.5, 2.0
    base = dict(nstates=np.array([1], np.int32), prior=np.ones((1, 1)), A=np.ones((1, 1, 1)),
                centres=np.full((1, 1, 1), mu), covars=np.full((1, 1, 1), sb2), covmode=0)
    mo = dict(prior=np.ones((1, 1)), A=np.ones((1, 1, 1)), centres=np.full((1, 1, 1), m),
              covars=np.full((1, 1, 1), s2))
    E = -0.5 * (math.log(2 * math.pi) + math.log(s2) + (sb2 + (mu - m) ** 2) / s2)
    pk = dic.pack_models([mo])
    L, rec = dr.host_pairs(check_lib, base, pk, T)
    assert rec == 0 and abs(L[0, 0] - T * E) < 1e-14 * abs(T * E)
    assert abs(dr.oracle_pairs(vo, base, [mo], T)[0, 0] - T * E) < 1e-14 * abs(T * E)
    # one cluster of weight 1, scale 2: LL = 2 T E
    pk["scale"][0] = 2.0
    assert abs(dr.host_mix(check_lib, L, pk)[0] - 2 * T * E) < 1e-14 * abs(2 * T * E)


def _struct(K, S, d, **over):
    """A myDIC.m struct whose every term is zero until a field is overridden."""
    hmm = [dict(N1=np.zeros(S), M=np.zeros((S, S)), N=np.zeros(S), prior=np.full(S, 1.0 / S),
                trans=np.full((S, S), 1.0 / S), pdf=[dict(mean=np.zeros(d), cov=np.eye(d))] * S,
                varpar=dict(alpha=np.ones(S), epsilon=np.ones((S, S)), beta=np.ones(S),
                            W=[np.eye(d)] * S, v=np.full(S, d + 1.0))) for _ in range(K)]
    out = dict(K=K, alpha=np.ones(K), omega=np.full(K, 1.0 / K), Nj=np.zeros(K), hmm=hmm,
               learn_hyps=dict(vbopt=dict(lambda0=1.0)))
    out.update(over)
    return out


def test_restatement_term_mu_and_term_omega_closed_forms():
    """With all counts zero only term_mu is left: P_d = 2 (-1/2 sum lambda0 / beta).
    At K = 1, term_omega = Nj (log 1 - (psi(a) - psi(a))) = 0 whatever Nj is."""
    h = _struct(2, 2, 2)
    h["learn_hyps"]["vbopt"]["lambda0"] = 0.5
    h["hmm"][0]["varpar"]["beta"] = np.array([1.0, 2.0])
    h["hmm"][1]["varpar"]["beta"] = np.array([4.0, 8.0])
    assert abs(dr.penalty(h) - (-(0.5 + 0.25 + 0.125 + 0.0625))) < 1e-15
    one = _struct(1, 1, 1, Nj=np.array([123.0]), alpha=np.array([3.7]))
    assert abs(dr.penalty(one) - (-1.0)) < 1e-15   # term_mu of one state alone


def test_restatement_two_clusters_by_hand():
    """K = 2, S = 1, d = 1.  alpha = (1, 2): psi(1) - psi(3) = -3/2, psi(2) - psi(3) = -1/2.
    S = 1: term_pi = term_eps = 0.  d = 1: term_W = N/2 (ln v - psi(v / 2) - ln 2), with
    psi(1) = -gamma (v = 2) and psi(2) = 1 - gamma (v = 4).  Likelihood: Kb = 1,
    Ni = 9, weights 1/2 each."""
    h = _struct(2, 1, 1, alpha=np.array([1.0, 2.0]), omega=np.array([1 / 3, 2 / 3]),
                Nj=np.array([3.0, 6.0]))
    h["learn_hyps"]["vbopt"]["lambda0"] = 2.0
    for i, (beta, v, n) in enumerate([(4.0, 2.0, 3.0), (8.0, 4.0, 6.0)]):
        vp = h["hmm"][i]["varpar"]
        vp["beta"], vp["v"], vp["W"] = np.array([beta]), np.array([v]), [np.array([[0.3 + i]])]
        h["hmm"][i]["N"], h["hmm"][i]["N1"], h["hmm"][i]["M"] = np.array([n]), np.array([1.0]), np.array([[n]])
        h["hmm"][i]["prior"], h["hmm"][i]["trans"] = np.ones(1), np.ones((1, 1))
    t_om = 3 * (math.log(1 / 3) + 1.5) + 6 * (math.log(2 / 3) + 0.5)
    t_mu = -0.5 * (2.0 / 4.0 + 2.0 / 8.0)
    t_W = 0.5 * 3 * EULER + 0.5 * 6 * (math.log(2) - 1 + EULER)
    P_d = 2 * (t_om + t_mu + t_W)
    a, b = -1.0, -1.5
    LL = math.log(0.5 * math.exp(9 * a) + 0.5 * math.exp(9 * b))
    got_P, got_D = dr.my_dic(h, [[a, b]], T=5)
    assert abs(got_P - P_d) < 1e-13 and abs(got_D - (2 * P_d - 2 * LL)) < 1e-12
    assert abs(dr.my_dic(h, [[a, b]], T=5, dt=1)[1] - (2 * P_d - 2 * LL / 5)) < 1e-12


# ----------------------------------------------------------------------------
# the host pair routine against the oracle
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_host_pairs_match_oracle(dic, check_lib, vo, name):
    base, models, T = build(name)
    pk = dic.pack_models(models)
    ref_L, ref_LL = oracle_LL(vo, base, models, pk, T)
    L, rec = dr.host_pairs(check_lib, base, pk, T)
    print(name, "pairs err", elem_err(L, ref_L), "recomputed", rec)
    assert np.isfinite(ref_L).all() and one_sign(ref_L, pk)
    assert elem_err(L, ref_L) < RTOL_PAIRS
    Lx, _ = dr.host_pairs(check_lib, base, pk, T, exact_only=True)   # reference order throughout
    assert elem_err(Lx, ref_L) < RTOL_PAIRS
    # LL: the LSE terms of a subject all have one sign here, so the sum keeps the bound
    LL = dr.host_mix(check_lib, L, pk)
    assert elem_err(LL, ref_LL) < RTOL_PAIRS


def underflow_case():
    """Cluster means 40 standard deviations apart, bases sitting on one of them, and a
    transition row that gives the state the evidence favours a probability of 1e-250:
    Z = 1e-250 * 1 + 1 * exp(-800) lies below 1e-200."""
    base = dict(nstates=np.array([2, 2], np.int32), prior=np.array([[0.6, 0.4], [0.3, 0.7]]),
                A=np.array([[[0.7, 0.3], [0.2, 0.8]], [[0.5, 0.5], [0.9, 0.1]]]),
                centres=np.array([[[0.0], [0.1]], [[40.0], [39.9]]]),
                covars=np.full((2, 2, 1), 1.0), covmode=0)
    A = np.array([[[1e-250, 1.0 - 1e-250], [0.5, 0.5]], [[0.4, 0.6], [1.0 - 1e-250, 1e-250]]])
    mo = dict(prior=np.array([[0.5, 0.5], [0.5, 0.5]]), A=A, centres=np.array([[[0.0], [40.0]]] * 2),
              covars=np.ones((2, 2, 1)), omega=np.array([0.5, 0.5]), scale=1.0)
    return base, [mo], 4


def test_underflow_pair_is_recomputed_in_reference_order(dic, check_lib, vo):
    base, models, T = underflow_case()
    pk = dic.pack_models(models)
    ref_L = dr.oracle_pairs(vo, base, models, T)
    L, rec = dr.host_pairs(check_lib, base, pk, T)
    print("underflow L", L.tolist(), "oracle", ref_L.tolist(), "recomputed", rec)
    assert rec >= 1, "the case does not reach the recompute path"
    assert np.isfinite(L).all() and elem_err(L, ref_L) < RTOL_PAIRS


# (Sb, N, the two bases that underflow): SBP = 4, 8 and 16.  The second base of a row lies in
# the second tile (67), in the second sub-tile (37: 32 bases a pass at SBP = 8; 21: 16 a pass
# at SBP = 16); base 3 at SBP = 16 sits in lanes 48..63 of its wave.
MIXED_WAVE = [(2, 70, (2, 67)), (5, 70, (2, 37)), (9, 40, (3, 21))]
# Seeds of the base sets, per Sb: the first from Sb on under which the conditions of
# mixed_wave_refs hold for both named bases, each in the cluster column of its own redo.
MIXED_WAVE_SEED = {2: 2, 5: 7, 9: 31}


def mixed_wave_case(Sb, N, positions):
    """underflow_case()'s model against N ordinary one-dimensional bases (random A and prior,
    centres in [10, 30] between the model's means at 0 and 40, variance 1), and against a
    copy in which the two bases at `positions` sit on one of the means, as underflow_case()'s
    do.  Returns (plain base set, modified base set, models, T)."""
    rng = np.random.default_rng(MIXED_WAVE_SEED[Sb])
    plain = dict(nstates=np.full(N, Sb, np.int32), prior=rng.dirichlet(np.ones(Sb), size=N),
                 A=rng.dirichlet(np.ones(Sb), size=(N, Sb)), centres=rng.uniform(10.0, 30.0, (N, Sb, 1)),
                 covars=np.ones((N, Sb, 1)), covmode=0)
    mod = dict(plain, centres=plain["centres"].copy())
    mod["centres"][positions[0], :, 0] = 0.1 * np.arange(Sb)
    mod["centres"][positions[1], :, 0] = 40.0 - 0.1 * np.arange(Sb)
    _, models, T = underflow_case()
    return plain, mod, models, T


def redo_columns(dic, check_lib, base, mo, T, p):
    """The clusters of model `mo` against which base p is recomputed in reference order:
    the host build on that base alone, one cluster at a time."""
    one = {k: (v[p:p + 1] if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    cols = []
    for c in range(np.asarray(mo["prior"]).shape[0]):
        pkc = dic.pack_models([{k: np.asarray(mo[k])[c:c + 1] for k in ("prior", "A", "centres", "covars")}])
        if dr.host_pairs(check_lib, one, pkc, T)[1]:
            cols.append(c)
    return cols


def mixed_wave_refs(dic, check_lib, vo, Sb, N, positions):
    """The references of a mixed-wave case, and the conditions without which it would not
    tell a redo of the two pairs' lanes from a redo of their whole waves.  Exactly the two
    named bases are recomputed, each against one cluster, and the oracle is finite.  The
    kernel runs the reference-order sweep only for that cluster, so in the wave of each
    named base (64 / SBP consecutive bases) an ordinary base must have, in that cluster's
    column, a reference-order L that differs in bits from its factorised L."""
    plain, mod, models, T = mixed_wave_case(Sb, N, positions)
    pk = dic.pack_models(models)
    ref_L, ref_LL = oracle_LL(vo, mod, models, pk, T)
    assert np.isfinite(ref_L).all() and one_sign(ref_L, pk)
    host_L, rec = dr.host_pairs(check_lib, mod, pk, T)
    plain_L, rec_plain = dr.host_pairs(check_lib, plain, pk, T)
    assert rec == 2 and rec_plain == 0, (rec, rec_plain)
    exact_plain, _ = dr.host_pairs(check_lib, plain, pk, T, exact_only=True)
    per_wave = 64 // state_bucket(Sb)
    differs = exact_plain != plain_L
    for p in positions:
        cols = redo_columns(dic, check_lib, mod, models[0], T, p)
        assert len(cols) == 1, (p, cols)
        mates = [q for q in range(N) if q // per_wave == p // per_wave and q not in positions]
        assert differs[mates, cols[0]].any(), (p, cols, mates)
    exact_mod, _ = dr.host_pairs(check_lib, mod, pk, T, exact_only=True)
    return plain, mod, pk, T, ref_L, ref_LL, host_L, exact_mod


@pytest.mark.parametrize("Sb,N,positions", MIXED_WAVE)
def test_mixed_wave_case_is_sensitive(dic, check_lib, vo, Sb, N, positions):
    _, _, _, _, ref_L, _, host_L, exact_mod = mixed_wave_refs(dic, check_lib, vo, Sb, N, positions)
    print("mixed wave", Sb, "host vs oracle", elem_err(host_L, ref_L), "exact", elem_err(exact_mod, ref_L))
    assert elem_err(host_L, ref_L) < RTOL_PAIRS and elem_err(exact_mod, ref_L) < RTOL_PAIRS


def many_tiles_case(N=16385):
    """One-state, one-dimensional bases, T = 2, and two models (K = 1, S = 1; K = 2, S = 2
    with unequal weights): the smallest shape at which dic_reduce_kernel's lanes add more
    than one tile each (N > 256 tiles of 64)."""
    rng = np.random.default_rng(16385)
    base = dict(nstates=np.ones(N, np.int32), prior=np.ones((N, 1)), A=np.ones((N, 1, 1)),
                centres=rng.uniform(0.0, 5.0, (N, 1, 1)), covars=rng.uniform(0.5, 1.5, (N, 1, 1)), covmode=0)
    models = [dict(make_reduced(1, 1, 1, 0, seed=600), scale=1.3),
              dict(make_reduced(2, 2, 1, 0, seed=601), omega=np.array([0.3, 0.7]), scale=0.8)]
    return base, models, 2


def test_many_tiles_case_host_matches_oracle(dic, check_lib, vo):
    base, models, T = many_tiles_case()
    pk = dic.pack_models(models)
    ref_L, ref_LL = oracle_LL(vo, base, models, pk, T)
    L, rec = dr.host_pairs(check_lib, base, pk, T)
    assert rec == 0 and np.isfinite(ref_L).all() and one_sign(ref_L, pk)
    assert elem_err(L, ref_L) < RTOL_PAIRS
    assert elem_err(dr.host_mix(check_lib, L, pk), ref_LL) < RTOL_PAIRS


def test_nan_constant_reaches_only_its_pairs(dic, check_lib):
    base, models, T = build("mixed_sizes")
    pk = dic.pack_models(models)
    good, _ = dr.host_pairs(check_lib, base, pk, T)
    pk["m"][1, 0, 0] = np.nan
    L, _ = dr.host_pairs(check_lib, base, pk, T)
    assert np.isnan(L[:, 1]).all()
    keep = [c for c in range(pk["C"]) if c != 1]
    assert np.array_equal(L[:, keep], good[:, keep])


# ----------------------------------------------------------------------------
# my_dic / dic_grid on a stand-in engine
# ----------------------------------------------------------------------------
def fake_fit(vb, K, S, d, seed, omega=None):
    """An EM result with made-up counts: make_case's perturbed posterior (full W, as
    vbhem_h3m_cluster fits), its point estimates, positive statistics."""
    cs = make_case(6, K, S, 2, d, 1, seed=seed)
    P = cs["P"]
    rng = np.random.default_rng(seed)
    point = vb.host.convert_to_point(P, 1)
    if omega is not None:
        point["omega"] = np.asarray(omega, dtype=np.float64)
    syn = dict(Nj_rho1=rng.uniform(0.1, 3.0, (K, S)), Nj_rho2rho=rng.uniform(0.1, 9.0, (K, S, S)),
               Nj_rho=rng.uniform(0.5, 20.0, (K, S)))
    res = types.SimpleNamespace(post=P, syn=syn, Nj=rng.uniform(1.0, 8.0, K), point=point)
    return dict(result=res, hyp=None, K=K, S=S)


def subject_hmms(n, d, seed, empty=()):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i in empty:
            out.append(None)
            continue
        s = 1 + i % 3
        out.append(dict(prior=rng.dirichlet(np.ones(s)), trans=rng.dirichlet(np.ones(s), size=s),
                        pdf=[dict(mean=rng.uniform(0, 5, d), cov=np.diag(rng.uniform(0.5, 1.5, d)))
                             for _ in range(s)]))
    return out


def standin(vo, dic):
    """loglik(base, models, T) from the oracle's L and loops."""
    def fn(base, models, T):
        pk = dic.pack_models(models)
        L = dr.oracle_pairs(vo, base.numpy(), [dict(m, covars=m["covars"]) for m in models], T)
        return dr.mix(L, pk["model_off"], pk["logw"], pk["scale"])
    return fn


def ref_dic(vo, dic, vb, hmms, fit, T, dt, lambda0):
    from vbhem_amd import vhem
    base = vhem.hmms_to_h3m(hmms, "diag").numpy()
    pt = fit["result"].point
    cov = np.diagonal(pt["covars"], axis1=-2, axis2=-1)
    mo = dict(prior=pt["prior"], A=pt["A"], centres=pt["centres"], covars=cov)
    L = dr.oracle_pairs(vo, base, [mo], T)
    h = dr.fit_struct(fit["result"], fit["hyp"] or dict(vbopt=dict(lambda0=lambda0)))
    return dr.my_dic(h, L.tolist(), T, dt)


@pytest.mark.parametrize("dt", [0, 1])
def test_my_dic_equals_restatement(dic, vb, vo, dt):
    hmms = subject_hmms(7, 2, 3, empty=(2,))        # one empty entry stays in Kb
    fit = fake_fit(vb, 3, 2, 2, seed=11)
    T = 6
    P_d, D = dic.my_dic(hmms, fit, T, dt=dt, lambda0=0.7, loglik=standin(vo, dic))
    rP, rD = ref_dic(vo, dic, vb, hmms, fit, T, dt, 0.7)
    assert abs(P_d - rP) <= 1e-12 * abs(rP) and abs(D - rD) <= 1e-12 * abs(rD)
    # the learned lambda0 wins over the argument
    fit2 = dict(fit, hyp=dict(vbopt=dict(lambda0=0.2)))
    P2, _ = dic.my_dic(hmms, fit2, T, dt=dt, lambda0=0.7, loglik=standin(vo, dic))
    assert abs(P2 - ref_dic(vo, dic, vb, hmms, fit2, T, dt, None)[0]) <= 1e-12 * abs(P2)
    assert P2 != P_d


def test_my_dic_uses_uniform_weights_not_omega(dic, vb, vo):
    """myDIC.m:160,169 mixes with hmms_to_h3m(h3m.hmm).omega = 1 / K; term_omega alone
    reads the fit's omega.  A fit with omega = (0.98, 0.02) must follow the restatement
    and stay away from the omega-weighted value."""
    hmms = subject_hmms(6, 2, 5)
    fit = fake_fit(vb, 2, 2, 2, seed=12, omega=[0.98, 0.02])
    T = 5
    P_d, D = dic.my_dic(hmms, fit, T, lambda0=1.0, loglik=standin(vo, dic))
    rP, rD = ref_dic(vo, dic, vb, hmms, fit, T, 0, 1.0)
    assert abs(D - rD) <= 1e-12 * abs(rD)
    base = dic._as_base(hmms)
    mo = dict(dic.dic_model(fit, base.N))
    mo["logw"] = np.log(np.array([0.98, 0.02]))
    weighted = 2 * P_d - 2 * standin(vo, dic)(base, [mo], T)[0]
    assert abs(weighted - D) > 1e-3 * abs(D)


def test_my_dic_missing_lambda0_raises(dic, vb, vo):
    with pytest.raises(ValueError, match="lambda0"):
        dic.my_dic(subject_hmms(4, 2, 1), fake_fit(vb, 2, 2, 2, seed=13), 5, loglik=standin(vo, dic))


def test_dic_grid_cells_and_argmin(dic, vb, vo):
    """Cell (k, s) of the result is model (K[k], S[s]): every cell has its own fit."""
    Ks, Ss = [1, 2, 3], [1, 2]
    hmms = subject_hmms(6, 2, 7)
    cells = [[fake_fit(vb, K, S, 2, seed=20 + 3 * K + S) for S in Ss] for K in Ks]
    clustered = dict(model_all=[dict(cells[k][0], model_all_s=cells[k]) for k in range(len(Ks))])
    T = 4
    calls = []
    inner = standin(vo, dic)

    def counting(base, models, T_):
        calls.append(len(models))
        return inner(base, models, T_)
    out = dic.dic_grid(hmms, clustered, T, lambda0=0.9, loglik=counting)
    assert calls == [len(Ks) * len(Ss)]             # every cell in one likelihood call
    assert out["DIC"].shape == (3, 2) and out["K"] == Ks and out["S"] == Ss
    for k in range(len(Ks)):
        for s in range(len(Ss)):
            rP, rD = ref_dic(vo, dic, vb, hmms, cells[k][s], T, 0, 0.9)
            assert abs(out["P_d"][k, s] - rP) <= 1e-12 * abs(rP)
            assert abs(out["DIC"][k, s] - rD) <= 1e-12 * abs(rD)
    assert out["argmin"] == tuple(int(x) for x in np.unravel_index(np.argmin(out["DIC"]), (3, 2)))


# ----------------------------------------------------------------------------
# BIC / AIC, vbh3m_remove_empty
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("div_T", [0, 1])
def test_vhem_bic_aic_equal_restatement(dic, div_T):
    rng = np.random.default_rng(4)
    Ks, Ss, dim, Kb = [1, 2, 4], [2, 3], 2, 9
    grid = []
    for K in Ks:
        row = []
        for S in Ss:
            Z = rng.dirichlet(np.ones(K), size=Kb)
            row.append(dict(Z=Z, L_elbo1=-rng.uniform(1, 30, (Kb, K)), hemopt=dict(Nv=50, tau=7)))
        grid.append(row)
    lists = [[dict(c, Z=c["Z"].tolist(), L_elbo1=c["L_elbo1"].tolist()) for c in row] for row in grid]
    for fn, ref in ((dic.vhem_bic, dr.vhem_bic), (dic.vhem_aic, dr.vhem_aic)):
        got, want = fn(grid, Ks, Ss, dim, div_T), np.array(ref(lists, Ks, Ss, dim, div_T))
        assert got.shape == (3, 2) and np.max(np.abs(got - want) / np.abs(want)) < 1e-12
    # K = S = 1, one subject, Z = 1: log_ests = Nv L, BIC = log(Nv T) 2 dim - 2 Nv L
    one = [[dict(Z=np.ones((1, 1)), L_elbo1=np.array([[-2.0]]), hemopt=dict(Nv=10, tau=5))]]
    assert abs(dic.vhem_bic(one, 1, 1, 2)[0, 0] - (math.log(50) * 4 + 40)) < 1e-12
    assert abs(dic.vhem_aic(one, 1, 1, 2)[0, 0] - (2 * 4 + 40)) < 1e-12


def scripted_h3m():
    """Three clusters of three states: cluster 1 has Nj = 0.5 (below 1), state 1 of
    cluster 2 has N = 1e-4 (below 1e-3)."""
    rng = np.random.default_rng(8)
    hm = []
    for j in range(3):
        N = np.array([5.0, 1e-4 if j == 2 else 3.0, 4.0])
        eps = rng.uniform(0.5, 4.0, (3, 3))
        al = rng.uniform(0.5, 4.0, 3)
        hm.append(dict(prior=al / al.sum(), trans=eps / eps.sum(1, keepdims=True),
                       pdf=[dict(mean=np.array([10.0 * j + s, 0.0]), cov=np.eye(2)) for s in range(3)],
                       N=N, N1=rng.uniform(0.1, 1, 3), M=rng.uniform(0.1, 3, (3, 3)),
                       varpar=dict(alpha=al, epsilon=eps, beta=rng.uniform(1, 2, 3), v=rng.uniform(4, 6, 3),
                                   m=rng.normal(size=(3, 2)), W=np.stack([np.eye(2)] * 3))))
    label = np.array([0, 2, 2, 0, 1, 2])
    return dict(hmm=hm, omega=np.array([0.5, 0.1, 0.4]), Z=rng.dirichlet(np.ones(3), size=6),
                L_elbo=-rng.uniform(1, 9, (6, 3)), Nj=np.array([2.5, 0.5, 3.0]), label=label,
                groups=[np.flatnonzero(label == j) for j in range(3)], group_size=np.array([2, 1, 3]), K=3)


def test_vbh3m_remove_empty_scripted(dic):
    h = scripted_h3m()
    out, empty = dic.vbh3m_remove_empty(h)
    as_lists = dict(h, hmm=[dict(g, varpar={k: np.asarray(v).tolist() for k, v in g["varpar"].items()},
                                 N=g["N"].tolist(), N1=g["N1"].tolist(), M=g["M"].tolist(),
                                 prior=g["prior"].tolist(), trans=g["trans"].tolist()) for g in h["hmm"]],
                    omega=h["omega"].tolist(), Z=h["Z"].tolist(), L_elbo=h["L_elbo"].tolist(),
                    Nj=h["Nj"].tolist(), label=h["label"].tolist(), group_size=h["group_size"].tolist())
    ref, rz, kept = dr.vbh3m_remove_empty(as_lists)
    assert list(empty) == rz == [1]
    assert np.allclose(out["omega"], ref["omega"], rtol=1e-15) and abs(out["omega"].sum() - 1) < 1e-15
    assert np.array_equal(out["Z"], np.array(ref["Z"])) and np.array_equal(out["L_elbo"], np.array(ref["L_elbo"]))
    assert out["Nj"].tolist() == ref["Nj"] == [2.5, 3.0]
    # labels: 0 stays, 2 -> 1; the subject of the removed cluster keeps its old number (1)
    assert out["label"].tolist() == ref["label"] == [0, 1, 1, 0, 1, 1]
    assert [g.tolist() for g in out["groups"]] == [[0, 3], [1, 2, 5]] and out["group_size"].tolist() == [2, 3]
    assert len(out["hmm"]) == 2 and [len(g["prior"]) for g in out["hmm"]] == [3, 2]
    for g, src, order in zip(out["hmm"], (h["hmm"][0], h["hmm"][2]), kept):
        assert [p["mean"][0] for p in g["pdf"]] == [src["pdf"][k]["mean"][0] for k in order]
        assert abs(np.sum(g["prior"]) - 1) < 1e-15 and np.allclose(np.sum(g["trans"], 1), 1, rtol=1e-15)
        assert np.array_equal(g["N"], src["N"][order])
    assert 1 not in kept[1]                         # the state with N = 1e-4 is gone
    # nothing below the thresholds: only the reordering is left
    same, none = dic.vbh3m_remove_empty(dict(h, Nj=np.array([2.5, 1.0, 3.0])), thresh=1.0)
    assert len(none) == 0 and len(same["hmm"]) == 3


# ----------------------------------------------------------------------------
# the C ABI's host side
# ----------------------------------------------------------------------------
def test_workspace_does_not_scale_with_N_times_C(check_lib):
    """Nothing in the workspace is proportional to N * C: at N = 1e6, G = 30, C = 105 it
    is below 1 % of an [N][C] buffer, at the smallest and the largest state counts."""
    N, G, C = 10 ** 6, 30, 105
    for SB, S, d in ((3, 5, 2), (16, 16, 16)):
        nb = check_lib.diccheck_workspace_bytes(N, SB, d, 0, G, C, S, 6, 10)
        assert 0 < nb < 0.01 * N * C * 8, (SB, S, d, nb)


def test_workspace_refuses_unsupported_shapes(check_lib):
    assert check_lib.diccheck_workspace_bytes(10, 3, 2, 0, 2, 4, 17, 2, 5) == 0    # S = 17
    assert check_lib.diccheck_workspace_bytes(10, 17, 2, 0, 2, 4, 3, 2, 5) == 0    # SB = 17
    assert check_lib.diccheck_workspace_bytes(10, 3, 2, 1, 2, 4, 3, 2, 5) == 0     # full covariance
    assert check_lib.diccheck_workspace_bytes(10, 3, 2, 0, 2, 130, 3, 65, 5) == 0  # 65 clusters in a model
    assert check_lib.diccheck_workspace_bytes(10, 3, 2, 0, 2, 4, 3, 2, 5) > 0
