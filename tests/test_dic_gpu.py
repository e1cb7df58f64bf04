"""The DIC likelihood on the GPU (vbhmm_dic_loglik, csrc/vbhmm_dic.hip): per-pair values
and per-model sums against the host build of the same pair routine and the oracle, the
kernel's tile, wave and sub-tile edges in every (cluster-state, base-state) bucket pair,
the reference-order redo in waves that also hold ordinary pairs, the reduction over more
than 256 tiles, a ragged grid, position independence bit for bit, NaN containment, the
unsupported shapes and their fallback, both engines of vbhem_amd.dic.loglik_grid, and the
planted end-to-end run.

Every parity bound is RTOL_PAIRS = 1e-10 (elem_err).  Largest errors seen on an MI355X,
device against the oracle unless another reference is named:
  test_pairs_and_sums_match_host_and_oracle, L: S8_Sb8 3.6e-16, S5_Sb9 4.4e-16, S9_Sb3 2.1e-16,
      S16_Sb5 2.6e-16, d16_S3 5.8e-16, K64 4.4e-16, S3_Sb5 2.0e-16, S3_Sb9 2.0e-16; LL <= 1.9e-16
  test_tile_and_wave_edges_larger_clusters, L against the host build (its reference):
      4.1e-16 (SB 3, S 6) the largest of the six
  test_redo_takes_only_the_underflowing_pairs: L 4.2e-16, LL 1.8e-16 (SB 9); the redone rows
      against the host build in reference order 2.0e-16 (SB 9); the other rows bit-identical
  test_reduce_over_more_than_256_tiles: L 4.5e-16, LL 1.7e-15 at both N (16384 terms added
      per lane and then in lane order, against the oracle's sum in index order)
  test_unsupported_shapes_and_fallback, 65 clusters through the pairs engine: LL 1.5e-16"""
import numpy as np
import pytest

import dic_ref as dr
from cases import make_case, make_reduced
from conftest import RTOL_PAIRS, elem_err
from test_dic import (EDGE_S, EDGES, MIXED_WAVE, SHAPES, build, many_tiles_case, mixed_wave_refs, one_sign,
                      oracle_LL, underflow_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dic(vb):
    from vbhem_amd import dic as mod
    return mod


@pytest.fixture(scope="module")
def check_lib(capi_lib):
    return dr.load_diccheck()


@pytest.mark.parametrize("name", list(SHAPES) + ["underflow"])
def test_pairs_and_sums_match_host_and_oracle(dic, check_lib, vo, name):
    base, models, T = underflow_case() if name == "underflow" else build(name)
    pk = dic.pack_models(models)
    ref_L, ref_LL = oracle_LL(vo, base, models, pk, T)
    host_L, rec = dr.host_pairs(check_lib, base, pk, T)
    rc, LL, L = dr.device_loglik(check_lib, base, pk, T)
    assert rc == 0
    print(name, "L vs oracle", elem_err(L, ref_L), "vs host", elem_err(L, host_L), "LL", elem_err(LL, ref_LL),
          "host recomputed", rec)
    assert one_sign(ref_L, pk)
    assert elem_err(L, ref_L) < RTOL_PAIRS and elem_err(L, host_L) < RTOL_PAIRS
    assert elem_err(LL, ref_LL) < RTOL_PAIRS
    assert elem_err(LL, dr.host_mix(check_lib, host_L, pk)) < RTOL_PAIRS
    # without the per-pair output the sums are the same bits
    rc2, LL2, _ = dr.device_loglik(check_lib, base, pk, T, want_pairs=False)
    assert rc2 == 0 and np.array_equal(LL, LL2)


# EDGES (test_dic.py): N on both sides of a wave, a pass of the workgroup and a tile, per SB.
@pytest.fixture(scope="module")
def edge_refs(dic, check_lib):
    """Per (SB, S): a base set of the largest N, two models (1 cluster of S - 1 states; 3
    clusters of S, one more than the two block buffers hold) and the host build's L for all
    of it, computed once.  S = 3, 6 and 11 are the cluster-state buckets 4, 8 and 16."""
    out = {}
    for Sb, Ns in EDGES.items():
        base = make_case(max(Ns), 2, 3, Sb, 2, 0, seed=300 + Sb, ragged=True, tau=3)["base"]
        assert base["nstates"].max() == Sb
        for S in EDGE_S:
            seed = Sb if S == 3 else Sb + 100 * S
            models = [dict(make_reduced(1, S - 1, 2, 0, seed=310 + seed), scale=1.5),
                      dict(make_reduced(3, S, 2, 0, seed=320 + seed), omega=np.array([0.2, 0.5, 0.3]), scale=0.7)]
            pk = dic.pack_models(models)
            out[Sb, S] = (base, pk, dr.host_pairs(check_lib, base, pk, 3)[0])
    return out


def sweep_edges(check_lib, edge_refs, Sb, S):
    base, pk, host_L = edge_refs[Sb, S]
    worst = 0.0
    for N in EDGES[Sb]:
        sub = {k: (v[:N] if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        rc, LL, L = dr.device_loglik(check_lib, sub, pk, 3)
        assert rc == 0, N
        worst = max(worst, elem_err(L, host_L[:N]))
        assert elem_err(L, host_L[:N]) < RTOL_PAIRS, N
        assert elem_err(LL, dr.host_mix(check_lib, host_L[:N], pk)) < RTOL_PAIRS, N
    print("edges Sb", Sb, "S", S, "L vs host", worst)


@pytest.mark.parametrize("Sb", list(EDGES))
def test_tile_and_wave_edges(check_lib, edge_refs, Sb):
    sweep_edges(check_lib, edge_refs, Sb, 3)


@pytest.mark.parametrize("S", EDGE_S[1:])
@pytest.mark.parametrize("Sb", list(EDGES))
def test_tile_and_wave_edges_larger_clusters(check_lib, edge_refs, Sb, S):
    """The same sweep in the cluster-state buckets 8 and 16: with SB = 3, 5 and 9 the
    instances (8, 4) ... (16, 16), every sub-tile count (1, 2, 4) at both register widths."""
    sweep_edges(check_lib, edge_refs, Sb, S)


@pytest.mark.parametrize("Sb,N,positions", MIXED_WAVE)
def test_redo_takes_only_the_underflowing_pairs(dic, check_lib, vo, Sb, N, positions):
    """Two underflowing bases among ordinary ones: the waves that hold them run the sweep
    again in reference order, and only the lanes of the two bases may take its result.
    mixed_wave_refs asserts, for each of the two and in the cluster column of its redo, that
    an ordinary base of its wave has other bits in reference order.  The device runs on the plain and on the modified set have the same N, so the
    same tiling: every other base's row of L must come out bit for bit the same."""
    plain, mod, pk, T, ref_L, ref_LL, host_L, exact_L = mixed_wave_refs(dic, check_lib, vo, Sb, N, positions)
    rc, LL, L = dr.device_loglik(check_lib, mod, pk, T)
    assert rc == 0
    rc0, _, L0 = dr.device_loglik(check_lib, plain, pk, T)
    assert rc0 == 0
    low = list(positions)
    print("mixed wave Sb", Sb, "L vs oracle", elem_err(L, ref_L), "vs host", elem_err(L, host_L), "LL",
          elem_err(LL, ref_LL), "redone rows vs reference order", elem_err(L[low], exact_L[low]))
    assert elem_err(L, ref_L) < RTOL_PAIRS and elem_err(L, host_L) < RTOL_PAIRS
    assert elem_err(LL, ref_LL) < RTOL_PAIRS
    assert elem_err(LL, dr.host_mix(check_lib, host_L, pk)) < RTOL_PAIRS
    others = [i for i in range(N) if i not in positions]
    assert np.array_equal(L[others], L0[others])
    assert elem_err(L[low], exact_L[low]) < RTOL_PAIRS


@pytest.fixture(scope="module")
def many_tiles_ref(dic, check_lib, vo):
    base, models, T = many_tiles_case()
    pk = dic.pack_models(models)
    ref_L, _ = oracle_LL(vo, base, models, pk, T)
    return base, models, T, pk, ref_L, dr.host_pairs(check_lib, base, pk, T)[0]


@pytest.mark.parametrize("N", [16384, 16385])
def test_reduce_over_more_than_256_tiles(check_lib, many_tiles_ref, N):
    """256 and 257 tiles: at 257 lane 0 of dic_reduce_kernel adds a second partial."""
    base, models, T, pk, ref_L, host_L = many_tiles_ref
    ref_L, host_L = ref_L[:N], host_L[:N]
    ref_LL = dr.mix(ref_L, pk["model_off"], pk["logw"], pk["scale"])
    assert one_sign(ref_L, pk)
    sub = {k: (v[:N] if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    rc, LL, L = dr.device_loglik(check_lib, sub, pk, T)
    assert rc == 0
    rows = np.unique(np.concatenate([[0, 63, 64, 8191, 8192, 16383, N - 1],
                                     np.random.default_rng(N).integers(0, N, 200)]))
    print("N", N, "L vs oracle", elem_err(L[rows], ref_L[rows]), "vs host", elem_err(L[rows], host_L[rows]),
          "LL vs oracle", elem_err(LL, ref_LL))
    assert elem_err(L[rows], ref_L[rows]) < RTOL_PAIRS and elem_err(L[rows], host_L[rows]) < RTOL_PAIRS
    assert elem_err(LL, ref_LL) < RTOL_PAIRS
    assert elem_err(LL, dr.host_mix(check_lib, host_L, pk)) < RTOL_PAIRS


def ragged_grid(seed=0):
    """Six models, K in {1, 2, 3} x S in {1, 3}; the (3, 3) model mixes cluster sizes
    3, 1, 2 and one of its clusters has weight 0 (logw = -inf)."""
    base = make_case(70, 2, 3, 3, 2, 0, seed=400 + seed, ragged=True, tau=5)["base"]
    models = []
    for K in (1, 2, 3):
        for S in (1, 3):
            red = make_reduced(K, S, 2, 0, seed=410 + seed + 10 * K + S)
            rng = np.random.default_rng(K * 7 + S)
            mo = dict(red, omega=rng.dirichlet(np.ones(K)), scale=float(rng.uniform(0.5, 2.0)))
            if (K, S) == (3, 3):
                mo["nstates"] = np.array([3, 1, 2])
                for j, n in enumerate(mo["nstates"]):
                    mo["A"][j, :n, :n] /= mo["A"][j, :n, :n].sum(-1, keepdims=True)
                    mo["prior"][j, :n] /= mo["prior"][j, :n].sum()
                mo["omega"] = np.array([0.6, 0.0, 0.4])
            models.append(mo)
    return base, models, 5


@pytest.fixture(scope="module")
def ragged_ref(dic, vo):
    base, models, T = ragged_grid()
    pk = dic.pack_models(models)
    L, LL = oracle_LL(vo, base, models, pk, T)
    return base, models, T, pk, L, LL


def test_ragged_grid(check_lib, ragged_ref):
    base, models, T, pk, ref_L, ref_LL = ragged_ref
    assert np.isneginf(pk["logw"]).sum() == 1 and one_sign(ref_L, pk)
    rc, LL, L = dr.device_loglik(check_lib, base, pk, T)
    assert rc == 0
    assert elem_err(L, ref_L) < RTOL_PAIRS and elem_err(LL, ref_LL) < RTOL_PAIRS


def test_position_independence_bit_for_bit(dic, check_lib, ragged_ref):
    base, models, T, pk, _, _ = ragged_ref
    _, whole, _ = dr.device_loglik(check_lib, base, pk, T, want_pairs=False)
    order = [4, 0, 5, 2, 1, 3]
    _, shuffled, _ = dr.device_loglik(check_lib, base, dic.pack_models([models[g] for g in order]), T,
                                      want_pairs=False)
    assert np.array_equal(shuffled, whole[order])
    for g in range(len(models)):
        others = [h for h in range(len(models)) if h != g]
        for grid, at in (([g], 0), ([g] + others, 0), (others + [g], len(others))):
            rc, LL, _ = dr.device_loglik(check_lib, base, dic.pack_models([models[h] for h in grid]), T,
                                         want_pairs=False)
            assert rc == 0 and LL[at] == whole[g], (g, len(grid), at)


def test_nan_in_one_model_stays_there(dic, check_lib, ragged_ref):
    base, models, T, pk, _, _ = ragged_ref
    _, whole, _ = dr.device_loglik(check_lib, base, pk, T, want_pairs=False)
    for field in ("m", "logA", "c"):
        bad = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in pk.items()}
        c = int(pk["model_off"][3])                 # a cluster of model 3 (K = 2, S = 3)
        bad[field][(c, 0, 0) if field != "c" else (c, 0)] = np.nan
        rc, LL, L = dr.device_loglik(check_lib, base, bad, T)
        assert rc == 0
        assert np.isnan(LL[3]) and np.isnan(L[:, c]).all(), field
        keep = [g for g in range(pk["G"]) if g != 3]
        assert np.array_equal(LL[keep], whole[keep]), field


def test_unsupported_shapes_and_fallback(dic, check_lib, vo):
    base = make_case(5, 2, 3, 3, 2, 0, seed=500, tau=4)["base"]
    big = [dict(make_reduced(2, 17, 2, 0, seed=501), scale=1.0)]
    rc, _, _ = dr.device_loglik(check_lib, base, dic.pack_models(big), 4)
    assert rc == -2                                  # VBHEM_ERR_UNSUPPORTED: S = 17
    full = dict(base, covars=np.stack([np.stack([np.diag(v) for v in b]) for b in base["covars"]]))
    small = [dict(make_reduced(2, 3, 2, 0, seed=502), scale=1.0)]
    rc, _, _ = dr.device_loglik(check_lib, full, dic.pack_models(small), 4, covmode=1)
    assert rc == -2                                  # full covariance
    from vbhem_amd.h3m import BaseSet
    bs = BaseSet.from_numpy(dict(base, omega=np.full(5, 0.2)))
    got = dic.loglik_grid(bs, big, 4, "cuda:0").cpu().numpy()          # falls back to the pairs loop
    want = dic.loglik_grid(bs, big, 4, "cuda:0", engine="pairs").cpu().numpy()
    assert elem_err(got, want) < RTOL_PAIRS and np.isfinite(got).all()
    # one cluster more than val[kMaxModelClusters][.] holds, beside a model the kernel takes
    many = [dict(make_reduced(65, 2, 2, 0, seed=503), scale=1.0), small[0]]
    rc, _, _ = dr.device_loglik(check_lib, base, dic.pack_models(many), 4)
    assert rc == -2                                  # 65 clusters in a model
    got = dic.loglik_grid(bs, many, 4, "cuda:0").cpu().numpy()
    want = dic.loglik_grid(bs, many, 4, "cuda:0", engine="pairs").cpu().numpy()
    pk = dic.pack_models(many)
    ref_L, ref_LL = oracle_LL(vo, base, many, pk, 4)
    print("65 clusters: fallback vs pairs engine", elem_err(got, want), "vs oracle", elem_err(got, ref_LL))
    assert elem_err(got, want) < RTOL_PAIRS and np.isfinite(got).all()
    assert one_sign(ref_L, pk) and elem_err(got, ref_LL) < RTOL_PAIRS
    wide = make_case(5, 2, 3, 3, 17, 0, seed=504, tau=4)["base"]
    rc, _, _ = dr.device_loglik(check_lib, wide, dic.pack_models([dict(make_reduced(2, 3, 17, 0, seed=505))]), 4)
    assert rc == -2                                  # d = 17


def test_fused_equals_pairs_engine(dic, ragged_ref):
    from vbhem_amd.h3m import BaseSet
    base, models, T, pk, ref_L, ref_LL = ragged_ref
    bs = BaseSet.from_numpy(dict(base, omega=np.full(base["prior"].shape[0], 1.0)))
    f_LL, f_L = dic.loglik_grid(bs, models, T, "cuda:0", return_pairs=True)
    p_LL, p_L = dic.loglik_grid(bs, models, T, "cuda:0", engine="pairs", return_pairs=True)
    assert elem_err(f_L.cpu().numpy(), p_L.cpu().numpy()) < RTOL_PAIRS
    assert elem_err(f_LL.cpu().numpy(), p_LL.cpu().numpy()) < RTOL_PAIRS
    assert elem_err(f_LL.cpu().numpy(), ref_LL) < RTOL_PAIRS


def test_planted_end_to_end(dic, vb, vo):
    """planted_hmms(20) -> vbhem_h3m_cluster over K = 1:3, S = 1:3 -> dic_grid: finite and
    equal to the restatement fed the same fits and the oracle's L.  P_d is host math
    (1e-12); LL is held to RTOL_PAIRS, so |dDIC| <= 2 RTOL_PAIRS |LL| + 2e-12 |P_d|."""
    from vbhem_amd import cluster, vhem
    hmms, _ = vhem.planted_hmms(20, seed=3)
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20,
               Nv=100, seed=1001, trials=4, max_iter=30, minDiff=1e-5, learn_hyps=0, initmode="baseem")
    res = cluster.vbhem_h3m_cluster(None, [1, 2, 3], [1, 2, 3], opt, device="cuda:0",
                                    base=vhem.hmms_to_h3m(hmms, "full"))
    out = dic.dic_grid(hmms, res, 20, lambda0=opt["lambda0"], device="cuda:0")
    print("planted DIC grid\n", out["DIC"], "\nP_d\n", out["P_d"], "\nargmin", out["argmin"])
    assert out["DIC"].shape == (3, 3) and np.isfinite(out["DIC"]).all() and out["argmin"] is not None
    base = vhem.hmms_to_h3m(hmms, "diag").numpy()
    for k, row in enumerate(dic.grid_cells(res)):
        for s, fit in enumerate(row):
            pt = fit["result"].point
            mo = dict(prior=pt["prior"], A=pt["A"], centres=pt["centres"],
                      covars=np.diagonal(pt["covars"], axis1=-2, axis2=-1))
            L = dr.oracle_pairs(vo, base, [mo], 20)
            h = dr.fit_struct(fit["result"], dict(vbopt=dict(lambda0=opt["lambda0"])))
            rP, rD = dr.my_dic(h, L.tolist(), 20)
            LL = (2 * rP - rD) / 2
            assert abs(out["P_d"][k, s] - rP) <= 1e-12 * abs(rP)
            assert abs(out["DIC"][k, s] - rD) <= 2 * RTOL_PAIRS * abs(LL) + 2e-12 * abs(rP), (k, s)
