"""The Dunn index and the PPK log-likelihood on the GPU (vbhem_amd/evaluate.py over
score.kld_jobs): against the restatement (tests/dunn_ref.py) and against the same
values composed from score.vbhmm_kld calls at RTOL_PAIRS under conftest.stat_err, its
memory against the [H + K][N_total] matrix it must not build, and a CCFD run scored
end to end."""
import numpy as np
import pytest
import torch

import dunn_ref as dr
import ppk_ref as pr
import score_ref as sr
from conftest import RTOL_PAIRS, stat_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ev(vb, capi_lib):
    from vbhem_amd import evaluate
    return evaluate


@pytest.fixture(scope="module")
def score(vb, capi_lib):
    from vbhem_amd import score as mod
    return mod


def case_args(pooled):
    hmms, data, centres, groups, cs = dr.dunn_case()
    if pooled == "members":
        return centres, hmms, data, groups, None
    return [hmms[i] for i in cs], hmms, data, groups, cs


@pytest.mark.parametrize("pooled", ["members", "centre"])
def test_dunn_index_matches_restatement(ev, pooled):
    centres, hmms, data, groups, cs = case_args(pooled)
    ref = dr.dunn_reference(pooled)
    assert np.isfinite(ref["inter_vct"]).all() and all(np.isfinite(m).all() for m in ref["intra"])
    got = ev.dunn_index(centres, hmms, data, groups, pooled, cs, device=DEV)
    assert [len(m) for m in got["intra"]] == [1, 2, 4] and got["inter"].shape == (3, 3) and got["kept"] == [0, 1, 2]
    err = max(stat_err(np.concatenate(got["intra"]), np.concatenate(ref["intra"])),
              stat_err(got["inter"], ref["inter"]), stat_err(got["inter_vct"], ref["inter_vct"]),
              stat_err(got["DI"], ref["DI"]))
    print("dunn err", err)
    assert err < RTOL_PAIRS
    assert np.array_equal(got["inter_vct"], got["inter"][np.triu_indices(3, 1)]) and not np.tril(got["inter"]).any()
    assert got["DI"] == got["inter_vct"].min() / max(m.max() for m in got["intra"])


@pytest.mark.parametrize("pooled", ["members", "centre"])
def test_dunn_index_matches_composed_vbhmm_kld(ev, score, pooled):
    centres, hmms, data, groups, cs = case_args(pooled)
    got = ev.dunn_index(centres, hmms, data, groups, pooled, cs, device=DEV)
    cd = dr.cendata(data, groups, "vb" if pooled == "members" else "ccfd", cs)
    kld = lambda a, b, x: score.vbhmm_kld(a, b, list(x), device=DEV)[0]
    intra = [np.array([0.5 * (kld(c, hmms[i], cd[j]) + kld(hmms[i], c, data[i])) for i in groups[j]])
             for j, c in enumerate(centres)]
    vct = np.array([0.5 * (kld(centres[i], centres[j], cd[i]) + kld(centres[j], centres[i], cd[j]))
                    for i in range(3) for j in range(i + 1, 3)])
    err = max(stat_err(np.concatenate(got["intra"]), np.concatenate(intra)), stat_err(got["inter_vct"], vct))
    print("against vbhmm_kld", err)
    assert err < RTOL_PAIRS


def test_dropped_clusters(ev):
    """An empty cluster and a cluster without a centre leave the index of the others."""
    centres, hmms, data, groups, _ = case_args("members")
    full = ev.dunn_index(centres, hmms, data, groups, device=DEV)
    more = ev.dunn_index([centres[0], centres[1], None, centres[1], centres[2]], hmms, data,
                         [groups[0], np.zeros(0, dtype=np.int64), groups[1], groups[1], groups[2]], device=DEV)
    assert more["kept"] == [0, 3, 4] and more["DI"] == full["DI"]
    assert np.array_equal(more["inter"], full["inter"])


def test_memory(ev):
    """512 subjects of 8 trials, K = 4: the peak rise of the whole call stays below the
    [H + K][N_total] log-likelihood matrix of the ll_matrix route."""
    H, per, T, K = 512, 8, 5, 4
    rng = np.random.default_rng(9)
    hmms = [sr.make_hmm(rng, 3, 2, False) for _ in range(H)]
    centres = [sr.make_hmm(rng, 3, 2, False) for _ in range(K)]
    data = [[rng.uniform(0, 4, (T, 2)) for _ in range(per)] for _ in range(H)]
    groups = [np.arange(j, H, K) for j in range(K)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = ev.dunn_index(centres, hmms, data, groups, device=DEV)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = (H + K) * (H * per) * 8
    print("peak rise", rise, "bound", bound)
    assert rise < bound
    assert np.isfinite(got["DI"]) and [len(m) for m in got["intra"]] == [H // K] * K
    # one member's distance against the restatement
    j, q = 2, 17
    i = int(groups[j][q])
    pooled = [s for m in groups[j] for s in data[m]]
    ref = 0.5 * (dr.vbhmm_kld(centres[j], hmms[i], pooled) + dr.vbhmm_kld(hmms[i], centres[j], data[i]))
    assert stat_err(got["intra"][j][q], ref) < RTOL_PAIRS


def test_mixture_loglik_matches_restatement(ev):
    hmms, data, centres, _, _ = dr.dunn_case()
    w = np.array([0.2, 0.5, 0.3])
    ref = dr.ppk_loglik(centres, w, data)
    got = ev.mixture_loglik(centres, w, data, device=DEV)
    print("mixture_loglik err", stat_err(got, ref))
    assert np.isfinite(ref) and stat_err(got, ref) < RTOL_PAIRS
    # an empty PPK cluster (no centre, weight 0) is left out
    assert ev.mixture_loglik(centres + [None], np.append(w, 0.0), data, device=DEV) == got


def test_ccfd_end_to_end(ev):
    """Two planted families of 8 three-state HMMs, 10 sampled trials each (the case of
    tests/test_ccfd_gpu.py's end-to-end test): myccfd, then evaluate_run with the index."""
    from vbhem_amd import ccfd
    hmms, fam = pr.families(3, 2, 2, 8, seed=0)
    rng = np.random.default_rng(77)
    data = [sr.sample_data(rng, [h], [int(v) for v in rng.integers(1, 9, 10)], 2) for h in hmms]
    res = ccfd.myccfd(hmms, data, device=DEV)
    out = ev.evaluate_run("ccfd", res, fam, num_hmm=2, num_sta=3, hmms=hmms, data=data, cpt_dist=True, device=DEV)
    assert np.isfinite(out["DI"]) and out["DI"] > 0
    assert out["RI"] == ev.rand_index(fam, res["label"])[0] and out["purity"] == ev.purity(fam, res["label"])
    assert out["K_select"] == len(res["ccfd_result"]["icl"]) >= 2
    icl = res["ccfd_result"]["icl"]
    ref = dr.dunn([hmms[i] for i in icl], hmms, data, res["groups"], "ccfd", icl)
    assert stat_err(out["DI"], ref["DI"]) < RTOL_PAIRS
    s = ev.summarize([out, out])
    assert s["mean_DI"] == out["DI"] and s["std_DI"] == 0.0
