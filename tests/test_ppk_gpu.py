"""The probability product kernel Gram matrix on the GPU (ppk.py over
hmm_ppk_gram_kernel): parity with the numpy restatement (tests/ppk_ref.py) at
RTOL_PAIRS under conftest.stat_err, the three modes against each other bit for
bit, the inputs' edge cases, and ppk_sc end to end."""
import numpy as np
import pytest
import torch

import ppk_ref as pr
import score_ref as sr
from conftest import RTOL_PAIRS, stat_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ppk(vb, capi_lib):
    from vbhem_amd import ppk as mod
    return mod


@pytest.fixture(scope="module")
def score(vb, capi_lib):
    from vbhem_amd import score as mod
    return mod


def elem_rel(got, ref):
    """The largest elementwise relative error over the entries above 1e-200 (reported)."""
    big = np.abs(ref) > 1e-200
    return float(np.max(np.abs(got - ref)[big] / np.abs(ref)[big])) if big.any() else 0.0


def check_sym(ppk, hmms, ref, **kw):
    got = ppk.ppk_matrix(ppk.PpkSet(hmms, device=DEV, rho=kw.pop("rho", 0.5)), **kw).cpu().numpy()
    print("stat_err", stat_err(got, ref), "elementwise", elem_rel(got, ref))
    assert got.shape == ref.shape and stat_err(got, ref) < RTOL_PAIRS
    assert np.array_equal(got, got.T)
    return got


# ----------------------------------------------------------------------------
# parity and shapes
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_gpu_matches_restatement(ppk, shape):
    check_sym(ppk, pr.make_set(*shape), pr.reference(*shape))


# tile sides are 4 (2 at 16 states x 8 dimensions): one HMM, a partial tile, one past
# a tile, several tiles with a partial one at the end
@pytest.mark.parametrize("H", [1, 2, 5, 17, 33])
def test_gpu_set_sizes(ppk, H):
    check_sym(ppk, pr.make_set(3, 2, False, H=H), pr.reference(3, 2, False, H=H))


@pytest.mark.parametrize("K,d,diag,H", [(16, 8, False, 2), (16, 8, False, 5), (8, 3, True, 5), (9, 2, False, 6)])
def test_gpu_set_sizes_of_the_larger_buckets(ppk, K, d, diag, H):
    check_sym(ppk, pr.make_set(K, d, diag, H=H), pr.reference(K, d, diag, H=H))


@pytest.mark.parametrize("T,rho", [(1, 0.5), (2, 0.5), (10, 0.3), (3, 1.0)])
def test_gpu_T_and_rho(ppk, T, rho):
    hmms = pr.make_set(5, 3, False, H=4)
    check_sym(ppk, hmms, pr.reference(5, 3, False, H=4, T=T, rho=rho), T=T, rho=rho)


def test_gpu_rectangular(ppk):
    a, b = pr.make_set(3, 2, False, H=3), pr.make_set(3, 2, False, H=17)
    sa, sb = ppk.PpkSet(a, device=DEV), ppk.PpkSet(b, device=DEV)
    ab, ba = ppk.ppk_matrix(sa, sb).cpu().numpy(), ppk.ppk_matrix(sb, sa).cpu().numpy()
    assert ab.shape == (3, 17) and ba.shape == (17, 3)
    ref = pr.gram(a, b)
    assert stat_err(ab, ref) < RTOL_PAIRS and stat_err(ba, ref.T) < RTOL_PAIRS
    # sets of different padded state counts (buckets 4 and 16)
    c = pr.make_set(9, 2, False, H=5)
    ac = ppk.ppk_matrix(sa, ppk.PpkSet(c, device=DEV)).cpu().numpy()
    ca = ppk.ppk_matrix(ppk.PpkSet(c, device=DEV), sa).cpu().numpy()
    ref = pr.gram(a, c)
    assert stat_err(ac, ref) < RTOL_PAIRS and stat_err(ca, ref.T) < RTOL_PAIRS


# ----------------------------------------------------------------------------
# the modes against each other
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("K,d,H", [(3, 2, 17), (8, 4, 6), (16, 8, 5)])
def test_gpu_modes_agree_bitwise(ppk, K, d, H):
    s = ppk.PpkSet(pr.make_set(K, d, False, H=H), device=DEV)
    sym = ppk.ppk_matrix(s)
    full = ppk.ppk_matrix(s, s)
    assert torch.equal(sym, sym.T)
    assert torch.equal(torch.triu(sym), torch.triu(full))
    assert stat_err(np.tril(sym.cpu().numpy()), np.tril(full.cpu().numpy())) < RTOL_PAIRS
    diag = ppk._gram(s, s, 10, ppk.MODE_DIAG)
    assert diag.shape == (H,) and torch.equal(diag, torch.diagonal(full))
    nrm = ppk.ppk_matrix(s, normalize=True)
    assert torch.max(torch.abs(torch.diagonal(nrm) - 1.0)).item() < 1e-15
    assert torch.equal(nrm, nrm.T)
    want = full / torch.sqrt(diag[:, None] * diag[None, :])
    assert torch.equal(ppk.ppk_matrix(s, s, normalize=True), want)
    assert torch.equal(ppk.ppk_matrix(s), sym)  # two runs


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def packed_base_set(p):
    from vbhem_amd.h3m import BaseSet
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return BaseSet(t(p["nstates"]), t(p["prior"]), t(p["trans"]), t(p["mean"]), t(p["cov"]),
                   torch.ones(len(p["nstates"]), dtype=torch.float64), p["covmode"])


@pytest.mark.parametrize("diag", [False, True])
def test_gpu_poisoned_padding_and_base_set(ppk, score, diag):
    hmms = pr.make_set(5, 3, diag, H=6)
    packed = score.pack_hmms(hmms)
    from_dicts = ppk.ppk_matrix(ppk.PpkSet(hmms, device=DEV))
    clean = ppk.ppk_matrix(ppk.PpkSet(packed_base_set(packed), device=DEV))
    assert torch.equal(from_dicts, clean)
    bad = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in packed.items()}
    for h, K in enumerate(bad["nstates"]):
        bad["mean"][h, K:] = np.nan
        bad["cov"][h, K:] = np.nan
        bad["prior"][h, K:] = np.nan
        bad["trans"][h, K:, :] = np.nan
        bad["trans"][h, :, K:] = np.nan
    assert np.isnan(bad["mean"]).any() and np.isnan(bad["trans"]).any()
    poisoned = ppk.ppk_matrix(ppk.PpkSet(packed_base_set(bad), device=DEV))
    assert torch.equal(poisoned, clean)
    assert stat_err(poisoned.cpu().numpy(), pr.reference(5, 3, diag, H=6)) < RTOL_PAIRS


def test_gpu_translation_invariance(ppk):
    hmms = pr.grid_set()
    base = ppk.ppk_matrix(ppk.PpkSet(hmms, device=DEV)).cpu().numpy()
    moved = ppk.ppk_matrix(ppk.PpkSet(pr.shifted(hmms, 4096.0), device=DEV)).cpu().numpy()
    print("translated vs unshifted:", stat_err(moved, base), elem_rel(moved, base))
    assert stat_err(moved, base) < RTOL_PAIRS
    assert stat_err(base, pr.gram(hmms)) < RTOL_PAIRS


def test_gpu_far_apart_families_underflow_cleanly(ppk):
    rng = np.random.default_rng(21)
    near = [sr.make_hmm(rng, 3, 2, False) for _ in range(3)]
    far = [sr.make_hmm(rng, 3, 2, False, centre=1e4) for _ in range(3)]
    K = ppk.ppk_matrix(ppk.PpkSet(near + far, device=DEV)).cpu().numpy()
    assert not np.isnan(K).any() and (K >= 0).all()
    assert K[:3, 3:].max() < 1e-300 and K[:3, :3].min() > 1e-30 and K[3:, 3:].min() > 1e-30
    assert stat_err(K, pr.gram(near + far)) < RTOL_PAIRS


# ----------------------------------------------------------------------------
# errors, the C-ABI through host arrays, ppk_sc end to end
# ----------------------------------------------------------------------------
def test_gpu_not_positive_definite_is_rejected_and_consumed(ppk):
    from vbhem_amd import _capi
    hmms = pr.make_set(3, 2, False, H=3)
    good = ppk.ppk_matrix(ppk.PpkSet(hmms, device=DEV))
    broken = [dict(h, pdf=[dict(p) for p in h["pdf"]]) for h in hmms]
    broken[2]["pdf"][1]["cov"] = np.array([[1.0, 0.0], [0.0, -3.0]])
    with pytest.raises(_capi.VbhemError, match="HMM 2 state 1 is not positive definite"):
        ppk.PpkSet(broken, device=DEV)
    s = torch.arange(8, device=DEV, dtype=torch.float64).sum()
    torch.cuda.synchronize()
    assert float(s) == 28.0
    assert torch.equal(ppk.ppk_matrix(ppk.PpkSet(hmms, device=DEV)), good)


def test_gpu_argument_errors(ppk):
    from vbhem_amd import _capi
    hmms = pr.make_set(3, 2, False, H=3)
    for kw in (dict(rho=0.0), dict(rho=-0.5), dict(pad=-0.1)):
        with pytest.raises(_capi.VbhemError, match="status -1"):
            ppk.PpkSet(hmms, device=DEV, **kw)
    s = ppk.PpkSet(hmms, device=DEV)
    with pytest.raises(_capi.VbhemError, match="status -1"):
        ppk.ppk_matrix(s, T=0)
    with pytest.raises(_capi.VbhemError, match="status -1"):
        ppk.ppk_matrix(s, ppk.PpkSet(pr.make_set(3, 3, False, H=2), device=DEV))
    with pytest.raises(ValueError):
        ppk.ppk_matrix(s, ppk.PpkSet(hmms, rho=0.3, device=DEV))
    rng = np.random.default_rng(0)
    with pytest.raises(_capi.VbhemError, match="status -2"):
        ppk.PpkSet([sr.make_hmm(rng, 17, 2, False)], device=DEV)
    with pytest.raises(_capi.VbhemError, match="status -2"):
        ppk.PpkSet([sr.make_hmm(rng, 2, 9, False)], device=DEV)


def test_ppkcheck_device_entry(ppk, score):
    """The C-ABI through plain host arrays (tests/ppkcheck): the kernels themselves."""
    pc = pr.load_ppkcheck()
    ha, hb = pr.make_set(9, 3, False, H=5), pr.make_set(4, 3, False, H=3, seed=1)
    pa, pb = score.pack_hmms(ha), score.pack_hmms(hb)
    rc, sym = pr.run_ppkcheck(pc, pa, device=True)
    assert rc == 0 and stat_err(sym, pr.reference(9, 3, False, H=5)) < RTOL_PAIRS
    assert np.array_equal(sym, ppk.ppk_matrix(ppk.PpkSet(ha, device=DEV)).cpu().numpy())
    rc, rect = pr.run_ppkcheck(pc, pa, pb, T=3, device=True)
    assert rc == 0 and stat_err(rect, pr.gram(ha, hb, T=3)) < RTOL_PAIRS
    rc, dg = pr.run_ppkcheck(pc, pa, mode=pr.MODE_DIAG, device=True)
    assert rc == 0 and np.array_equal(dg, np.diag(sym))
    rc, host = pr.run_ppkcheck(pc, pa)
    assert rc == 0 and stat_err(sym, host) < RTOL_PAIRS


def test_ppk_sc_end_to_end(ppk):
    hmms, fam = pr.families(3, 2, 3, 8)
    res = ppk.ppk_sc(hmms, 3, seed=5, device=DEV)
    assert pr.one_label_per_family(res["label"], fam)
    assert stat_err(res["A"], pr.families_gram(3, 2, 3, 8)) < RTOL_PAIRS
    cpu = ppk.ppk_sc_from_gram(hmms, pr.families_gram(3, 2, 3, 8), 3, seed=5)
    assert np.array_equal(res["label"], cpu["label"])
    # within a family the rows of U differ by rounding only, so which member is nearest
    # the centre is not determined by the Gram matrix to 1e-10; membership is
    assert all(res["ind_center"][k] in res["group"][k] for k in range(3))
    assert all(res["hmms"][k] is hmms[res["ind_center"][k]] for k in range(3))
