"""KL jobs on the GPU (score.kld_jobs over the kernels of vbhmm_kld.hip): bitwise
equality with the CCFD distance on the jobs that distance is made of, the restatement
(tests/dunn_ref.py) at RTOL_PAIRS under conftest.stat_err over every state and dimension
bucket, gathered lists at the tile edges against score.ll_matrix, a job's value
independent of its place in the call, NaN for empty lists and empty sequences, a == b,
and the C ABI through plain host arrays."""
import numpy as np
import pytest
import torch

import ccfd_ref as cr
import dunn_ref as dr
import score_ref as sr
from conftest import RTOL_PAIRS, stat_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def score(vb, capi_lib):
    from vbhem_amd import score as mod
    return mod


@pytest.fixture(scope="module")
def ccfd(vb, capi_lib):
    from vbhem_amd import ccfd as mod
    return mod


@pytest.fixture(scope="module")
def tile(score):
    """The tile case resident on the device: (HmmSet, SequenceBatch, per-subject lists,
    ll_matrix [33][N] normalised, on the host)."""
    from vbhem_amd.vbhmm import SequenceBatch
    hmms, data = dr.tile_case()
    hset = score.HmmSet(hmms, DEV)
    sb = SequenceBatch([s for g in data for s in g], 2, DEV)
    first = np.concatenate([[0], np.cumsum([len(g) for g in data])])
    own = [np.arange(first[i], first[i + 1]) for i in range(len(data))]
    ll = score.ll_matrix(hset, sb).cpu().numpy()
    return hset, sb, own, ll


def test_bitwise_equal_to_the_ccfd_distance(score, ccfd, tile):
    """Every ordered pair (i, j != i) over subject i's own trials: 0.5 (kl[i, j] + kl[j, i])
    is ccfd.distance_matrix's entry bit for bit."""
    hset, sb, own, _ = tile
    hmms, data = dr.tile_case()
    H = len(hmms)
    D = ccfd.distance_matrix(hmms, data, device=DEV).cpu().numpy()
    jobs = [(i, j, i) for i in range(H) for j in range(H) if j != i]
    kl = score.kld_jobs(hset, sb, own, jobs)
    assert kl.dtype == torch.float64 and kl.device.type == "cuda" and tuple(kl.shape) == (H * (H - 1),)
    K = np.zeros((H, H))
    for (i, j, _), v in zip(jobs, kl.cpu().numpy()):
        K[i, j] = v
    S = 0.5 * (K + K.T)
    assert np.isfinite(D).all() and S.tobytes() == D.tobytes()


@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_matches_restatement(score, shape):
    K, d, diag = shape
    hmms, data, _ = cr.distance_case(K, d, diag)
    seqs = [s for g in data for s in g]
    assert min(len(s) for s in seqs) >= 1
    first = np.concatenate([[0], np.cumsum([len(g) for g in data])])
    lists = [np.arange(first[i], first[i + 1]) for i in range(3)] + [np.arange(len(seqs))[::-1]]
    jobs = [(a, b, l) for a in range(3) for b in range(3) for l in (a, 3)]
    ref = dr.kld_jobs(hmms, seqs, lists, jobs)
    assert np.isfinite(ref).all()
    got = score.kld_jobs(score.HmmSet(hmms, DEV), seqs, lists, jobs).cpu().numpy()
    print("kld_jobs err", stat_err(got, ref))
    assert stat_err(got, ref) < RTOL_PAIRS


def test_gathered_lists_at_the_tile_edges(score, tile):
    hset, sb, own, ll = tile
    N = sb.N
    lists = [dr.gathered(c, kind, N) for c in (1, 127, 128, 129, 257) for kind in (0, 1, 2)]
    jobs = [(a, b, l) for l in range(len(lists)) for a, b in ((l % 33, (l + 5) % 33), (32 - l, l % 33))]
    got = score.kld_jobs(hset, sb, lists, jobs).cpu().numpy()
    want = dr.jobs_from_ll(ll, lists, jobs)
    assert np.isfinite(want).all()
    print("against ll_matrix", stat_err(got, want))
    assert stat_err(got, want) < RTOL_PAIRS


def test_value_does_not_depend_on_the_other_jobs(score, tile):
    """A job alone, first and last among 500 other jobs, for a packed job and a long one;
    two identical calls."""
    hset, sb, own, _ = tile
    rng = np.random.default_rng(3)
    lists = list(own) + [dr.gathered(257, 1, sb.N), dr.gathered(5, 2, sb.N)]
    others = [(int(a), int(b), int(l)) for a, b, l in zip(rng.integers(0, 33, 500), rng.integers(0, 33, 500),
                                                         rng.integers(0, len(lists), 500))]
    for job in ((3, 7, len(lists) - 1), (3, 7, len(lists) - 2), (9, 7, 4)):
        alone = score.kld_jobs(hset, sb, lists, [job]).cpu().numpy()
        first = score.kld_jobs(hset, sb, lists, [job] + others).cpu().numpy()
        last = score.kld_jobs(hset, sb, lists, others + [job]).cpu().numpy()
        again = score.kld_jobs(hset, sb, lists, others + [job]).cpu().numpy()
        assert np.isfinite(alone).all()
        assert alone.tobytes() == first[:1].tobytes() == last[-1:].tobytes()
        assert first[1:].tobytes() == last[:-1].tobytes() and last.tobytes() == again.tobytes()


def test_empty_list_empty_sequence_and_no_jobs(score):
    hmms, seqs = dr.small_case()
    seqs = list(seqs[:40]) + [np.zeros((0, 2))]
    hset = score.HmmSet(hmms, DEV)
    lists = [[0, 1, 2], [], [3, 40, 4], [5]]
    jobs = [(0, 1, 0), (2, 1, 1), (3, 1, 2), (4, 1, 3), (5, 1, 0)]      # one b: all five in one tile
    got = score.kld_jobs(hset, seqs, lists, jobs).cpu().numpy()
    assert np.isnan(got[[1, 2]]).all() and np.isfinite(got[[0, 3, 4]]).all()
    want = dr.kld_jobs(hmms, seqs, lists, [jobs[i] for i in (0, 3, 4)])
    assert stat_err(got[[0, 3, 4]], want) < RTOL_PAIRS
    none = score.kld_jobs(hset, seqs, lists, np.zeros((0, 3), dtype=np.int64))
    assert tuple(none.shape) == (0,) and none.dtype == torch.float64 and none.device.type == "cuda"


def test_a_equals_b(score, tile):
    hset, sb, own, _ = tile
    jobs = [(i, i, i) for i in range(33)] + [(4, 4, 1)]
    got = score.kld_jobs(hset, sb, own, jobs).cpu().numpy()
    assert (np.abs(got) <= 1e-12).all()


def test_c_abi_and_refusal(score):
    """vbhmm_kld_jobs through plain host arrays (tests/kldcheck) equals the host walk of
    the planned tiles at RTOL_PAIRS (the host's exp and log are not the device's); an index
    out of range raises and names itself."""
    from vbhem_amd import _capi
    lib = dr.load_kldcheck()
    hmms, seqs = dr.small_case()
    packed = score.pack_hmms(hmms)
    lists = [dr.gathered(c, c % 3, 300) for c in dr.EDGE_LENGTHS] + [[]]
    jobs = [(l % 6, (l + j) % 6, l) for l in range(len(lists)) for j in range(3)]
    rc, msg, host, _, _ = dr.run_jobs(lib, packed, seqs, 2, lists, jobs)
    assert rc == 0, msg
    rc, dev = dr.run_jobs(lib, packed, seqs, 2, lists, jobs, device=True)
    assert rc == 0
    empty = np.array([l == len(lists) - 1 for _, _, l in jobs])
    assert np.isnan(dev[empty]).all() and np.isfinite(dev[~empty]).all()
    print("device against the host walk", stat_err(dev[~empty], host[~empty]))
    assert stat_err(dev[~empty], host[~empty]) < RTOL_PAIRS
    hset = score.HmmSet(hmms, DEV)
    with pytest.raises(_capi.VbhemError, match="job 1: HMM b = 6"):
        score.kld_jobs(hset, seqs, lists, [(0, 1, 0), (0, 6, 0)])
    with pytest.raises(_capi.VbhemError, match="list 0 item 1: sequence 300"):
        score.kld_jobs(hset, seqs, [[0, 300]], [(0, 1, 0)])
