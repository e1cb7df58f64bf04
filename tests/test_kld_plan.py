"""The planner of vbhmm_kld_jobs (csrc/vbhmm_kld_plan.h) on the CPU, through its host
build (tests/kldcheck): every (job, item) lands in exactly one tile lane and every
own-table slot is written exactly once, at the tile edges and for gathered lists; the
host walk of the planned tiles -- the kernels' chain of additions -- equals the
restatement (tests/dunn_ref.py) at RTOL_PAIRS under conftest.stat_err; and every
invalid argument is refused with VBHEM_ERR_ARG and the offender named, before anything
could reach a kernel."""
import ctypes

import numpy as np
import pytest

import dunn_ref as dr
from conftest import RTOL_PAIRS, stat_err

H, N = 6, 300


@pytest.fixture(scope="module")
def lib():
    return dr.load_kldcheck()


@pytest.fixture(scope="module")
def packed(vb):
    from vbhem_amd import score
    return score.pack_hmms(dr.small_case()[0])


def walk(lib, packed, lists, jobs):
    rc, msg, kl, own_hits, pair_hits = dr.run_jobs(lib, packed, dr.small_case()[1], 2, lists, jobs)
    assert rc == 0, msg
    # every own-table slot written once, every (job, item) taken once
    assert (own_hits == 1).all() and (pair_hits == 1).all()
    want = dr.jobs_from_ll(dr.small_ll(), lists, jobs)
    nonempty = np.array([len(lists[l]) > 0 for _, _, l in jobs], dtype=bool)
    assert np.isfinite(want[nonempty]).all() and np.isnan(want[~nonempty]).all()
    print("walk err", stat_err(kl, want))
    assert stat_err(kl, want) < RTOL_PAIRS
    return kl


@pytest.mark.parametrize("c", dr.EDGE_LENGTHS)
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["reversed", "strided", "repeated"])
def test_edge_lengths_and_gathered_items(lib, packed, c, kind):
    lists = [dr.gathered(c, kind, N)]
    jobs = [(0, 1, 0), (2, 1, 0), (4, 5, 0)]
    walk(lib, packed, lists, jobs)
    rc, _, counts = dr.run_plan(lib, H, N, lists, jobs)
    passes = -(-c // 128)
    # three unique (a, list) runs; jobs 0 and 1 share b and pack only while both fit a tile
    assert rc == 0 and counts[0] == 3 * c and counts[1] == 3 * passes and counts[2] == 3 * c
    assert counts[4] == passes and counts[3] == (2 if 2 * c <= 128 else 3)
    assert 12 * counts[0] <= counts[5] <= 12 * counts[0] + 1024    # no table grows with the (job, item) pairs


def test_257_items_take_three_passes(lib):
    rc, _, counts = dr.run_plan(lib, H, N, [dr.gathered(257, 0, N)], [(0, 1, 0)])
    assert rc == 0 and counts[3] == 1 and counts[4] == 3 and counts[1] == 3


def test_short_jobs_pack_to_exactly_128_lanes_and_one_over(lib, packed):
    lists = [dr.gathered(60, 1, N), dr.gathered(8, 0, N), dr.gathered(9, 2, N)]
    fits = [(0, 3, 0), (1, 3, 0), (2, 3, 1)]          # 60 + 60 + 8 = 128: one tile
    over = [(0, 4, 0), (1, 4, 0), (2, 4, 2)]          # 60 + 60 + 9 = 129: the last job opens a tile
    rc, _, counts = dr.run_plan(lib, H, N, lists, fits)
    assert rc == 0 and counts[2] == 128 and counts[3] == 1
    rc, _, counts = dr.run_plan(lib, H, N, lists, over)
    assert rc == 0 and counts[2] == 129 and counts[3] == 2
    both = walk(lib, packed, lists, fits + over)
    # a job's value does not depend on what it is packed with
    assert np.array_equal(walk(lib, packed, lists, fits), both[:3])
    assert np.array_equal(walk(lib, packed, lists, [over[2]]), both[5:])


def test_a_list_shared_by_many_jobs(lib, packed):
    """300 jobs over three lists (one empty), more jobs of one b than a tile has lanes, b in
    no order: one own run per unique (a, list), NaN for the empty list alone."""
    lists = [dr.gathered(3, 0, N), [], [5]]
    jobs = [(j % H, (5 * j + 1) % H, 1 if j % 7 == 0 else 0 if j % 3 else 2) for j in range(300)]
    kl = walk(lib, packed, lists, jobs)
    empty = np.array([l == 1 for _, _, l in jobs])
    assert np.isnan(kl[empty]).all() and np.isfinite(kl[~empty]).all()
    rc, _, counts = dr.run_plan(lib, H, N, lists, jobs)
    uniq = {(a, l) for a, _, l in jobs}
    assert rc == 0 and counts[0] == sum(len(lists[l]) for _, l in uniq)
    # the same job gives the same bits wherever it stands
    again = walk(lib, packed, lists, jobs[::-1])[::-1]
    assert kl.tobytes() == again.tobytes()


def test_a_equals_b_and_no_jobs(lib, packed):
    kl = walk(lib, packed, [dr.gathered(130, 1, N)], [(2, 2, 0), (0, 0, 0)])
    assert (np.abs(kl) <= 1e-12).all()
    rc, msg, counts = dr.run_plan(lib, H, N, [[1, 2]], np.zeros((0, 3)))
    assert rc == 0 and not counts[:5].any()


BAD = [
    ("a = -1", [(0, 1, 0), (-1, 1, 0)], None, "job 1: HMM a = -1 is outside [0, 6)"),
    ("a = H", [(0, 1, 0), (H, 1, 0)], None, "job 1: HMM a = 6 is outside [0, 6)"),
    ("b = -1", [(0, -1, 0)], None, "job 0: HMM b = -1 is outside [0, 6)"),
    ("b = H", [(0, 1, 0), (0, 1, 1), (0, H, 0)], None, "job 2: HMM b = 6 is outside [0, 6)"),
    ("list = -1", [(0, 1, -1)], None, "job 0: list -1 is outside [0, 3)"),
    ("list = n_lists", [(0, 1, 3)], None, "job 0: list 3 is outside [0, 3)"),
    ("item = -1", [(0, 1, 1)], None, "list 1 item 1: sequence -1 is outside [0, 300)"),
    ("item = N", [(0, 1, 0), (0, 1, 2)], None, "list 2 item 0: sequence 300 is outside [0, 300)"),
    ("decreasing offsets", [(0, 1, 0)], [0, 3, 2, 4], "list offsets decrease at list 1"),
]


@pytest.mark.parametrize("name,jobs,offsets,needle", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_and_named(lib, name, jobs, offsets, needle):
    lists = [[0, 1, 2], [3, -1], [N]]
    rc, msg, _ = dr.run_plan(lib, H, N, lists, jobs, offsets)
    assert rc == dr.ERR_ARG and needle in msg, msg


def test_an_unused_list_is_not_checked(lib):
    rc, msg, counts = dr.run_plan(lib, H, N, [[0, 1, 2], [-5, N + 7]], [(0, 1, 0)])
    assert rc == 0 and counts[2] == 3, msg


def test_the_library_refuses_before_it_touches_the_device(capi_lib):
    """vbhmm_kld_jobs itself, with null device pointers: the refusal comes from the host
    checks, and vbhem_last_error() names the offender."""
    from vbhem_amd import _capi
    desc = _capi.ScoreHmmsT(H, 3, 2, 0, 0, 0, 0, 0, 0)
    host = np.zeros(2)                 # stands in for the sequences' arrays: never read, the refusal comes first
    sd = _capi.SeqsT(N, 2, 0, host.ctypes.data, host.ctypes.data)
    off, items = dr.flat_lists([[0, 1, 2], [3, N]])
    for jobs, needle in (([(0, 1, 0), (0, H, 0)], "job 1: HMM b = 6"), ([(0, 1, 1)], "list 1 item 1: sequence 300")):
        jb = np.ascontiguousarray(jobs, dtype=np.int32)
        rc = capi_lib.vbhmm_kld_jobs(ctypes.byref(desc), 0, ctypes.byref(sd), 2, off.ctypes.data, items.ctypes.data,
                                     len(jb), jb.ctypes.data, 0, 0, 0, 0)
        assert rc == dr.ERR_ARG and needle in capi_lib.vbhem_last_error().decode()
    jb = np.ascontiguousarray([(0, 1, 0)], dtype=np.int32)
    assert capi_lib.vbhmm_kld_jobs_workspace_bytes(2, off.ctypes.data, 1, jb.ctypes.data) >= 3 * 8 + 3 * 4
    assert capi_lib.vbhmm_kld_jobs(ctypes.byref(desc), 0, ctypes.byref(sd), 2, off.ctypes.data, items.ctypes.data,
                                   0, jb.ctypes.data, 0, 0, 0, 0) == 0      # no jobs: nothing to do
    dec = np.array([0, 3, 2], dtype=np.int32)
    assert capi_lib.vbhmm_kld_jobs_workspace_bytes(2, dec.ctypes.data, 1, jb.ctypes.data) == 0
