"""CCFD clustering without a GPU (vbhem_amd/ccfd.py over its numpy engine, and the
host loops of tests/ccfdcheck): the restatement of CCFD.m / myccfd.m
(tests/ccfd_ref.py) pinned on hand-worked inputs, the search's rules on scripted
fitnesses, the numpy engine against the restatement on planted inputs, the row
routines and the host distance loop against the restatement, and the errors."""
import numpy as np
import pytest

import ccfd_ref as cr
import score_ref as sr
from conftest import RTOL_PAIRS, stat_err


@pytest.fixture(scope="module")
def ccfd(vb):
    from vbhem_amd import ccfd as mod
    return mod


@pytest.fixture(scope="module")
def check_lib():
    return cr.load_ccfdcheck()


def line(*x):
    x = np.array(x, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


# ----------------------------------------------------------------------------
# the restatement pinned on its own
# ----------------------------------------------------------------------------
def test_restatement_hand_worked_five_points():
    """Points 0, 1, 2, 10, 11 on a line, dc = 1.5.  By hand: only point 1 has two
    neighbours within 1.5; the others tie at one and keep their index order behind
    it; every point's nearest denser point and the distance to it; the top point
    gets the largest delta (8)."""
    rho, ordrho, delta, nneigh, maxd = cr.sweeps(line(0, 1, 2, 10, 11), 1.5)
    assert rho == [1, 2, 1, 1, 1]
    assert ordrho == [1, 0, 2, 3, 4]            # ties in rho: index order
    assert delta == [1, 8, 1, 8, 1] and nneigh == [1, -1, 1, 2, 3] and maxd == 11


def test_restatement_equal_distances_go_to_the_lower_rank():
    D = np.array([[0, 1, 3, 2], [1, 0, 1, 2], [3, 1, 0, 5], [2, 2, 5, 0]], dtype=np.float64)
    rho, ordrho, delta, nneigh, _ = cr.sweeps(D, 1.5)
    assert rho == [1, 2, 1, 0] and ordrho == [1, 0, 2, 3]
    # point 3 is at distance 2 from points 0 and 1: point 1 has the lower rank
    assert delta[3] == 2 and nneigh[3] == 1


def test_restatement_entry_equal_to_dc():
    """D[2][3] = 8 = dc: not counted by rho (strict), counted by the border test."""
    D = line(0, 1, 2, 10, 11)
    rho = cr.sweeps(D, 8.0)[0]
    assert rho == [2, 2, 2, 1, 1]
    cl = [0, 0, 0, 1, 1]
    assert cr.border_rho(D, 8.0, cl, rho, 2) == [1.5, 1.5]
    assert cr.border_rho(D, 7.999, cl, rho, 2) == [0.0, 0.0]


def test_restatement_negative_distance():
    D = line(0, 1, 2, 10, 11)
    D[0, 1] = D[1, 0] = -0.5
    rho, ordrho, delta, nneigh, maxd = cr.sweeps(D, 1.5)
    assert rho == [1, 2, 1, 1, 1] and delta[0] == -0.5 and nneigh[0] == 1 and maxd == 11
    # all distances negative: max(max(dist)) is the diagonal's 0, and the top point's
    # delta is the placeholder -1 when every other delta lies below it
    rho, ordrho, delta, nneigh, maxd = cr.sweeps(-line(0, 2, 4) - 2 * (1 - np.eye(3)), -5.0)
    assert maxd == 0 and rho == [1, 0, 1] and ordrho == [0, 2, 1]
    assert delta == [-1, -4, -6] and nneigh == [-1, 0, 0]


def test_restatement_fitness_divides_by_the_number_of_points():
    D, truth = cr.planted(2, 20, 1)
    res = cr.CCFD(D, 10, cr.upper(D))
    icl, cl = res["icl"], res["cl"]
    assert len(icl) == 2
    sums = [sum(D[i, icl[j]] for i in range(40) if cl[i] == j) for j in range(2)]
    fit1 = (sums[0] / 40 + sums[1] / 40) / 2
    assert res["fitness"] == pytest.approx(D[icl[0], icl[1]] / fit1, rel=1e-14)
    by_size = (sums[0] / (cl == 0).sum() + sums[1] / (cl == 1).sum()) / 2
    assert abs(res["fitness"] - D[icl[0], icl[1]] / by_size) > 0.1 * res["fitness"]


# ----------------------------------------------------------------------------
# the search on scripted fitnesses
# ----------------------------------------------------------------------------
SEARCH_D = np.array([[0.0, 0.0, 100.0], [0.0, 0.0, 50.0], [100.0, 50.0, 0.0]])   # dc = percent


class Script:
    """A CCFD double: call n of the search returns fitness script[n] (None: fails) and
    labels that carry n; the final call (with a dc) returns its dc as its fitness."""

    def __init__(self, script):
        self.script, self.calls, self.final = list(script), [], None

    def result(self, dc, final=False):
        n = len(self.calls)
        if final:
            self.final = dc
            return dict(fitness=-dc, dc=dc, icl=np.array([0]), cl=np.zeros(3, dtype=np.int64),
                        rho=np.zeros(3, dtype=np.int64), delta=np.zeros(3), nneigh=np.zeros(3, dtype=np.int64),
                        halo=np.zeros(3, dtype=np.int64))
        self.calls.append(dc)
        f = self.script[n]
        if f is None:
            return None
        return dict(fitness=f, dc=dc, icl=np.array([n % 3]), cl=np.full(3, n, dtype=np.int64))

    def for_ref(self, dist, p0, pur, slope, dc=None):
        res = self.result(float(p0) if dc is None else dc, dc is not None)
        if res is None:
            raise cr.NoSingular("scripted")
        return res

    def for_module(self, ccfd):
        def run(engine, stats, dcs, slope, want_halo):
            out = []
            for dc in dcs:
                res = self.result(dc, want_halo)
                out.append(ccfd.NoSingularPoints("scripted") if res is None else res)
            return out
        return run


# the double's labels name calls, not clusters: the weights of such a result are 0 / 0
scripted = pytest.mark.filterwarnings("ignore:invalid value encountered")


def run_both(ccfd, monkeypatch, script):
    """(trajectory of cut-offs, final percent, final dc, the label's call number) of the
    restatement and of the module under the same script."""
    out = []
    a = Script(script)
    res = cr.myccfd_from_dist(SEARCH_D, 3, a.for_ref)
    out.append((a.calls, res["ccfd_result"]["percent"], a.final, int(res["label"][0])))
    b = Script(script)
    monkeypatch.setattr(ccfd, "_run_candidates", b.for_module(ccfd))
    res = ccfd.myccfd_from_dist(SEARCH_D)
    out.append((b.calls, res["ccfd_result"]["percent"], b.final, int(res["label"][0])))
    assert out[0][0] == pytest.approx(out[1][0], rel=1e-15) and out[0][1:] == out[1][1:]
    return out[1]


@scripted
def test_search_all_equal_takes_the_third(ccfd, monkeypatch):
    calls, percent, final, label = run_both(ccfd, monkeypatch, [1.0] * 18)
    want, p, r = [], 10.0, 3.0
    while r > 0:
        want += [p - r, p, p + r]
        p, r = p + r, r - 0.5
    assert calls == pytest.approx(want) and percent == 20.5
    assert final == pytest.approx(20.5) and label == 17       # the last round's third candidate


@scripted
def test_search_first_maximum_and_trajectory(ccfd, monkeypatch):
    # round 1: (5, 5, 1) -> the first of the two maxima, percent 7; round 2: the middle;
    # round 3: the third; then all equal
    script = [5, 5, 1, 0, 2, 1, 1, 2, 3] + [4.0] * 9
    calls, percent, final, label = run_both(ccfd, monkeypatch, script)
    assert calls[:9] == pytest.approx([7, 10, 13, 4.5, 7, 9.5, 5, 7, 9])
    assert percent == 9 + 1.5 + 1 + 0.5 and label == 17 and final == pytest.approx(calls[17])


@scripted
def test_search_slots_persist_across_rounds(ccfd, monkeypatch):
    # the last round fails three times: all equal at -realmax, so the third slot, which
    # still holds the fifth round's result (call 14)
    script = [1.0] * 15 + [None] * 3
    calls, percent, final, label = run_both(ccfd, monkeypatch, script)
    assert label == 14 and final == pytest.approx(calls[14]) and percent == 20.5
    # a slot that failed this round keeps its older result while another wins
    script = [1.0, 2.0, 3.0] + [None, 1.0, None] * 5
    calls, percent, final, label = run_both(ccfd, monkeypatch, script)
    assert label == 16 and percent == 13.0


def test_search_never_filled_slot_raises(ccfd, monkeypatch):
    for script in ([None] * 18, [1.0, 2.0, None] * 5 + [None] * 3):
        with pytest.raises(cr.NoSingular):
            cr.myccfd_from_dist(SEARCH_D, 3, Script(script).for_ref)
        monkeypatch.setattr(ccfd, "_run_candidates", Script(script).for_module(ccfd))
        with pytest.raises(ccfd.NoSingularPoints):
            ccfd.myccfd_from_dist(SEARCH_D)


# ----------------------------------------------------------------------------
# planted inputs: the numpy engine against the restatement
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("G,per,seed", cr.PLANTED)
def test_planted_numpy_engine_equals_restatement(ccfd, G, per, seed):
    D, _ = cr.planted(G, per, seed)
    hmms = [dict(name=i) for i in range(len(D))]
    got = ccfd.myccfd_from_dist(np.array(D), hmms=hmms, device="cpu")
    cr.check_planted(got, G, per, seed)
    assert [h["name"] for h in got["hmms"]] == list(got["ccfd_result"]["icl"])
    # one CCFD call at the chosen cut-off: the same vectors, and the neighbours
    one = ccfd.CCFD(np.array(D), None, dc=got["ccfd_result"]["dc"])
    ref = cr.CCFD(D, None, None, 3, got["ccfd_result"]["dc"])
    assert np.array_equal(one["nneigh"], ref["nneigh"]) and np.array_equal(one["halo"], ref["halo"])
    pct = ccfd.CCFD(np.array(D), 10.0)
    assert pct["dc"] == pytest.approx(cr.CCFD(D, 10.0, cr.upper(D))["dc"], rel=1e-12)


@pytest.mark.parametrize("N", [2, 3, 17, 65])
def test_numpy_engine_passes_equal_restatement(ccfd, N):
    D, dcs, cl, rho_b, want = cr.pass_case(N)
    eng = ccfd.NumpyEngine(np.array(D))
    rho = eng.rho(dcs)
    assert np.array_equal(rho, want["rho"])
    ranks = [ccfd.rank_of(r) for r in rho]
    assert np.array_equal(np.stack(ranks), want["rank"])
    delta, nneigh = eng.delta(ranks, want["maxd"])
    assert delta.tobytes() == want["delta"].tobytes() and np.array_equal(nneigh, want["nneigh"])
    assert np.array_equal(eng.border(dcs[0], cl, rho_b), want["border"])
    mn, mx, maxd = eng.stats()
    assert (mn, mx, maxd) == (want["rowmin"].min(), want["rowmax"][:-1].max(), want["maxd"])


# ----------------------------------------------------------------------------
# the host loops of tests/ccfdcheck
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", cr.PASS_SIZES)
def test_row_routines_on_the_host_equal_restatement(check_lib, N):
    D, dcs, cl, rho_b, want = cr.pass_case(N)
    got = cr.run_passes_host(check_lib, D, dcs, want["rank"], want["maxd"], cl, rho_b)
    for k in ("rowmin", "rowmax", "rho", "nneigh", "border"):
        assert np.array_equal(got[k], want[k]), k
    assert got["delta"].tobytes() == want["delta"].tobytes()
    if N >= 3:
        assert (want["nneigh"][:, 0] == -1).all() and (want["delta"][:, 0] == np.where(want["rank"][:, 0] == 0, -1, 5)).all()


@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_host_distance_loop_matches_restatement(vb, check_lib, shape):
    from vbhem_amd import score
    K, d, diag = shape
    hmms, data, ref = cr.distance_case(K, d, diag)
    rc, D = cr.run_distance_check(check_lib, score.pack_hmms(hmms), data, d)
    print("distance err", stat_err(D, ref))
    assert rc == 0 and np.isfinite(ref).all()
    assert stat_err(D, ref) < RTOL_PAIRS
    assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()


def test_host_distance_empty_segment_is_nan(vb, check_lib):
    from vbhem_amd import score
    hmms, data, _ = cr.distance_case(3, 2, False)
    data = [data[0], [], data[2]]
    ref = cr.distance(hmms, data)
    rc, D = cr.run_distance_check(check_lib, score.pack_hmms(hmms), data, 2)
    assert rc == 0 and np.isnan(ref[1, [0, 2]]).all() and np.isnan(D[1, [0, 2]]).all() and np.isnan(D[[0, 2], 1]).all()
    assert D[1, 1] == 0 and stat_err(D[0, 2], ref[0, 2]) < RTOL_PAIRS


# ----------------------------------------------------------------------------
# errors
# ----------------------------------------------------------------------------
def test_errors(ccfd):
    with pytest.raises(ValueError, match="at least 2"):
        ccfd.myccfd_from_dist(np.zeros((1, 1)))
    with pytest.raises(ValueError, match="square"):
        ccfd.CCFD(np.zeros((2, 3)), 10)
    bad = np.array(cr.planted(2, 20, 1)[0])
    bad[3, 5] = bad[5, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ccfd.myccfd_from_dist(bad)
    bad[3, 5] = bad[5, 3] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        ccfd.CCFD(bad, 10)
    same = 2.5 * (1 - np.eye(6))
    with pytest.raises(ccfd.NoSingularPoints):
        ccfd.CCFD(same, 10)
    with pytest.raises(ccfd.NoSingularPoints):
        ccfd.myccfd_from_dist(same)
    with pytest.raises(cr.NoSingular):
        cr.myccfd_from_dist(same)
    assert issubclass(ccfd.NoSingularPoints, RuntimeError)
