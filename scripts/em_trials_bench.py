"""The EM of R batched trials, host engine against device engine
(em.vbhem_h3m_c_trials(..., em_engine=...)): both run alternating in one
process on the same initial posteriors, a host clock around each run with the device
synchronised before and after, one warm-up run of each first, then --repeats timed runs of
each; the median, the fastest and the slowest run are reported, in milliseconds end to
end and per EM iteration (end to end / iterations of the loop = the longest trial's).

Shapes: (a) the face demo's (a face-like stand-in for its subjects: K = 3, S = 3, d = 2,
tau = 5, 50 trials), (b) 10,000 bases of C3 (K = 8, S = 5, d = 2, 16 trials), (c) 2,000
bases of C4 (K = 16, S = 8, d = 8, 8 trials).  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import pkgload

vb = pkgload.load()
from vbhem_amd import em  # noqa: E402
from vbhem_amd.estep import EStepEngine  # noqa: E402


def trial_posts(P, R, seed):
    """R distinct initialisations: P and R - 1 re-perturbed copies."""
    posts = [P.copy()]
    for r in range(1, R):
        Q = P.copy()
        rng = np.random.default_rng(seed * 100 + r)
        Q.epsilon = Q.epsilon * rng.uniform(0.3, 1.7, Q.epsilon.shape)
        Q.eta = Q.eta * rng.uniform(0.3, 1.7, Q.eta.shape)
        Q.m = Q.m + rng.normal(0.0, 0.5, Q.m.shape) * np.maximum(1.0, np.abs(Q.m).max() / 20)
        Q.alpha = Q.alpha * rng.uniform(0.5, 1.5, Q.alpha.shape)
        posts.append(Q)
    return posts


def shape_a(dev):
    K, S, d, N = 3, 3, 2, 20
    base = vb.synth_base_set(N, K, 3, d, vb.COV_FULL, seed=1001, device=dev, face=True)
    opt = vb.default_options(K, S, d, tau=5, Nv=100, covmode=vb.COV_FULL, v0=10.0, W0=0.001)
    rb, rg, om = vb.baseem_draws(base.to("cpu"), K, S, seed=78)
    return "a_face_like", base, vb.baseem_init(base.to("cpu"), opt, rb, rg, om), opt, 50


def shape_b(dev):
    base, post, opt = vb.synth_workload("C3", device=dev, N=10_000)
    return "b_C3_10000", base, post, opt, 16


def shape_c(dev):
    base, post, opt = vb.synth_workload("C4", device=dev, N=2_000)
    return "c_C4_2000", base, post, opt, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--shapes", default="abc")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for key, make in (("a", shape_a), ("b", shape_b), ("c", shape_c)):
        if key not in args.shapes:
            continue
        name, base, post, opt, R = make(dev)
        K, S, d = post.m.shape
        opt = dict(opt, max_iter=args.max_iter)
        posts = trial_posts(post, R, 7)
        eng = {e: EStepEngine(base, R * K, S, opt["tau"], device=dev, trials=R) for e in ("host", "device")}
        times = {"host": [], "device": []}
        last = {}
        for rep in range(args.repeats + 1):  # the first of each is the warm-up
            for e in ("host", "device"):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                last[e] = em.vbhem_h3m_c_trials(posts, eng[e], opt, em_engine=e)
                torch.cuda.synchronize(dev)
                if rep:
                    times[e].append((time.perf_counter() - t0) * 1e3)
        h, g = last["host"], last["device"]
        loops = max(a.iters + (0 if a.stable else 1) for a in h.results)
        row = dict(shape=name, N=base.N, K=K, S=S, d=d, R=R, tau=opt["tau"], max_iter=opt["max_iter"],
                   minDiff=opt["minDiff"], repeats=args.repeats, loop_iterations=loops,
                   iters_host=[a.iters for a in h.results], iters_device=[a.iters for a in g.results],
                   same_iters=[a.iters for a in h.results] == [a.iters for a in g.results],
                   same_best=h.best == g.best,
                   bound_rel_diff=float(np.nanmax(np.abs((g.LLall - h.LLall) / h.LLall))))
        for e in ("host", "device"):
            t = np.array(times[e])
            row[e] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()),
                          ms_per_iteration=float(np.median(t) / loops))
        row["speedup_median"] = row["host"]["ms_median"] / row["device"]["ms_median"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
