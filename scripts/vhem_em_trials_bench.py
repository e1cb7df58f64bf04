"""The VHEM EM of R batched trials, host engine against device engine
(vhem.hem_h3m_c_trials(..., em_engine=...)): both run alternating in one
process on the same initial mixtures, a host clock around each run with the device
synchronised before and after, one warm-up run of each first, then --repeats timed runs of
each; the median, the fastest and the slowest run are reported, in milliseconds end to end
and per EM iteration (end to end / E-steps of the loop = the longest trial's).

Shapes (those of scripts/em_trials_bench.py): (a) a face-like stand-in for the demo's
subjects (N = 20, K = 3, S = 3, d = 2, 50 trials), (b) 10,000 bases of C3 (K = 8, S = 5,
d = 2 diag, 16 trials), (c) 2,000 bases of C4 (K = 16, S = 8, d = 8 full, 8 trials).  The
initial mixtures are 'baseem' initialisations, one Generator per trial.  One JSON line per
shape; "verdict" is "gain" when the device engine's slowest run is below the host
engine's fastest, else "no gain"."""
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
from vbhem_amd import vhem  # noqa: E402
from vbhem_amd.estep import EStepEngine  # noqa: E402


def shape_a(dev):
    return "a_face_like", vb.synth_base_set(20, 3, 3, 2, vb.COV_FULL, seed=1001, device=dev, face=True), 3, 3, 5, 50


def shape_b(dev):
    base, post, opt = vb.synth_workload("C3", device=dev, N=10_000)
    return "b_C3_10000", base, post.m.shape[0], post.m.shape[1], opt["tau"], 16


def shape_c(dev):
    base, post, opt = vb.synth_workload("C4", device=dev, N=2_000)
    return "c_C4_2000", base, post.m.shape[0], post.m.shape[1], opt["tau"], 8


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
        name, base, K, S, tau, R = make(dev)
        cov = base.covmode
        opt = vhem.default_hemopt(K, S, seed=1, initmode="baseem", tau=int(tau), max_iter=args.max_iter,
                                  covar_type="full" if cov == vb.COV_FULL else "diag")
        cpu = base.to("cpu")
        inits = [vhem.initialize_hem_h3m_c(cpu, opt, np.random.Generator(np.random.PCG64(100 + r)))
                 for r in range(R)]
        eng = {e: EStepEngine(base, R * K, S, int(tau), device=dev, trials=R) for e in ("host", "device")}
        times = {"host": [], "device": []}
        last = {}
        for rep in range(args.repeats + 1):  # the first of each is the warm-up
            for e in ("host", "device"):
                rngs = [np.random.Generator(np.random.PCG64(500 + r)) for r in range(R)]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                last[e] = vhem.hem_h3m_c_trials(inits, eng[e], opt, rngs, em_engine=e)
                torch.cuda.synchronize(dev)
                if rep:
                    times[e].append((time.perf_counter() - t0) * 1e3)
        h, g = last["host"], last["device"]
        loops = max(len(a["LogLs"]) for a in h)
        LLh, LLg = np.array([a["LogL"] for a in h]), np.array([a["LogL"] for a in g])
        row = dict(shape=name, N=base.N, K=K, S=S, d=base.d, R=R, tau=int(tau), max_iter=opt["max_iter"],
                   termvalue=opt["termvalue"], repeats=args.repeats, loop_esteps=loops,
                   num_iter_host=[a["num_iter"] for a in h], num_iter_device=[a["num_iter"] for a in g],
                   same_num_iter=[a["num_iter"] for a in h] == [a["num_iter"] for a in g],
                   same_best=int(np.nanargmax(LLh)) == int(np.nanargmax(LLg)),
                   fallback_trials=g[0]["fallback_trials"],
                   LogL_rel_diff=float(np.nanmax(np.abs((LLg - LLh) / LLh))))
        for e in ("host", "device"):
            t = np.array(times[e])
            row[e] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()),
                          ms_per_iteration=float(np.median(t) / loops))
        row["speedup_median"] = row["host"]["ms_median"] / row["device"]["ms_median"]
        row["verdict"] = "gain" if row["device"]["ms_max"] < row["host"]["ms_min"] else "no gain"
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
