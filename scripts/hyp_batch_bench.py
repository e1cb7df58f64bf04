"""The hyperparameter learning of a clustering's unique trials, host loop against batched
device runs (cluster.vbhem_h3m_c(..., learn_hyps=1, hyp_engine=...)): both
run alternating in one process from the same seed, a host clock around each whole
clustering call (trials, then the learning of the unique ones) with the device
synchronised before and after, one warm-up run of each first, then --repeats timed runs of
each; the median, the fastest and the slowest run are reported in milliseconds.
hyp_engine="host" is the code of the commit before the option existed, byte for byte: the
option only chooses between that loop and hyp.vbhem_h3m_c_hyp_batch.

Shapes: (a) the face demo's (a face-like stand-in for its subjects: K = 3, S = 3, d = 2,
tau = 5, 50 trials), (c) 2,000 bases of C4 (K = 16, S = 8, d = 8, 8 trials).  The trials' own
EM runs on em_engine="device" in both.  One JSON line per shape."""
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
from vbhem_amd import cluster  # noqa: E402


def shape_a(dev):
    K, S, d, N = 3, 3, 2, 20
    base = vb.synth_base_set(N, K, 3, d, vb.COV_FULL, seed=1001, device=dev, face=True)
    opt = vb.default_options(K, S, d, tau=5, Nv=100, covmode=vb.COV_FULL, v0=10.0, W0=0.001)
    return "a_face_like", base, opt, 50


def shape_c(dev):
    base, post, opt = vb.synth_workload("C4", device=dev, N=2_000)
    return "c_C4_2000", base, opt, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--hyp-length", type=int, default=3, help="line searches per unique trial")
    ap.add_argument("--shapes", default="ac")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for key, make in (("a", shape_a), ("c", shape_c)):
        if key not in args.shapes:
            continue
        name, base, opt, R = make(dev)
        K, S = int(opt["K"]), int(opt["S"])
        opt = dict(opt, max_iter=args.max_iter, trials=R, seed=1001, initmode="baseem", em_engine="device",
                   learn_hyps=1, hyp_length=args.hyp_length)
        times = {"host": [], "device": []}
        last = {}
        for rep in range(args.repeats + 1):  # the first of each is the warm-up
            for e in ("host", "device"):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                last[e] = cluster.vbhem_h3m_c(base, dict(opt, hyp_engine=e), dev)
                torch.cuda.synchronize(dev)
                if rep:
                    times[e].append((time.perf_counter() - t0) * 1e3)
        h, g = last["host"], last["device"]
        uniq = np.isfinite(h["LLall"])
        row = dict(shape=name, gpu=torch.cuda.get_device_name(dev), N=base.N, K=K, S=S, d=base.d, trials=R,
                   tau=opt["tau"], max_iter=opt["max_iter"], hyp_length=args.hyp_length, repeats=args.repeats,
                   unique_trials=int(uniq.sum()), same_unique=bool(np.array_equal(uniq, np.isfinite(g["LLall"]))),
                   same_best=h["best"] == g["best"],
                   evaluations_host=int(h["hyp"]["evaluations"]) if h["hyp"] else None,
                   evaluations_device=int(g["hyp"]["evaluations"]) if g["hyp"] else None,
                   bound_rel_diff=float(np.nanmax(np.abs((g["LLall"] - h["LLall"]) / h["LLall"])))
                   if uniq.any() and np.array_equal(uniq, np.isfinite(g["LLall"])) else None)
        for e in ("host", "device"):
            t = np.array(times[e])
            row[e] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))
        row["speedup_median"] = row["host"]["ms_median"] / row["device"]["ms_median"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
