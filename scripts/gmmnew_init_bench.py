#!/usr/bin/env python
"""Times the 'gmmNew' initialisation of the clustering trials on the host (one
h3m.gmmnew_init per trial, numpy) against the batched device path (h3m.gmmnew_init_batch:
every trial's hierarchical EM in one GPU call) under the two schedules of its k-means++
seeding (--schedule block | tiled | both: one workgroup per trial inside the EM call, or
the tiled seeding call followed by the EM call from its centres), at two shapes:

    (1) the demo:   the 10 subject HMMs of tests/golden/demo_fixations.npz (learned here
                    with the fused engine), K = 3, S = 3, 50 trials, host and device;
    (2) synthetic:  --n-bases base HMMs (default 10,000) of Sb = 8 states, d = 8, K = 16,
                    S = 8 (80,000 points; 100,000 bases give C4's 800,000), --trials trials
                    (default 16) on the device; the host is timed on --host-trials trials
                    (default ONE; 0: not at all) and its time per trial reported.

Host clock; every device call ends in a copy back to the host.  One warm-up of each schedule
per shape, then --repeats repeats in which the schedules alternate, in the same process on
the same draws (median and [fastest, slowest]).  Also reported per schedule: the seconds of
the device path's parts (seed: the tiled seeding call, a part of fit), the Lloyd passes and
E-steps the trials evaluated, the rounds every trial's seeding used under the tiled schedule
(S - 1 seeding rounds and the Lloyd passes), and the largest difference of a trial's state
centres from the host's relative to the largest |coordinate| (trials timed on both).  One
JSON line per shape.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pkgload  # noqa: E402
from vbhmm_em_bench import DEMO_VBOPT, demo_subjects, note, spread  # noqa: E402

PARTS = ("points", "fit", "seed", "host")


def host_points(base):
    bn = base.numpy()
    ns = bn["nstates"]
    return (np.concatenate([bn["centres"][i, :int(ns[i])] for i in range(base.N)]),
            np.concatenate([bn["covars"][i, :int(ns[i])] for i in range(base.N)]))


def one_shape(vb, name, base, opt, seeds, host_trials, repeats, dev, schedules):
    h3m = vb.h3m
    for sch in schedules:
        h3m.gmmnew_init_batch(base, opt, seeds[:2], dev, schedule=sch)       # warm-up
    td, parts, posts = {s: [] for s in schedules}, {s: [] for s in schedules}, {}
    for r in range(repeats):
        for sch in schedules:
            info = {}
            t0 = time.perf_counter()
            posts[sch] = h3m.gmmnew_init_batch(base, opt, seeds, dev, info=info, schedule=sch)
            td[sch].append(time.perf_counter() - t0)
            parts[sch].append(info)
            note(name, sch, "repeat", r, round(td[sch][-1], 4), {k: round(info[k], 4) for k in PARTS})
    th, diff, t_points = [], {s: 0.0 for s in schedules}, 0.0
    n = int(sum(int(v) for v in base.nstates.cpu().numpy()))
    if host_trials:
        t0 = time.perf_counter()
        pts = host_points(base)
        t_points = time.perf_counter() - t0
        for i in range(host_trials):
            t0 = time.perf_counter()
            P = h3m.gmmnew_init(base, opt, seeds[i], pts)
            th.append(time.perf_counter() - t0)
            for sch in schedules:
                diff[sch] = max(diff[sch], float(np.abs(P.m - posts[sch][i].m).max() / np.abs(pts[0]).max()))
            note(name, "host trial", i, round(th[-1], 3))
    out = dict(bench="gmmnew_init", shape=name, points=n, d=base.d, K=opt["K"], S=opt["S"], trials=len(seeds),
               host_trials_timed=host_trials)
    for sch in schedules:
        last = parts[sch][-1]
        out[sch] = dict(seconds=spread(td[sch]),
                        parts={k: float(np.median([p[k] for p in parts[sch]])) for k in PARTS},
                        fit_seconds=spread([p["fit"] for p in parts[sch]]), replayed_trials=len(last["replayed"]),
                        lloyd=last["lloyd"], esteps_min_max=[min(last["esteps"]), max(last["esteps"])],
                        max_centre_difference=diff[sch])
        if sch == "tiled":
            out[sch]["rounds_used"] = [opt["S"] - 1 + v for v in last["lloyd"]]
            out[sch]["rounds_launched"] = (opt["S"] - 1) + 100
    if len(schedules) == 2:
        a, b = posts["block"], posts["tiled"]
        out["tiled_vs_block_max_centre_difference"] = max(float(np.abs(p.m - q.m).max()) for p, q in zip(a, b))
        for key in ("seconds", "fit_seconds"):
            out["tiled_median_over_block_fastest_" + key] = out["tiled"][key]["median"] / out["block"][key]["min"]
    if host_trials:
        per_trial = float(np.median(th))
        out.update(host_seconds_per_trial=spread(th), host_points_seconds=t_points,
                   host_seconds_all_trials_extrapolated=per_trial * len(seeds) + t_points)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-bases", "--bases", dest="bases", type=int, default=10000)
    ap.add_argument("--host-trials", type=int, default=1)
    ap.add_argument("--trials", type=int, default=16, help="device trials at the synthetic shape")
    ap.add_argument("--schedule", choices=["block", "tiled", "both"], default="block")
    ap.add_argument("--shapes", nargs="*", default=["demo", "synthetic"])
    a = ap.parse_args()
    schedules = ["block", "tiled"] if a.schedule == "both" else [a.schedule]
    vb = pkgload.load()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    if "demo" in a.shapes:
        from vbhem_amd import vbhmm_em as em
        vopt = em.vbhmm_default_options(2, **dict(DEMO_VBOPT, numtrials=10))
        hmms, _ = em.vbhmm_learn_batch(demo_subjects(), [1, 2, 3], vopt, device=a.device, engine="fused", init="device")
        hmms = [em.vbhmm_remove_empty(h, 1e-3) for h in hmms]
        base = vb.hmms_to_h3m_hem(hmms, vb.COV_FULL, use_post=True)
        opt = vb.default_options(3, 3, 2, seed=1000)
        seeds = [1000 + t for t in range(1, 51)]
        print(json.dumps(one_shape(vb, "demo", base, opt, seeds, len(seeds), a.repeats, a.device, schedules)),
              flush=True)
    if "synthetic" in a.shapes:
        base = vb.synth_base_set(a.bases, 16, 8, 8, vb.COV_FULL, seed=1005)
        opt = vb.default_options(16, 8, 8, v0=10.0, seed=2000)
        seeds = [2000 + t for t in range(1, a.trials + 1)]
        print(json.dumps(one_shape(vb, "synthetic", base, opt, seeds, min(a.host_trials, len(seeds)), a.repeats,
                                   a.device, schedules)), flush=True)


if __name__ == "__main__":
    main()
