#!/usr/bin/env python
"""Times the 'wtkmeans' initialisation of the clustering trials on the host (one
h3m.wtkmeans_init per trial, numpy) against the batched device path
(h3m.wtkmeans_init_batch: every trial's k-means in two GPU calls) under its two schedules
(--schedule block | tiled | both: one workgroup per trial, or every pass over a grid of
point tiles), at two shapes:

    (1) the demo:   the 10 subject HMMs of tests/golden/demo_fixations.npz (learned here
                    with the fused engine), K = 3, S = 3, 50 trials, host and device;
    (2) synthetic:  --n-bases base HMMs (default 10,000) of Sb = 8 states, d = 8, K = 16,
                    S = 8 (80,000 points; 100,000 bases give C4's 800,000), --trials trials
                    (default 16) on the device; the host is timed on --host-trials trials
                    (default ONE; 0: not at all) and its time per trial reported.

Host clock; every device part ends in a copy back to the host.  One warm-up of each
schedule per shape, then --repeats repeats in which the schedules alternate, in the same
process on the same draws (median and [fastest, slowest]).  Also reported per schedule: the
seconds of the device path's parts, the rounds every trial used under the tiled schedule
(K - 1 seeding rounds, the Lloyd passes, the first assignment, one round per energy the
stopping rule read), and the largest difference of a trial's state centres from the host's
relative to the largest |coordinate| (trials timed on both).  One JSON line per shape.
Needs a GPU.
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

PARTS = ("points", "cluster", "states", "host")


def rounds_used(K, iters):
    """The rounds a trial of the tiled schedule used, from its iteration counts."""
    return [int((K - 1) + it0 + 1 + min(it1 + 2, 101)) for it0, it1 in np.asarray(iters).tolist()]


def one_shape(vb, name, base, opt, seeds, host_trials, repeats, dev, schedules):
    h3m = vb.h3m
    for sch in schedules:
        h3m.wtkmeans_init_batch(base, opt, seeds[:2], dev, schedule=sch)     # warm-up
    td, parts, posts = {s: [] for s in schedules}, {s: [] for s in schedules}, {}
    for r in range(repeats):
        for sch in schedules:
            info = {}
            t0 = time.perf_counter()
            posts[sch] = h3m.wtkmeans_init_batch(base, opt, seeds, dev, info=info, schedule=sch)
            td[sch].append(time.perf_counter() - t0)
            parts[sch].append(info)
            note(name, sch, "repeat", r, round(td[sch][-1], 4), {k: round(info[k], 4) for k in PARTS})
    th, diff, t_points = [], {s: 0.0 for s in schedules}, 0.0
    n = int(sum(int(v) for v in base.nstates.cpu().numpy()))
    if host_trials:
        t0 = time.perf_counter()
        pts = h3m.wtkmeans_points(base, opt.get("initopt_mode", "r0"))
        t_points = time.perf_counter() - t0
        for i in range(host_trials):
            t0 = time.perf_counter()
            P = h3m.wtkmeans_init(base, opt, seeds[i], pts)
            th.append(time.perf_counter() - t0)
            for sch in schedules:
                diff[sch] = max(diff[sch], float(np.abs(P.m - posts[sch][i].m).max() / np.abs(pts[0]).max()))
            note(name, "host trial", i, round(th[-1], 3))
    out = dict(bench="wtk_init", shape=name, points=n, d=base.d, K=opt["K"], S=opt["S"], trials=len(seeds),
               host_trials_timed=host_trials)
    for sch in schedules:
        last = parts[sch][-1]
        out[sch] = dict(seconds=spread(td[sch]),
                        parts={k: float(np.median([p[k] for p in parts[sch]])) for k in PARTS},
                        cluster_seconds=spread([p["cluster"] for p in parts[sch]]),
                        second_stage_items=last["items"], replayed_trials=len(last["replayed"]),
                        iters=np.asarray(last["iters"]).tolist(), max_centre_difference=diff[sch])
        if sch == "tiled":
            out[sch]["rounds_used"] = rounds_used(opt["K"], last["iters"])
            out[sch]["rounds_launched"] = (opt["K"] - 1) + 100 + 1 + 101
    if len(schedules) == 2:
        a, b = posts["block"], posts["tiled"]
        out["tiled_vs_block_max_centre_difference"] = max(float(np.abs(p.m - q.m).max()) for p, q in zip(a, b))
        for key in ("seconds", "cluster_seconds"):
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
