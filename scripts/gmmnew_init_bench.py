#!/usr/bin/env python
"""Times the 'gmmNew' initialisation of the clustering trials on the host (one
h3m.gmmnew_init per trial, numpy) against the batched device path (h3m.gmmnew_init_batch:
every trial's hierarchical EM in one GPU call), at two shapes:

    (1) the demo:   the 10 subject HMMs of tests/golden/demo_fixations.npz (learned here
                    with the fused engine), K = 3, S = 3, 50 trials, host and device;
    (2) synthetic:  --bases base HMMs (default 10,000) of Sb = 8 states, d = 8, K = 16,
                    S = 8 (80,000 points), --trials trials (default 16) on the device; the
                    host is timed on --host-trials trials (default ONE) and its time per
                    trial reported.

Host clock; the device call ends in a copy back to the host.  One warm-up of the device
path per shape, then --repeats repeats (minimum and median).  Also reported: the seconds
of the device path's parts, the E-steps the trials evaluated, and the largest difference
of a trial's state centres between the two paths relative to the largest |coordinate|
(trials timed on both).  One JSON line per shape.  Needs a GPU.
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


def host_points(base):
    bn = base.numpy()
    ns = bn["nstates"]
    return (np.concatenate([bn["centres"][i, :int(ns[i])] for i in range(base.N)]),
            np.concatenate([bn["covars"][i, :int(ns[i])] for i in range(base.N)]))


def one_shape(vb, name, base, opt, seeds, host_trials, repeats, dev):
    h3m = vb.h3m
    h3m.gmmnew_init_batch(base, opt, seeds[:2], dev)                        # warm-up
    td, parts, posts = [], [], None
    for r in range(repeats):
        info = {}
        t0 = time.perf_counter()
        posts = h3m.gmmnew_init_batch(base, opt, seeds, dev, info=info)
        td.append(time.perf_counter() - t0)
        parts.append(info)
        note(name, "device repeat", r, round(td[-1], 4), {k: round(info[k], 4) for k in ("points", "fit", "host")})
    th, diff = [], 0.0
    t0 = time.perf_counter()
    pts = host_points(base)
    t_points = time.perf_counter() - t0
    for i in range(host_trials):
        t0 = time.perf_counter()
        P = h3m.gmmnew_init(base, opt, seeds[i], pts)
        th.append(time.perf_counter() - t0)
        diff = max(diff, float(np.abs(P.m - posts[i].m).max() / np.abs(pts[0]).max()))
        note(name, "host trial", i, round(th[-1], 3))
    med = {k: float(np.median([p[k] for p in parts])) for k in ("points", "fit", "host")}
    per_trial = float(np.median(th))
    return dict(shape=name, points=int(pts[0].shape[0]), d=base.d, K=opt["K"], S=opt["S"], trials=len(seeds),
                device_seconds=spread(td), device_parts=med, replayed_trials=len(parts[-1]["replayed"]),
                esteps_min_max=[min(parts[-1]["esteps"]), max(parts[-1]["esteps"])],
                host_trials_timed=host_trials, host_seconds_per_trial=spread(th), host_points_seconds=t_points,
                host_seconds_all_trials_extrapolated=per_trial * len(seeds) + t_points,
                ratio_host_over_device=(per_trial * len(seeds) + t_points) / float(np.median(td)),
                max_centre_difference=diff)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bases", type=int, default=10000)
    ap.add_argument("--host-trials", type=int, default=1)
    ap.add_argument("--trials", type=int, default=16, help="device trials at the synthetic shape")
    ap.add_argument("--shapes", nargs="*", default=["demo", "synthetic"])
    a = ap.parse_args()
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
        print(json.dumps(one_shape(vb, "demo", base, opt, seeds, len(seeds), a.repeats, a.device)), flush=True)
    if "synthetic" in a.shapes:
        base = vb.synth_base_set(a.bases, 16, 8, 8, vb.COV_FULL, seed=1005)
        opt = vb.default_options(16, 8, 8, v0=10.0, seed=2000)
        seeds = [2000 + t for t in range(1, a.trials + 1)]
        print(json.dumps(one_shape(vb, "synthetic", base, opt, seeds, a.host_trials, a.repeats, a.device)), flush=True)


if __name__ == "__main__":
    main()
