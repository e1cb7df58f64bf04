#!/usr/bin/env python
"""Times the random trials' GMM fits of base-HMM learning on the host (one numpy EM per
trial, vbhmm_em.gmm_fit_randsample) against init="device" (random_gmm_batch: the same
draws, every fit in batched vbhmm_gmm_fit_batch calls), at the two shapes of
scripts/vbhmm_em_bench.py:

    (i)  the demo:  10 subjects x K = 1:3 x 50 trials (tests/golden/demo_fixations.npz);
    (ii) exprmt1's: --subjects seeded synthetic subjects of 25 sequences x T = 50,
                    K = 1:3 x 10 trials.

Per shape: vbhmm_learn_batch(engine="fused") end to end under init="host" and
init="device" with the seconds of its parts (gmm: draws + fits + replay rounds; init:
vbhmm_init + packing, or the gather of the device posteriors; device: the fused EM call;
unpack), the up-front draws alone, the first round's device fits alone, and the share of
the GMMs in each end-to-end time.  Host clock around a device synchronise, one warm-up per
init, the two alternating within a repeat, in one process.  One JSON line per shape.
Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pkgload  # noqa: E402
from vbhmm_em_bench import DEMO_VBOPT, KS, clock, demo_subjects, note, spread, synthetic_subjects  # noqa: E402


def draws_alone(subjects, opt):
    """The up-front draws of random_gmm_batch: numtrials row sets per (subject, K > 1)."""
    t0 = time.perf_counter()
    fits = []
    for s, d in enumerate(subjects):
        N = sum(a.shape[0] for a in d)
        for K in KS:
            if K == 1 or N <= K:
                continue
            rng = np.random.default_rng(opt["seed"])
            fits += [(s, K, rng.choice(N, K, replace=False), 0.0) for _ in range(int(opt["numtrials"]))]
    return time.perf_counter() - t0, fits


def one_shape(em, vbhmm, dev, name, subjects, opt, repeats, host_repeats):
    for init in ("host", "device"):  # warm-up
        em.vbhmm_learn_batch(subjects[:2], KS, opt, device=dev, engine="fused", init=init)
    t = dict(host=[], device=[])
    parts = dict(host=[], device=[])
    LL = {}
    for r in range(repeats):
        for init in ("host", "device"):
            if init == "host" and r >= host_repeats:
                continue
            part = {}
            dt, (_, L) = clock(lambda: em.vbhmm_learn_batch(subjects, KS, opt, device=dev, engine="fused",
                                                            init=init, timing=part), dev)
            t[init].append(dt)
            parts[init].append(part)
            LL[init] = L
            note(name, init, "repeat", r, "seconds", round(dt, 3), {k: round(v, 3) for k, v in part.items()})
    t_draw, fits = draws_alone(subjects, opt)
    sbt = vbhmm.SubjectBatch(subjects, 2, dev)
    copt, _ = em.vbhmm_clip_hyps(opt)
    hv = em.em_hyper_vector(copt, em._w0inv(copt, 2)[0])
    em.gmm_fit_batch(sbt, fits[:64], hyper=hv, KM=4)
    tf, st = [], None
    for _ in range(repeats):
        dt, (res, _) = clock(lambda: em.gmm_fit_batch(sbt, fits, hyper=hv, KM=4), dev)
        tf.append(dt)
        st = [g["status"] for g in res]
    med = {i: {k: float(np.median([p[k] for p in parts[i]])) for k in parts[i][0]} for i in parts}
    e2e = {i: float(np.median(t[i])) for i in t}
    return dict(shape=name, subjects=len(subjects), fits=len(fits), ill_conditioned_first_round=st.count("ill_conditioned"),
                host_seconds=spread(t["host"]), device_seconds=spread(t["device"]), host_parts=med["host"],
                device_parts=med["device"], draws_seconds=t_draw, device_fit_call_seconds=spread(tf),
                gmm_share_host=med["host"]["gmm"] / e2e["host"], gmm_share_device=med["device"]["gmm"] / e2e["device"],
                speedup_end_to_end=e2e["host"] / e2e["device"],
                max_rel_LL_difference=float(np.max(np.abs(LL["device"] - LL["host"]) / np.abs(LL["host"]))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=1, help="init='host' repeats at the synthetic shape")
    ap.add_argument("--subjects", type=int, default=2000)
    ap.add_argument("--shapes", nargs="*", default=["demo", "synthetic"])
    a = ap.parse_args()
    pkgload.load()
    from vbhem_amd import vbhmm, vbhmm_em as em
    if "demo" in a.shapes:
        opt = em.vbhmm_default_options(2, **dict(DEMO_VBOPT, numtrials=50))
        print(json.dumps(one_shape(em, vbhmm, a.device, "demo", demo_subjects(), opt, a.repeats, a.repeats)), flush=True)
    if "synthetic" in a.shapes:
        opt = em.vbhmm_default_options(2, **dict(DEMO_VBOPT, mu0=[160.0, 205.0], numtrials=10))
        print(json.dumps(one_shape(em, vbhmm, a.device, "synthetic", synthetic_subjects(a.subjects), opt, a.repeats,
                                   a.host_repeats)), flush=True)


if __name__ == "__main__":
    main()
