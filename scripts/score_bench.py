#!/usr/bin/env python
"""Times score.ll_matrix (hmm_score_kernel) on the GPU at two shapes:

    64 HMMs x 100,000 sequences, K = 3, d = 2, T = 10
    1,000 HMMs x 10,000 sequences, K = 5, d = 4, T = 10

and prints one JSON line per shape: pair-steps per second (H N T / time) of one
batched launch, and the time of that launch against H single-HMM launches over
the same data (prepared sets built beforehand; outputs compared bit for bit).

Protocol: untimed batched launches for --settle-ms (the clocks settle), then
--windows windows that alternate the two variants; each window warms the
variant up once, then times --reps batched calls (a tenth as many loops) between
two device events (the stream is synchronised on the second).  The line reports
the median window and the range.  Needs a GPU; there is no CPU path.
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
import pkgload  # noqa: E402

SHAPES = [dict(H=64, N=100_000, K=3, d=2, T=10), dict(H=1000, N=10_000, K=5, d=4, T=10)]


def synth(vb, H, N, K, d, T, seed):
    """A packed full-covariance set of H K-state HMMs and N sequences of length T
    drawn around the states' means."""
    rng = np.random.default_rng(seed)
    prior = rng.dirichlet(np.ones(K), size=H)
    trans = rng.dirichlet(np.ones(K), size=(H, K))
    mean = rng.uniform(0, 5, (H, K, d))
    L = rng.normal(size=(H, K, d, d))
    cov = L @ L.transpose(0, 1, 3, 2) / d + 0.5 * np.eye(d)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    base = vb.BaseSet(torch.full((H,), K, dtype=torch.int32), t(prior), t(trans), t(mean), t(cov),
                      torch.full((H,), 1.0 / H, dtype=torch.float64), vb.COV_FULL)
    x = mean[rng.integers(0, H, N * T), rng.integers(0, K, N * T)] + rng.normal(0, 0.8, (N * T, d))
    return base, list(x.reshape(N, T, d))


def timed(fn, reps, dev):
    fn()  # warm-up of this variant
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=100, help="batched calls per window (the loop: a tenth)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=600.0)
    ap.add_argument("--scale", type=float, default=1.0, help="scale H and N (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_bench.py needs a GPU")
    vb = pkgload.load()
    from vbhem_amd import score
    from vbhem_amd.vbhmm import SequenceBatch
    dev = torch.device(args.device)
    for i, s in enumerate(SHAPES):
        H, N = max(1, int(s["H"] * args.scale)), max(1, int(s["N"] * args.scale))
        K, d, T = s["K"], s["d"], s["T"]
        base, data = synth(vb, H, N, K, d, T, seed=100 + i)
        batch = SequenceBatch(data, d, dev)
        hset = score.HmmSet(base, dev)
        singles = [score.HmmSet(base.shard(h, h + 1), dev) for h in range(H)]
        loop_out = torch.empty((H, N), dtype=torch.float64, device=dev)

        def batched():
            return score.ll_matrix(hset, batch, normalize=False)

        def looped():
            for h, one in enumerate(singles):
                loop_out[h] = score.ll_matrix(one, batch, normalize=False)[0]
            return loop_out

        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            batched()
            torch.cuda.synchronize(dev)
        tb, tl = [], []
        for _ in range(args.windows):
            ms, a = timed(batched, args.reps, dev)
            tb.append(ms)
            ms, b = timed(looped, max(1, args.reps // 10), dev)
            tl.append(ms)
        same = bool(torch.equal(a, b))
        mb, ml = float(np.median(tb)), float(np.median(tl))
        print(json.dumps(dict(
            shape=dict(H=H, N=N, K=K, d=d, T=T), kernel="hmm_score_kernel(ll)",
            batched_ms=round(mb, 4), batched_ms_range=[round(min(tb), 4), round(max(tb), 4)],
            pair_steps_per_s=round(H * N * T / (mb * 1e-3), 1),
            loop_ms=round(ml, 4), loop_ms_range=[round(min(tl), 4), round(max(tl), 4)],
            loop_over_batched=round(ml / mb, 3), outputs_equal=same,
            protocol=dict(settle_ms=args.settle_ms, windows=args.windows, reps=args.reps,
                          timer="device events around the calls"))), flush=True)


if __name__ == "__main__":
    main()
