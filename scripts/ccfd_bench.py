#!/usr/bin/env python
"""Times CCFD clustering on the GPU:

  1. the fused distance (ccfd.distance_matrix's kernels) against the unfused one,
     0.5 (K + K') of score.kld_matrix's steps (ll_matrix, the own-likelihood gather,
     the padded segment mean), at two shapes:
         1,000 HMMs x 10 trials, K = 3, d = 2, T = 10
         4,000 HMMs x 25 trials, K = 5, d = 4, T = 10
     Both sides start from the same prepared HmmSet and SequenceBatch, so the host's
     packing of the trials is in neither.  The unfused side is skipped, and the line
     says so, when its [H][N_total] matrix and padded gather do not fit.
  2. ccfd.myccfd_from_dist (the search: 19 CCFD calls) on the device engine against the
     numpy engine, on a planted Euclidean matrix of 4,000 points.

One JSON line each.  Protocol as scripts/score_bench.py: untimed calls for --settle-ms,
then --windows windows that alternate the variants; each window warms its variant up
once and times at least --reps calls, and at least --window-ms of them, between two
device events (the search: wall clock, one call).  The line reports the median window and the range.  Needs a GPU.
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
from score_bench import synth, timed  # noqa: E402

SHAPES = [dict(H=1000, per=10, K=3, d=2, T=10), dict(H=4000, per=25, K=5, d=4, T=10)]


def planted_matrix(N, G, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn((G, 2), generator=g, dtype=torch.float64) * 8
    pts = centres[torch.arange(N) % G] + torch.randn((N, 2), generator=g, dtype=torch.float64)
    D = torch.cdist(pts.to(dev), pts.to(dev))
    D = torch.triu(D, 1)
    return (D + D.T).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=600.0)
    ap.add_argument("--window-ms", type=float, default=250.0, help="least timed work per window")
    ap.add_argument("--scale", type=float, default=1.0, help="scale H (rehearsal)")
    ap.add_argument("--search-points", type=int, default=4000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ccfd_bench.py needs a GPU")
    vb = pkgload.load()
    from vbhem_amd import ccfd, score
    from vbhem_amd.vbhmm import SequenceBatch
    dev = torch.device(args.device)
    for i, s in enumerate(SHAPES):
        H, per, K, d, T = max(2, int(s["H"] * args.scale)), s["per"], s["K"], s["d"], s["T"]
        N = H * per
        base, data = synth(vb, H, N, K, d, T, seed=300 + i)
        batch, hset, counts = SequenceBatch(data, d, dev), score.HmmSet(base, dev), [per] * H
        owner = torch.repeat_interleave(torch.arange(H, device=dev), per)
        cols = torch.arange(N, device=dev)

        def fused():
            return ccfd._distance_batch(hset, batch, counts)[0]

        def unfused():
            ll = score.ll_matrix(hset, batch, True)
            Kl = score._segment_mean(ll[owner, cols][None, :] - ll, counts).T
            S = 0.5 * (Kl + Kl.T)
            S.fill_diagonal_(0.0)
            return S

        # [H][N] doubles, and the padded gather's [H][H][per] three times over
        need = 8 * (H * N + 3 * H * H * per)
        fits = need < 0.6 * torch.cuda.mem_get_info(dev)[0]
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            fused()
            torch.cuda.synchronize(dev)
        tf, tu, a, b = [], [], None, None
        reps = max(args.reps, int(np.ceil(args.window_ms / timed(fused, 1, dev)[0])))
        for _ in range(args.windows):
            ms, a = timed(fused, reps, dev)
            tf.append(ms)
            if fits:
                ms, b = timed(unfused, reps, dev)
                tu.append(ms)
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fused()
        torch.cuda.synchronize(dev)
        peak_f = torch.cuda.max_memory_allocated(dev) - before
        line = dict(shape=dict(H=H, trials=per, K=K, d=d, T=T), fused_ms=round(float(np.median(tf)), 3),
                    fused_ms_range=[round(min(tf), 3), round(max(tf), 3)], fused_peak_bytes=int(peak_f),
                    pair_steps_per_s=round(H * N * T / (float(np.median(tf)) * 1e-3), 1))
        if fits:
            torch.cuda.reset_peak_memory_stats(dev)
            unfused()
            torch.cuda.synchronize(dev)
            big = np.abs(b.cpu().numpy()).max()
            line.update(unfused_ms=round(float(np.median(tu)), 3),
                        unfused_ms_range=[round(min(tu), 3), round(max(tu), 3)],
                        unfused_peak_bytes=int(torch.cuda.max_memory_allocated(dev) - before),
                        unfused_over_fused=round(float(np.median(tu)) / float(np.median(tf)), 3),
                        max_abs_difference_over_max=float((a - b).abs().max().cpu()) / float(big))
        else:
            line.update(unfused="skipped: needs about %.1f GB, does not fit" % (need / 1e9))
        line["protocol"] = dict(settle_ms=args.settle_ms, windows=args.windows, reps=reps,
                                timer="device events around the calls")
        print(json.dumps(line), flush=True)
        del batch, hset, a, b

    P = max(16, int(args.search_points * args.scale))
    D = planted_matrix(P, 8, dev)
    Dh = D.cpu().numpy()
    out = {}
    for name, arg in (("device", D), ("numpy", Dh)):
        try:
            ccfd.myccfd_from_dist(arg) if name == "device" else None   # warm-up of the kernels
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = ccfd.myccfd_from_dist(arg)
            torch.cuda.synchronize(dev)
            out[name] = (time.perf_counter() - t0, res)
        except ccfd.NoSingularPoints as e:
            out[name] = (float("nan"), None)
            print("search on the %s engine raised: %s" % (name, e), file=sys.stderr)
    line = dict(search=dict(points=P, groups=8, calls=19),
                device_engine_s=round(out["device"][0], 4), numpy_engine_s=round(out["numpy"][0], 4))
    if out["device"][1] and out["numpy"][1]:
        rd, rn = out["device"][1]["ccfd_result"], out["numpy"][1]["ccfd_result"]
        line.update(numpy_over_device=round(out["numpy"][0] / out["device"][0], 2), NCLUST=rd["NCLUST"],
                    labels_equal=bool(np.array_equal(rd["cl"], rn["cl"])), timer="wall clock, one call each")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
