#!/usr/bin/env python
"""Device time of the stratified metric sums beside the plain ones — ``kernels.depth_metric_sums_strata`` (eight strata: edges 20 40 60,
on / off ground) and ``kernels.depth_metric_sums``, two launches each — on one 352 x 1216 crop of a 375 x 1242 frame.

The two calls alternate, call by call, in one process; each is timed by a pair of device events around it, after ``--warmup`` untimed
rounds.  Ground truth: ``--density`` of the pixels hold a return in 1 .. 80 m (0.05 is about a LiDAR ground truth, 1.0 the worst case: a
logarithm at every pixel), half of those below the horizon on the analytic ground plane.  ``--batch n`` times the batched entry points
for n images instead.  The last line is one JSON object: median and minimum in microseconds per call."""
import argparse
import json
import os.path as osp
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

from gedepth_amd import kernels as K  # noqa: E402

RECT = (int(0.40810811 * 352), int(0.99189189 * 352), int(0.03594771 * 1216), int(0.96405229 * 1216))        # Garg
LIMITS = (256, 1e-3, 80)
EDGES = (20.0, 40.0, 60.0)


def frame(seed, density, H=375, W=1242):
    rng = np.random.default_rng(seed)
    v = np.arange(H, dtype=np.float64).reshape(H, 1)
    plane = np.where(v > 173.0, 1.65 * 721.5377 / np.maximum(v - 172.854, 1e-6), -5.0) * np.ones((1, W))
    depth = np.where(rng.random((H, W)) < density, rng.uniform(1.0, 80.0, (H, W)), 0.0)
    on = (depth > 0) & (plane > 0) & (rng.random((H, W)) < 0.5)
    depth = np.where(on, plane * rng.uniform(0.95, 1.05, (H, W)), depth)
    raw = np.minimum(depth * 256, 65535).astype(np.uint16)
    pred = rng.uniform(1.0, 80.0, (352, 1216)).astype(np.float32)
    return torch.from_numpy(raw).cuda(), torch.from_numpy(pred).cuda(), torch.from_numpy(plane.astype(np.float32)).cuda()


def main(argv=None):
    p = argparse.ArgumentParser(description='Device time of the stratified metric sums beside the plain ones')
    p.add_argument('--density', type=float, default=0.05)
    p.add_argument('--batch', type=int, default=0, help='n images through the batched entry points; 0: the single-image ones')
    p.add_argument('--rounds', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), 'tools/benchmark_strata.py measures the MI355X'
    n = max(args.batch, 1)
    frames = [frame(k, args.density) for k in range(n)]
    gts, grounds = [f[0] for f in frames], [f[2] for f in frames]
    preds = torch.stack([f[1] for f in frames])
    tops, lefts = [375 - 352] * n, [int((1242 - 1216) / 2)] * n
    sums = torch.zeros(n, 10, device='cuda', dtype=torch.float64)
    rows = torch.zeros(n, 8, 10, device='cuda', dtype=torch.float64)
    if args.batch:
        calls = {'plain': lambda: K.depth_metric_sums_batch(preds, gts, tops, lefts, RECT, *LIMITS, sums),
                 'strata': lambda: K.depth_metric_sums_strata_batch(preds, gts, tops, lefts, RECT, *LIMITS, rows, EDGES, grounds, 0.1)}
    else:
        calls = {'plain': lambda: K.depth_metric_sums(preds[0], gts[0], tops[0], lefts[0], RECT, *LIMITS, sums[0]),
                 'strata': lambda: K.depth_metric_sums_strata(preds[0], gts[0], tops[0], lefts[0], RECT, *LIMITS, rows[0], EDGES, grounds[0], 0.1)}
    spent = {name: [] for name in calls}
    for rnd in range(args.warmup + args.rounds):
        for name, call in calls.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            end.record()
            end.synchronize()
            if rnd >= args.warmup:
                spent[name].append(1e3 * start.elapsed_time(end))
    assert torch.equal(rows[:, :, :4].sum(1), sums[:, :4]), 'the strata must add up to the plain counts'
    print(json.dumps(dict(shape='352x1216 of 375x1242', strata=8, density=args.density, batch=args.batch, rounds=args.rounds,
                          counted_pixels=[int(v) for v in sums[:, 0].tolist()],
                          us_per_call_median={k: round(statistics.median(v), 2) for k, v in spent.items()},
                          us_per_call_min={k: round(min(v), 2) for k, v in spent.items()})))


if __name__ == '__main__':
    main()
