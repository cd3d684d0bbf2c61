#!/usr/bin/env python
"""Device time of the error image and the error planes beside the plain metric sums — ``kernels.error_image`` followed by
``kernels.error_accumulate`` (one launch each) and ``kernels.depth_metric_sums`` (two launches) — on one 352 x 1216 crop of a 375 x 1242
frame with the Garg rectangle.

The two alternate, call by call, in one process; each is timed by a pair of device events around it, after ``--warmup`` untimed rounds.
Ground truth: ``--density`` of the pixels hold a return in 1 .. 80 m (0.05 is about a LiDAR ground truth, 1.0 the worst case: two divisions
at every pixel of the rectangle); ``--radius`` 0 .. 3 is the dilation.  ``--batch n`` times the batched entry points for n images instead.
The last line is one JSON object: median and minimum in microseconds per call.  There is no earlier code path to compare with: the plain
metric call on the same inputs is the yardstick the numbers are read against."""
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


def frame(seed, density, H=375, W=1242):
    rng = np.random.default_rng(seed)
    depth = np.where(rng.random((H, W)) < density, rng.uniform(1.0, 80.0, (H, W)), 0.0)
    raw = np.minimum(depth * 256, 65535).astype(np.uint16)
    pred = rng.uniform(1.0, 80.0, (352, 1216)).astype(np.float32)
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return torch.from_numpy(raw).cuda(), torch.from_numpy(pred).cuda(), torch.from_numpy(bgr).cuda()


def main(argv=None):
    p = argparse.ArgumentParser(description='Device time of the error image and planes beside the plain metric sums')
    p.add_argument('--density', type=float, default=0.05)
    p.add_argument('--radius', type=int, default=1)
    p.add_argument('--batch', type=int, default=0, help='n images through the batched entry points; 0: the single-image ones')
    p.add_argument('--rounds', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), 'tools/benchmark_error.py measures the MI355X'
    n = max(args.batch, 1)
    frames = [frame(k, args.density) for k in range(n)]
    gts, bgrs = [f[0] for f in frames], [f[2] for f in frames]
    preds = torch.stack([f[1] for f in frames])
    tops, lefts = [375 - 352] * n, [int((1242 - 1216) / 2)] * n
    sums = torch.zeros(n, 10, device='cuda', dtype=torch.float64)
    plane_sum = torch.zeros(352, 1216, device='cuda', dtype=torch.float64)
    plane_count = torch.zeros(352, 1216, device='cuda', dtype=torch.int32).view(torch.uint32)
    out = torch.empty(n, 352, 1216, 3, device='cuda', dtype=torch.uint8)

    def errors_batch():
        K.error_image_batch(preds, gts, bgrs, tops, lefts, RECT, *LIMITS, 0.05, args.radius, 1, want_err=False, out=out)
        K.error_accumulate_batch(preds, gts, tops, lefts, RECT, *LIMITS, plane_sum, plane_count)

    def errors_single():
        K.error_image(preds[0], gts[0], bgrs[0], tops[0], lefts[0], RECT, *LIMITS, 0.05, args.radius, 1, want_err=False, out=out[0])
        K.error_accumulate(preds[0], gts[0], tops[0], lefts[0], RECT, *LIMITS, plane_sum, plane_count)
    if args.batch:
        calls = {'plain': lambda: K.depth_metric_sums_batch(preds, gts, tops, lefts, RECT, *LIMITS, sums), 'errors': errors_batch}
    else:
        calls = {'plain': lambda: K.depth_metric_sums(preds[0], gts[0], tops[0], lefts[0], RECT, *LIMITS, sums[0]), 'errors': errors_single}
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
    counted = int(sums[:, 0].sum().item())
    total = int(plane_count.view(torch.int32).sum().item())
    assert total == counted * (args.warmup + args.rounds), 'every call must add every counted pixel once'      # uniform(1, 80): all e finite
    print(json.dumps(dict(shape='352x1216 of 375x1242', density=args.density, radius=args.radius, batch=args.batch, rounds=args.rounds,
                          counted_pixels=counted,
                          us_per_call_median={k: round(statistics.median(v), 2) for k, v in spent.items()},
                          us_per_call_min={k: round(min(v), 2) for k, v in spent.items()})))


if __name__ == '__main__':
    main()
