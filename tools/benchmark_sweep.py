#!/usr/bin/env python
"""Times of the prior sweep (include/gedepth_sweep.h), each next to the route it replaces, from one process.

Kernel: ``ge_infer_front_sweep`` with V = 5 and V = 8 variants on one 375 x 1242 frame (views = 2, the KITTI crop) against the composition
the library offers without it: V planes formed by the torch expression of the rule on the device, then ``ge_infer_front_batch`` with V table
rows that all point at the one uploaded frame.  Device events surround each route, the two routes alternate call by call, and the
median of ``--calls`` (default 200) is reported in microseconds; the composition's time includes its torch operations.

Loop: ms per frame of ``single_gpu_test(pre_eval=True, device_eval=True, prior_sweep=...)`` at V = 5 (two pitches, one height scale, no
prior) against V runs of the plain ``device_eval`` loop (``eval_batch=1``) over the same synthetic split, as tools/benchmark_eval.py
builds it (image and ground-truth PNGs of two sizes, decoded from files in every pass).  Round 0 warms up (the engines capture their
graphs there) and is not counted; the two settings then alternate for ``--rounds`` (default 3) rounds; medians.  The V plain runs
evaluate the SAME prior V times: they stand for the cost of V passes, not for their result.

The last line is one JSON object."""
import argparse
import json
import os.path as osp
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

from benchmark_eval import make_tree  # noqa: E402
from gedepth_amd import kernels as K  # noqa: E402
from gedepth_amd.depth.apis import init_depther  # noqa: E402
from gedepth_amd.depth.apis.test import single_gpu_test  # noqa: E402
from gedepth_amd.depth.core import PriorSweep  # noqa: E402
from gedepth_amd.depth.datasets import build_dataloader, build_dataset  # noqa: E402
from gedepth_amd.mmrt.config import Config  # noqa: E402

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def torch_plane(pe, c, s, drop):
    """The rule of include/gedepth_sweep.h as torch operations on the device plane ``pe``."""
    if drop:
        return torch.zeros_like(pe)
    if c == 0.0 and s == 1.0:
        return pe
    q = 1.0 / pe + c
    return torch.where(pe > 0, torch.where(q > 0, s / q, torch.zeros_like(pe)), pe)


def time_kernel(V, calls, seed=0):
    rng = np.random.default_rng(seed)
    H, W, Hc, Wc = 375, 1242, 352, 1216
    top, left = H - Hc, int((W - Wc) / 2)
    bgr = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    v = np.arange(H, dtype=np.float64).reshape(H, 1)
    pe = torch.from_numpy((np.where(v > 173.0, 1.65 * 721.5377 / np.maximum(v - 172.854, 1e-6), -5.0) * np.ones((1, W))).astype(np.float32)).cuda()
    pitches = (-1.0, -0.5, 0.5, 1.0) if V == 5 else (-1.5, -1.0, -0.5, 0.5, 1.0, 1.5)
    rows = PriorSweep(pitches, drop=V != 5).table()
    assert len(rows) == V
    out_a = torch.zeros(2 * V, 5, Hc, Wc, device='cuda')
    out_b = torch.zeros(2 * V, 5, Hc, Wc, device='cuda')

    def sweep():
        K.infer_front_sweep(bgr, pe, rows, out_a, top, left, MEAN, STD)

    def composition():
        planes = [torch_plane(pe, *r) for r in rows]
        K.infer_front_batch([bgr] * V, planes, out_b, [top] * V, [left] * V, MEAN, STD)
    spent = {'sweep': [], 'composition': []}
    for call in range(calls + 10):                                    # ten warm-up pairs
        for name, fn in (('sweep', sweep), ('composition', composition)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if call >= 10:
                spent[name].append(1e3 * t0.elapsed_time(t1))
    same = float((out_a.view(torch.int32) == out_b.view(torch.int32)).float().mean())
    return dict(V=V, sweep_us=round(statistics.median(spent['sweep']), 1), composition_us=round(statistics.median(spent['composition']), 1),
                sweep_us_min=round(min(spent['sweep']), 1), composition_us_min=round(min(spent['composition']), 1),
                written_MB=round(2 * V * 5 * Hc * Wc * 4 / 1e6, 1), equal_fraction=same)


def main(argv=None):
    p = argparse.ArgumentParser(description='Time the prior sweep\'s kernel and loop next to the routes they replace')
    p.add_argument('config')
    p.add_argument('checkpoint', nargs='?', default=None)
    p.add_argument('--calls', type=int, default=200)
    p.add_argument('--frames', type=int, default=32)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--no-loop', action='store_true', help='the kernel pair only')
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), 'tools/benchmark_sweep.py measures the MI355X'
    result = dict(config=osp.basename(args.config), calls=args.calls, kernel=[time_kernel(V, args.calls, args.seed) for V in (5, 8)])
    for k in result['kernel']:
        print(f'[kernel V={k["V"]}] sweep {k["sweep_us"]} us, composition {k["composition_us"]} us (medians of {args.calls})')
    if not args.no_loop:
        sweep = PriorSweep(pitch_deg=(-1.0, 1.0), height_scale=(1.05,), drop=True)
        V = sweep.count
        cfg = Config.fromfile(args.config)
        with tempfile.TemporaryDirectory() as root:
            cfg.data.test.data_root, cfg.data.test.split = root, make_tree(root, args.frames, args.seed)
            torch.manual_seed(args.seed)
            model = init_depther(cfg, args.checkpoint, device='cuda:0')
            ds = build_dataset(cfg.data.test, dict(test_mode=True))
            loader = build_dataloader(ds, 1, 0, dist=False, shuffle=False)
            assert len(ds) == args.frames and V == 5
            spent = {'sweep': [], 'plain_x_V': []}
            for rnd in range(args.rounds + 1):
                for name in spent:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if name == 'sweep':
                        _, rows = single_gpu_test(model, loader, pre_eval=True, device_eval=True, prior_sweep=sweep)
                    else:
                        for _ in range(V):
                            single_gpu_test(model, loader, pre_eval=True, device_eval=True)
                    elapsed = time.perf_counter() - t0
                    if rnd:
                        spent[name].append(1e3 * elapsed / args.frames)
                        print(f'[loop {name}] round {rnd}: {spent[name][-1]:.2f} ms / frame')
            result['loop'] = dict(V=V, frames=args.frames, rounds=args.rounds, names=sweep.names,
                                  source='synthetic 375x1242 + 370x1224, image and ground-truth PNGs',
                                  ms_per_frame_median={k: round(statistics.median(v), 3) for k, v in spent.items()},
                                  ms_per_frame_min={k: round(min(v), 3) for k, v in spent.items()},
                                  abs_rel={n: float(np.nanmean(rows[:, i, 4] / rows[:, i, 0])) for i, n in enumerate(sweep.names)})
    print(json.dumps(result))


if __name__ == '__main__':
    main()
