#!/usr/bin/env python
"""Time ``kernels.scene_points`` against what the library offered before it, in one process on one MI355X, the two alternated call by call.

Inputs at KITTI's size, synthetic and seeded: a (352, 1216) f32 prediction and slope-adjusted ground plane, a (375, 1242) f32 ground prior,
a (375, 1242) uint16 ground truth and the (375, 1242, 3) uint8 frame, all on the device, as the engine holds them after a frame.

  scene        one ``scene_points`` call with four layers; then the counts are read and the records are sliced to the total.
  composition  ATen crop + convert of the ground truth (``.float() / 256``) and crop of the ground prior, four ``depth_points`` calls, four
               count read-backs, ``torch.cat`` of the four slices.  (Its three ground layers stay white: painting them would be more ATen work.)

Per route two figures: ``device`` — device events around the launches alone (crop / convert and the kernels; no read-back), and ``wall`` —
a host clock around the whole route up to one hole-free record tensor and its counts, ending in a synchronise.  The two routes' records
are compared once (x y z and the prediction's colours equal).  Prints one line per round and a JSON summary line."""
import argparse
import json
import os.path as osp
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

from gedepth_amd import kernels as K  # noqa: E402

H, W, HF, WF = 352, 1216, 375, 1242
TOP, LEFT = HF - H, int((WF - W) / 2)
INTR = (721.5377, 721.5377, 609.5593 - LEFT, 172.854 - TOP)
DMIN, DMAX = 1e-3, 80.0


def inputs(seed):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(0.5, 100.0, (H, W)).astype(np.float32)
    v = np.arange(HF, dtype=np.float64).reshape(HF, 1)
    prior = (np.where(v > 173.0, 1.65 * 721.5377 / np.maximum(v - 172.854, 1e-6), -5.0) * np.ones((1, WF))).astype(np.float32)
    gt = np.where(rng.random((HF, WF)) < 0.05, rng.uniform(1.0, 80.0, (HF, WF)) * 256, 0).astype(np.uint16)      # LiDAR density
    adjusted = np.where(rng.random((H, W)) < 0.5, rng.uniform(3.0, 90.0, (H, W)), 0.0).astype(np.float32)
    frame = rng.integers(0, 256, (HF, WF, 3), dtype=np.uint8)
    return [torch.from_numpy(a).cuda() for a in (pred, prior, gt, adjusted, frame)]


def scene_launch(pred, prior, gt, adjusted, frame):
    L = K.SceneLayer
    layers = [L(pred, 'f32', DMIN, DMAX), L(prior, 'f32', DMIN, DMAX, (255, 0, 0), TOP, LEFT), L(gt, 'u16', DMIN, DMAX, (0, 255, 0), TOP, LEFT, 256.0),
              L(adjusted, 'f32', DMIN, DMAX, (0, 0, 255))]
    return K.scene_points(layers, *INTR, H, W, frame, TOP, LEFT)


def scene_finish(out):
    records, counts = out
    c = counts.tolist()
    return records[:c[4]], c[:4]


def composition_launch(pred, prior, gt, adjusted, frame):
    g = gt[TOP:TOP + H, LEFT:LEFT + W].float() / 256.0
    p = prior[TOP:TOP + H, LEFT:LEFT + W].contiguous()
    return [K.depth_points(pred, *INTR, frame, TOP, LEFT, DMIN, DMAX), K.depth_points(p, *INTR, None, 0, 0, DMIN, DMAX),
            K.depth_points(g, *INTR, None, 0, 0, DMIN, DMAX), K.depth_points(adjusted, *INTR, None, 0, 0, DMIN, DMAX)]


def composition_finish(outs):
    c = [int(count.item()) for _, count in outs]
    return torch.cat([records[:n] for (records, _), n in zip(outs, c)]), c


ROUTES = {'scene': (scene_launch, scene_finish), 'composition': (composition_launch, composition_finish)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--calls', type=int, default=200, help='timed calls per route and round')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    data = inputs(0)
    a, ca = scene_finish(scene_launch(*data))
    b, cb = composition_finish(composition_launch(*data))
    pa, pb = a.cpu().numpy(), b.cpu().numpy()
    assert ca == cb and np.array_equal(pa[:, :12], pb[:, :12]) and np.array_equal(pa[:ca[0]], pb[:cb[0]]), 'the two routes disagree'
    for launch, finish in ROUTES.values():
        for _ in range(args.warmup):
            finish(launch(*data))
    torch.cuda.synchronize()
    device = {k: [] for k in ROUTES}
    wall = {k: [] for k in ROUTES}
    for r in range(args.rounds):
        dev = {k: 0.0 for k in ROUTES}
        host = {k: 0.0 for k in ROUTES}
        for _ in range(args.calls):
            for name, (launch, finish) in ROUTES.items():                 # alternated call by call
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                out = launch(*data)
                e1.record()
                finish(out)
                torch.cuda.synchronize()
                host[name] += time.perf_counter() - t0
                dev[name] += e0.elapsed_time(e1)
        for name in ROUTES:
            device[name].append(dev[name] / args.calls * 1e3)
            wall[name].append(host[name] / args.calls * 1e6)
            print(f'[{name}] round {r + 1}: device {device[name][-1]:.1f} us, wall {wall[name][-1]:.1f} us per call', flush=True)
    print(json.dumps({'size': [H, W], 'layers': 4, 'points': ca, 'calls': args.calls, 'rounds': args.rounds,
                      'device_us_median': {k: round(statistics.median(v), 1) for k, v in device.items()},
                      'wall_us_median': {k: round(statistics.median(v), 1) for k, v in wall.items()}}))


if __name__ == '__main__':
    main()
