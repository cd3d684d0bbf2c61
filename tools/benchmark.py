#!/usr/bin/env python
"""Inference frames per second — CLI of the reference's tools/benchmark.py (config, checkpoint, --log-interval; 5 warm-up frames, 200
timed frames, ``torch.cuda.synchronize()`` around each frame, ``fps:`` lines), for three routes to the depth of one KITTI frame:

  reference  today's route: the host test pipeline (dataset ``__getitem__``: PIL decode, pe_165.npy, KB crop, flip copy, Normalize in
             numpy) and ``model(return_loss=False)`` = ``aug_test``, two batch-1 forwards launched from Python;
  engine     ``inference_depther(graph=False)``: PIL decode, ``ge_infer_front``, one batch-2 forward, ``ge_tta_merge``, eagerly;
  graph      ``inference_depther(graph=True)``: the same with forward + merge replayed from a hipGraph;
  batch      ``inference_depther(graph=True, batch=F)`` (``--batch F``, 2 .. 8): F frames per forward through the batched engine, the
             next batch's files decoding on a thread pool meanwhile.  Timed per list of ``--batch-frames`` files (the pool decodes ahead
             within a list) and reported per frame; the other modes run the same number of frames between two lists.

Every mode is timed from the image file to the depth map on the host.  The reference mode also reports the model call alone
(``reference_forward``), which is what the reference's tool times.  ``--mode all`` runs the three modes alternately, frame by frame, in
one process; with ``--batch F`` the batch mode alternates with them (``--mode graph,batch``: those two alone).  Frames: a seeded
synthetic 375 x 1242 tree with an analytic ground plane (default), or ``--data`` = a KITTI tree with
``input/<date>/pe/pe_165.npy`` (the frames of ``cfg.data.test``'s split).  The last line is one JSON object.
"""
import argparse
import json
import os
import os.path as osp
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

from gedepth_amd.depth.apis import inference_depther, init_depther  # noqa: E402
from gedepth_amd.mmrt.config import Config  # noqa: E402

MODES = ('reference', 'engine', 'graph')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Depth benchmark a model (single-frame inference)')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', nargs='?', default=None, help='checkpoint file (default: the initial weights)')
    p.add_argument('--log-interval', type=int, default=50, help='interval of logging')
    p.add_argument('--mode', default='all', help='all, or a comma-separated list of reference, engine, graph, batch')
    p.add_argument('--batch', type=int, default=0, help='F = 2 .. 8: also time the batched engine with F frames per forward (mode batch)')
    p.add_argument('--batch-frames', type=int, default=0, help='files per timed list of the batch mode (default 5 F)')
    p.add_argument('--bf16', action='store_true', help='bf16 autocast forward')
    p.add_argument('--data', default=None, help='KITTI tree (data_root of cfg.data.test) instead of the synthetic frames')
    p.add_argument('--frames', type=int, default=200, help='timed frames per mode')
    p.add_argument('--seed', type=int, default=0)
    args = p.parse_args(argv)
    args.modes = list(MODES) + (['batch'] if args.batch else []) if args.mode == 'all' else args.mode.split(',')
    if set(args.modes) - set(MODES + ('batch',)):
        p.error(f'--mode: {args.mode}')
    if ('batch' in args.modes) != bool(args.batch) or (args.batch and not 2 <= args.batch <= 8):
        p.error('mode batch needs --batch F with F in 2 .. 8, and --batch F a mode list that holds batch')
    args.batch_frames = args.batch_frames or 5 * args.batch
    return args


def make_synthetic_tree(root, frames=8, seed=0):
    """``root/input/<date>/<drive>/image_02/data/*.png`` (seeded uint8 375 x 1242 frames), ``root/input/<date>/pe/pe_165.npy`` (an
    analytic ground plane: camera 1.65 m above a flat road, horizon at row 172.854, focal 721.5377) and ``root/split.txt``."""
    rng = np.random.default_rng(seed)
    H, W, date = 375, 1242, '2011_09_26'
    drive = f'{date}_drive_0001_sync'
    img_dir = osp.join(root, 'input', date, drive, 'image_02', 'data')
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(osp.join(root, 'input', date, 'pe'), exist_ok=True)
    v = np.arange(H, dtype=np.float64).reshape(H, 1)
    pe = np.where(v > 173.0, 1.65 * 721.5377 / np.maximum(v - 172.854, 1e-6), -5.0) * np.ones((1, W))
    np.save(osp.join(root, 'input', date, 'pe', 'pe_165.npy'), pe)
    lines = []
    for f in range(frames):
        name = f'{f:010d}.png'
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(osp.join(img_dir, name))
        lines.append(f'{date}/{drive}/image_02/data/{name} {drive}/proj_depth/groundtruth/image_02/{name} 721.5377')    # no depth file is read
    split = osp.join(root, 'split.txt')
    with open(split, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return split


def main(argv=None):
    args = parse_args(argv)
    from gedepth_amd.depth.apis.test import _to_device
    from gedepth_amd.depth.datasets import build_dataset
    from gedepth_amd.depth.datasets.loader import collate
    assert torch.cuda.is_available(), 'tools/benchmark.py measures the MI355X'
    torch.backends.cudnn.benchmark = False
    cfg = Config.fromfile(args.config)
    tmp = None
    if args.data is None:
        tmp = tempfile.TemporaryDirectory()
        cfg.data.test.data_root = tmp.name
        cfg.data.test.split = make_synthetic_tree(tmp.name, seed=args.seed)
    else:
        cfg.data.test.data_root = args.data
    torch.manual_seed(args.seed)
    model = init_depther(cfg, args.checkpoint, device='cuda:0')
    ds = build_dataset(cfg.data.test, dict(test_mode=True))
    files = [osp.join(ds.img_dir, info['filename']) for info in ds.img_infos]
    modes = args.modes
    # the batch mode is timed per list of L files; the per-frame modes then run L frames per round, so every mode sees the same files
    L = args.batch_frames if args.batch else 1
    num_warmup = (5 + L - 1) // L * L
    total = num_warmup + (args.frames + L - 1) // L * L
    timed = total - num_warmup
    spent = {m: 0.0 for m in modes}
    forward_only = 0.0
    amp = dict(device_type='cuda', dtype=torch.bfloat16, enabled=args.bf16)

    def run(mode, i):
        nonlocal forward_only
        idx = i % len(files)
        if mode == 'reference':
            data = _to_device(collate([ds[idx]]), 'cuda:0')
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad(), torch.autocast(**amp):
                model(return_loss=False, rescale=True, **data)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        if mode == 'batch':
            inference_depther(model, [files[(i + k) % len(files)] for k in range(L)], bf16=args.bf16, graph=True, batch=args.batch)
            return 0.0
        inference_depther(model, files[idx], bf16=args.bf16, graph=mode == 'graph')
        return 0.0

    for i0 in range(0, total, L):
        for mode in modes:
            for i in ([i0] if mode == 'batch' else range(i0, i0 + L)):
                torch.cuda.synchronize()
                start = time.perf_counter()
                fwd = run(mode, i)
                torch.cuda.synchronize()
                elapsed = time.perf_counter() - start
                if i >= num_warmup:
                    spent[mode] += elapsed
                    if mode == 'reference':
                        forward_only += fwd
                    done = i + (L if mode == 'batch' else 1)
                    if done % args.log_interval == 0:
                        fps = (done - num_warmup) / spent[mode]
                        print(f'[{mode}] Done image [{done:<3}/ {total}], fps: {fps:.2f} img / s')
    args.frames = timed
    result = dict(config=osp.basename(args.config), frames=args.frames, warmup=num_warmup, bf16=args.bf16,
                  source='synthetic 375x1242' if args.data is None else args.data, fps={}, ms_per_frame={})
    for mode in modes:
        fps = args.frames / spent[mode]
        print(f'[{mode}] Overall fps: {fps:.2f} img / s')
        result['fps'][mode] = round(fps, 3)
        result['ms_per_frame'][mode] = round(1e3 * spent[mode] / args.frames, 3)
    if 'reference' in modes:
        result['fps']['reference_forward'] = round(args.frames / forward_only, 3)
        result['ms_per_frame']['reference_forward'] = round(1e3 * forward_only / args.frames, 3)
    if 'graph' in modes:
        result['captures'] = model._ge_inferencers[bool(args.bf16)].captures
    if 'batch' in modes:
        eng = model._ge_inferencers[(bool(args.bf16), args.batch)]
        result.update(batch=args.batch, batch_frames=L, batch_captures=eng.captures, batch_replays=eng.replays)
    print(json.dumps(result))
    if tmp is not None:
        tmp.cleanup()


if __name__ == '__main__':
    main()
