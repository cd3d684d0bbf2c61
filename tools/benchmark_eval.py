#!/usr/bin/env python
"""Time of the device evaluation loop per frame — ``single_gpu_test(pre_eval=True, device_eval=True, eval_batch=F)``, what
``tools/test.py --eval ... --device-eval --eval-batch F`` and ``tools/train.py --device-eval`` run — for several F in one process.

Frames: a seeded synthetic KITTI tree, 16 image / ground-truth PNG pairs of two sizes (375 x 1242 and 370 x 1224, each date with its
analytic ground plane), listed ``--frames`` times in the split, so every pass decodes ``--frames`` image and ``--frames`` ground-truth PNGs
from files.  Round 0 warms up (the engines capture their graphs there) and is not counted; the settings then alternate, pass by pass, for
``--rounds`` rounds.  A pass is timed from the call to the returned list of metric tuples (the loop ends with its one synchronising copy).
The last line is one JSON object: per F the median and the minimum of the passes in ms per frame.  ``--strata`` times every F twice, without
and with ``strata=StrataSpec()`` (eight strata: four distance bins, on / off ground), alternated pass by pass; the keys of the second are
``"<F>+strata"``.  ``--errors`` adds two more settings per F: ``errors=ErrorMaps()`` (the split's error planes only; ``"<F>+errors"``) and
``errors=ErrorMaps(dir)`` (also one error picture per frame, copied to the host per batch and encoded as PNG on the thread pool;
``"<F>+pictures"``).

With a DDAD config the tree is DDAD's at the real geometry: 8 frames of 1216 x 1936 as PNG, four of CAMERA_01 and four of CAMERA_05, each
with a ground truth of about 1 % valid pixels written with ``np.savez_compressed`` (as tools/preprocess_data_ddad.py writes its arrays) and
one ``ddad_pe.npz`` per camera; consecutive split entries alternate between the cameras, so a batch mixes them.  Every pass decodes
``--frames`` PNGs and inflates ``--frames`` ``.npz`` files.  ``--strata`` / ``--errors`` are KITTI's."""
import argparse
import json
import os
import os.path as osp
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

from gedepth_amd.depth.apis import init_depther  # noqa: E402
from gedepth_amd.depth.apis.test import single_gpu_test  # noqa: E402
from gedepth_amd.depth.datasets import build_dataloader, build_dataset  # noqa: E402
from gedepth_amd.mmrt.config import Config  # noqa: E402


def make_tree(root, frames, seed=0, unique=16):
    rng = np.random.default_rng(seed)
    files = []
    for date, (H, W) in (('2011_09_26', (375, 1242)), ('2011_09_28', (370, 1224))):
        drive = f'{date}_drive_0001_sync'
        img_dir = osp.join(root, 'input', date, drive, 'image_02', 'data')
        gt_dir = osp.join(root, 'gt_depth', drive, 'proj_depth', 'groundtruth', 'image_02')
        for d in (img_dir, gt_dir, osp.join(root, 'input', date, 'pe')):
            os.makedirs(d, exist_ok=True)
        v = np.arange(H, dtype=np.float64).reshape(H, 1)
        np.save(osp.join(root, 'input', date, 'pe', 'pe_165.npy'),
                np.where(v > 173.0, 1.65 * 721.5377 / np.maximum(v - 172.854, 1e-6), -5.0) * np.ones((1, W)))
        for f in range(unique // 2):
            name = f'{f:010d}.png'
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(osp.join(img_dir, name))
            depth = np.where(rng.random((H, W)) < 0.05, rng.uniform(1.0, 80.0, (H, W)), 0.0)      # about as sparse as a LiDAR ground truth
            Image.fromarray((depth * 256).astype(np.uint16)).save(osp.join(gt_dir, name))
            files.append(f'{date}/{drive}/image_02/data/{name} {drive}/proj_depth/groundtruth/image_02/{name} 721.5377')
    split = osp.join(root, 'split.txt')
    with open(split, 'w') as fh:
        fh.write('\n'.join(files[i % len(files)] for i in range(frames)) + '\n')
    return split


def make_ddad_tree(root, frames, seed=0, unique=8, size=(1216, 1936), cameras=('CAMERA_01', 'CAMERA_05')):
    """``unique`` frames of ``size``, dealt round-robin to ``cameras``, listed ``frames`` times -> the split file."""
    rng = np.random.default_rng(seed)
    H, W = size
    v = np.arange(H, dtype=np.float64).reshape(H, 1)
    lines = []
    for cam in cameras:
        os.makedirs(osp.join(root, 'pe', cam), exist_ok=True)
        pe = np.where(v > 0.45 * H, 1.5 * 0.9 * W / np.maximum(v - 0.45 * H, 1e-6), -3.0) * np.ones((1, W))      # a ground plane below the horizon
        np.savez(osp.join(root, 'pe', cam, 'ddad_pe.npz'), pe=pe.astype(np.float32))
    for f in range(unique):
        cam = cameras[f % len(cameras)]
        rgb_dir, d_dir = osp.join(root, '000001', 'rgb', cam), osp.join(root, '000001', 'depth', cam)
        os.makedirs(rgb_dir, exist_ok=True)
        os.makedirs(d_dir, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(osp.join(rgb_dir, f'{f}.png'))
        depth = np.where(rng.random((H, W)) < 0.01, rng.uniform(1.0, 150.0, (H, W)), 0.0).astype(np.float32)      # about 1 % valid
        np.savez_compressed(osp.join(d_dir, f'{f}.npz'), depth=depth)
        lines.append(f'{osp.join(rgb_dir, f"{f}.png")} {osp.join(d_dir, f"{f}.npz")}')
    split = osp.join(root, 'ddad_split.txt')
    with open(split, 'w') as fh:
        fh.write('\n'.join(lines[i % len(lines)] for i in range(frames)) + '\n')
    return split


def main(argv=None):
    p = argparse.ArgumentParser(description='Time the device evaluation loop per frame for several --eval-batch settings')
    p.add_argument('config')
    p.add_argument('checkpoint', nargs='?', default=None)
    p.add_argument('--eval-batch', type=int, nargs='+', default=[1, 2, 4, 8])
    p.add_argument('--frames', type=int, default=96)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--bf16', action='store_true')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--swin-t', action='store_true',
                   help='run the config\'s model at Swin-T width (the scaling of depthformer_swint_v.py): the DDAD configs ship at Swin-L only')
    p.add_argument('--strata', action='store_true', help='time every setting without and with the stratified sums (StrataSpec())')
    p.add_argument('--errors', action='store_true',
                   help='time every setting without and with the error maps: ErrorMaps() (planes only) and ErrorMaps(dir) (a PNG per frame)')
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), 'tools/benchmark_eval.py measures the MI355X'
    cfg = Config.fromfile(args.config)
    if args.swin_t:
        swin_t, rev = [64, 96, 192, 384, 768], [768, 384, 192, 96, 64]
        cfg.model.backbone.update(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24])
        cfg.model.neck.update(in_channels=swin_t, out_channels=swin_t)
        cfg.model.decode_head.update(in_channels=swin_t, up_sample_channels=swin_t)
        for neck in ('pe_mask_neck', 'dynamic_pe_neck'):
            if cfg.model.get(neck) is not None:
                cfg.model[neck].in_channels = rev
    ddad = any(t['type'] == 'LoadDDADImageFromFile' for t in cfg.data.test.pipeline)
    if ddad and (args.strata or args.errors):
        raise ValueError('--strata / --errors time KITTI settings: the DDAD protocol has neither')
    with tempfile.TemporaryDirectory() as root:
        if ddad:
            cfg.data.test.split = make_ddad_tree(root, args.frames, args.seed)        # full paths: a DDAD split has no data_root
            cfg.data.test.cameras = ['CAMERA_01', 'CAMERA_05']
            for t in cfg.data.test.pipeline:
                if t['type'] == 'LoadDDADImageFromFile':
                    t['pe_root'] = osp.join(root, 'pe')
        else:
            cfg.data.test.data_root, cfg.data.test.split = root, make_tree(root, args.frames, args.seed)
        torch.manual_seed(args.seed)
        model = init_depther(cfg, args.checkpoint, device='cuda:0')
        ds = build_dataset(cfg.data.test, dict(test_mode=True))
        loader = build_dataloader(ds, 1, 0, dist=False, shuffle=False)
        assert len(ds) == args.frames
        from gedepth_amd.depth.core import ErrorMaps, StrataSpec
        pictures = osp.join(root, 'error_pictures')
        extras = [('', None, None)] + ([('+strata', StrataSpec(), None)] if args.strata else [])
        extras += [('+errors', None, lambda: ErrorMaps()), ('+pictures', None, lambda: ErrorMaps(pictures))] if args.errors else []
        settings = [(f'{F}{tag}' if tag else F, F, spec, errors) for F in args.eval_batch for tag, spec, errors in extras]
        spent = {key: [] for key, _, _, _ in settings}
        summary = {}
        for rnd in range(args.rounds + 1):
            for key, F, spec, errors in settings:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.autocast('cuda', dtype=torch.bfloat16, enabled=args.bf16):
                    res = single_gpu_test(model, loader, pre_eval=True, device_eval=True, eval_batch=F, strata=spec,
                                          errors=errors and errors())
                elapsed = time.perf_counter() - t0
                res = res[0] if spec else res
                if rnd:
                    spent[key].append(1e3 * elapsed / args.frames)
                    print(f'[eval_batch={key}] round {rnd}: {spent[key][-1]:.2f} ms / frame')
                summary[key] = float(np.nanmean([r[3] for r in res]))                # abs_rel, to see that the settings evaluate the same
        result = dict(config=osp.basename(args.config), swin_t=args.swin_t, frames=args.frames, rounds=args.rounds, bf16=args.bf16,
                      source='synthetic 1216x1936 of two cameras, image PNGs and compressed .npz ground truth' if ddad else
                      'synthetic 375x1242 + 370x1224, image and ground-truth PNGs',
                      ms_per_frame_median={str(F): round(statistics.median(v), 3) for F, v in spent.items()},
                      ms_per_frame_min={str(F): round(min(v), 3) for F, v in spent.items()},
                      abs_rel={str(F): summary[F] for F in spent})
        print(json.dumps(result))


if __name__ == '__main__':
    main()
