#!/usr/bin/env python
"""Evaluate / run a depther — CLI of the reference's tools/test.py:21-68 (config, checkpoint, --eval, --options, --out,
--format-only, --show, --show-dir, --eval-options, --launcher), plus --ply-dir, --ground-dir and --scene-dir.

With a KITTI tree at ``cfg.data.test.data_root`` this is the Eigen-split protocol of the reference: test pipeline with
flip test-time augmentation, ``forward_test`` (``return_loss=False``), KB crop + Garg crop, per-image metrics, nan-mean
summary (gedepth_amd/depth/apis/test.py, gedepth_amd/depth/datasets/kitti.py).  ``--synthetic N`` runs the same model
protocol on N synthetic KITTI-shaped inputs instead (no dataset needed).

Any of ``--out`` / ``--format-only`` / ``--show`` / ``--show-dir`` / ``--ply-dir``, or ``--launcher pytorch``, runs the reference's dataset route:
``--show-dir DIR`` writes one colorized depth image per test image (``BaseDepther.show_result``), ``--format-only --show-dir DIR`` the
raw maps as ``.npy``, ``--out FILE.pkl`` pickles the results list (metric tuples with ``--eval``, else the maps) on rank 0, and
``--launcher pytorch`` (tools/dist_test.sh) evaluates one shard per rank with ``multi_gpu_test``.  ``--ply-dir DIR`` writes one coloured
point cloud per test image, ``DIR/<ori_filename with .ply>`` (binary PLY; ``BaseDepther.save_point_cloud`` with the image's ``cam_intrinsic``
meta and its KB-crop offsets); it combines with ``--show-dir``.

``--ground-dir DIR`` writes the ground embedding's maps of every test image: ``DIR/<name>_attention.png`` (where the model relies on the
ground, over [0, 1]), ``<name>_slope.png`` (the predicted slope over [-5, 5] degrees; adaptive models) and ``<name>_ground.png`` (the
slope-adjusted ground depth), or with ``--format-only`` one ``<name>.npz`` of the raw arrays (``BaseDepther.show_ground``).  The frames go
through the graphed engine (``DepthInferencer.ground_maps``): alone, or with ``--eval ... --device-eval`` in the same pass; with a host-loop
``--eval`` it raises.

``--scene-dir DIR`` (KITTI protocol) writes one scene cloud per test image, ``DIR/<ori_filename with .ply>``: the prediction's points coloured
from the image, the ground prior's in red, the LiDAR ground truth's in green and the slope-adjusted ground plane's in blue, in one binary
PLY whose header names the layers (``DepthInferencer.scene_points``, ``depth.utils.write_scene_ply``).  The frames go through the graphed
engine; it runs alone, without ``--eval`` or any other output.

``--device-eval`` (with ``--eval`` and ``--synthetic 0``; KITTI or DDAD protocol) evaluates on the device: frames go through the graphed
engine (flip-TTA for KITTI, the single view for DDAD) and each map is reduced to its metric sums by a HIP kernel, so no map is copied to the
host (``single_gpu_test(device_eval=True)``).  ``--eval-batch F`` (2 .. 8; KITTI or DDAD protocol) runs F frames per forward and one metric
call per batch, with the next batch's image PNGs and ground truths (KITTI: PNGs, DDAD: compressed ``.npz``) decoding on a thread pool meanwhile.

``--strata [EDGE ...]`` (with ``--eval --device-eval``; KITTI protocol) also reduces every map per distance bin of the ground truth (bare
``--strata``: edges 20 40 60 metres) and per on / off ground class: a LiDAR return is on the ground when it lies within
``--strata-ground-tol`` (default 0.1) times the ground depth of the plane the front end was fed; ``--strata-no-ground`` keeps the bins only.
The table is printed after the usual summary; ``--strata-out FILE.npz`` stores ``rows`` (N, S, 10), ``names`` and ``edges``.

``--error-dir DIR`` (with ``--eval --device-eval``; KITTI protocol, any ``--eval-batch``) shows where in the picture the error is: one
error picture per test image, ``DIR/<name in the split, '/' as '_'>`` — every LiDAR return in the colour of its abs-rel error's band
(blue below ``--error-tau`` / 16, red from ``--error-tau``, default 0.05), drawn ``2 * --error-radius + 1`` pixels wide over the darkened
frame — and for the split ``DIR/summary.npz`` (per-pixel ``sum`` and ``count`` of the abs-rel error, ``tau``, ``rect``, ``frames``) and
``DIR/mean_abs_rel.png``; the mean per eight image rows is printed.  ``--error-no-pictures`` keeps the split's summary only.  The metrics
printed are those without ``--error-dir``.

``--prior-sweep`` (with ``--eval --device-eval``; KITTI protocol, one device, ``--eval-batch 1``, without ``--strata`` / ``--error-dir`` /
``--ground-dir``) evaluates every frame under perturbed ground priors in one forward (include/gedepth_sweep.h): the calibrated plane, the
plane of a camera pitched by each ``--sweep-pitch D`` degrees (default -1 -0.5 0.5 1; positive brings the ground closer), of a camera
``--sweep-height S`` times as high (default none) and, unless ``--sweep-no-drop``, no prior at all; at most eight variants.  The usual
summary is the baseline's; the table after it has one line per variant with its differences to the baseline.  ``--sweep-out FILE.npz``
stores ``rows`` (N, V, 10), ``names``, ``pitch_deg``, ``height_scale`` and ``cam_height``.
"""
import argparse
import os
import os.path as osp
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

from gedepth_amd.depth.core import eval_metrics  # noqa: E402
from gedepth_amd.depth.datasets.synthetic import synthetic_batch  # noqa: E402
from gedepth_amd.depth.models import build_depther  # noqa: E402
from gedepth_amd.mmrt.checkpoint import load_checkpoint  # noqa: E402
from gedepth_amd.mmrt.config import Config, DictAction  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='depth test (and eval) a model')
    p.add_argument('config')
    p.add_argument('checkpoint', nargs='?', default=None)
    p.add_argument('--eval', nargs='+', default=None)
    p.add_argument('--options', nargs='+', default=None)
    p.add_argument('--synthetic', type=int, default=2, help='N synthetic inputs; 0 = evaluate cfg.data.test')
    p.add_argument('--flip-tta', action='store_true')
    p.add_argument('--bf16', action='store_true', help='bf16 autocast inference')
    p.add_argument('--device-eval', action='store_true',
                   help='with --eval and --synthetic 0: the graphed inference engine and the metric-sum kernel instead of the host loop')
    p.add_argument('--eval-batch', type=int, default=1,
                   help='with --device-eval (KITTI or DDAD protocol): frames per forward, 1 .. 8; the next batch\'s files decode on a thread pool')
    p.add_argument('--strata', nargs='*', type=float, default=None, metavar='EDGE',
                   help='with --eval --device-eval (KITTI protocol): metrics per distance bin (edges in metres; none given: 20 40 60) and '
                        'on / off ground')
    p.add_argument('--strata-ground-tol', type=float, default=0.1,
                   help='a return is on the ground when |gt - g| <= T * g for the ground depth g of its pixel, T in [0, 1]')
    p.add_argument('--strata-no-ground', action='store_true', help='distance bins only')
    p.add_argument('--strata-out', help='.npz file that receives the per-image sums of every stratum (rows, names, edges)')
    p.add_argument('--error-dir', help='with --eval --device-eval (KITTI protocol): directory that receives one error picture per test image '
                                       '(every LiDAR return in the colour of its abs-rel error), summary.npz and mean_abs_rel.png')
    p.add_argument('--error-tau', type=float, default=0.05, help='the abs-rel error at the middle of the ten colour bands, in (0, 1]')
    p.add_argument('--error-radius', type=int, default=1, help='a return is drawn 2 R + 1 pixels wide, R in 0 .. 3')
    p.add_argument('--error-no-pictures', action='store_true', help='the split\'s summary only, no picture per image')
    p.add_argument('--prior-sweep', action='store_true',
                   help='with --eval --device-eval (KITTI protocol, one device): every frame under perturbed ground priors in one forward')
    p.add_argument('--sweep-pitch', nargs='+', type=float, default=None, metavar='D',
                   help='the pitch errors in degrees (default: -1 -0.5 0.5 1); positive brings the ground closer')
    p.add_argument('--sweep-height', nargs='+', type=float, default=None, metavar='S', help='camera-height scales in [0.5, 2] (default: none)')
    p.add_argument('--sweep-no-drop', action='store_true', help='leave out the variant without a prior')
    p.add_argument('--sweep-out', help='.npz file that receives rows (N, V, 10), names, pitch_deg, height_scale and cam_height')
    p.add_argument('--out', help='output result file in pickle format (.pkl / .pickle), written by rank 0')
    p.add_argument('--format-only', action='store_true',
                   help='format the results (dataset.format_results) without evaluating; with --show-dir the raw maps are saved as .npy')
    p.add_argument('--show', action='store_true', help='show results (no display support here: warns and shows nothing)')
    p.add_argument('--show-dir', help='directory where the colorized depth maps (or, with --format-only, the raw .npy maps) are saved')
    p.add_argument('--ply-dir', help='directory where one coloured point cloud per test image is saved as a binary .ply')
    p.add_argument('--ground-dir', help='directory where the ground attention / slope / ground-depth pictures of every test image (or, with '
                                        '--format-only, one .npz of the raw maps) are saved; runs the graphed engine')
    p.add_argument('--scene-dir', help='directory where one scene cloud per test image (prediction, ground prior, ground truth and adjusted '
                                       'ground plane in one binary .ply) is saved; KITTI protocol, runs the graphed engine, alone')
    p.add_argument('--eval-options', nargs='+', default=None, help='k=v options for evaluate / format_results')
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='none', help='job launcher (pytorch: torch.distributed.run)')
    p.add_argument('--local_rank', '--local-rank', type=int, default=0)
    p.add_argument('--gpu-collect', action='store_true',
                   help='accepted for compatibility, no effect: multi_gpu_test always gathers with all_gather_object')
    p.add_argument('--tmpdir', help='accepted for compatibility, no effect: multi_gpu_test collects no temporary files')
    args = p.parse_args(argv)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    if args.scene_dir:
        clash = [flag for flag, on in (('--eval', args.eval), ('--out', args.out), ('--format-only', args.format_only), ('--show', args.show),
                                       ('--show-dir', args.show_dir), ('--ply-dir', args.ply_dir), ('--ground-dir', args.ground_dir),
                                       ('--device-eval', args.device_eval), ('--error-dir', args.error_dir)) if on]
        if clash:
            raise ValueError(f'--scene-dir cannot be combined with {" / ".join(clash)}: the scene clouds come from an engine loop of their '
                             'own that returns no results')
    if args.eval and args.format_only:
        raise ValueError('--eval and --format-only cannot be both specified')
    if args.device_eval and (not args.eval or args.synthetic != 0 or args.show or args.show_dir or args.ply_dir):
        raise ValueError('--device-eval needs --eval and --synthetic 0, and cannot be combined with --show / --show-dir / --ply-dir')
    if args.eval_batch != 1 and not args.device_eval:
        raise ValueError('--eval-batch needs --device-eval: it batches the device evaluation loop')
    if not 1 <= args.eval_batch <= 8:
        raise ValueError(f'--eval-batch must be in 1 .. 8, got {args.eval_batch}')
    if args.strata is None:
        if args.strata_out or args.strata_no_ground:
            raise ValueError('--strata-out / --strata-no-ground need --strata')
    else:
        if not (args.eval and args.device_eval):
            raise ValueError('--strata needs --eval and --device-eval: the strata are reduced by the device evaluation loop')
        if args.strata_out is not None and not args.strata_out.endswith('.npz'):
            raise ValueError('--strata-out must be an .npz file')
        args.strata = args.strata or [20.0, 40.0, 60.0]
    if args.error_dir is None:
        if args.error_no_pictures or args.error_tau != 0.05 or args.error_radius != 1:
            raise ValueError('--error-tau / --error-radius / --error-no-pictures need --error-dir')
    else:
        if not (args.eval and args.device_eval):
            raise ValueError('--error-dir needs --eval and --device-eval: the error maps are reduced by the device evaluation loop')
        error_maps(args)                                               # ValueError for a tau or radius outside its range
    if not args.prior_sweep:
        if args.sweep_pitch is not None or args.sweep_height is not None or args.sweep_no_drop or args.sweep_out:
            raise ValueError('--sweep-pitch / --sweep-height / --sweep-no-drop / --sweep-out need --prior-sweep')
    else:
        if not (args.eval and args.device_eval):
            raise ValueError('--prior-sweep needs --eval and --device-eval: the variants are the slots of the device evaluation loop\'s engine')
        clash = [flag for flag, on in (('--eval-batch', args.eval_batch != 1), ('--strata', args.strata is not None),
                                       ('--error-dir', args.error_dir), ('--ground-dir', args.ground_dir),
                                       ('--launcher pytorch', args.launcher == 'pytorch')) if on]
        if clash:
            raise ValueError(f'--prior-sweep cannot be combined with {" / ".join(clash)}: the sweep runs alone, on one device (its baseline '
                             'row is the ordinary result)')
        if args.sweep_out is not None and not args.sweep_out.endswith('.npz'):
            raise ValueError('--sweep-out must be an .npz file')
        prior_sweep(args)                                              # ValueError for a pitch or scale outside its range
    if args.eval_batch != 1 and args.ground_dir:
        raise ValueError('--eval-batch > 1 cannot be combined with --ground-dir: the ground maps come from the single-frame engine')
    if args.ground_dir and args.eval and not args.device_eval:
        raise ValueError('--ground-dir with --eval needs --device-eval: the ground maps come from the graphed engine, not from the host loop')
    if args.ground_dir and (args.show or args.show_dir or args.ply_dir or args.out):
        raise ValueError('--ground-dir cannot be combined with --show / --show-dir / --ply-dir / --out: those are outputs of the host loop')
    if args.out is not None and not args.out.endswith(('.pkl', '.pickle')):
        raise ValueError('The output file must be a pkl file.')
    return args


def strata_spec(args):
    """The ``StrataSpec`` of ``--strata`` and its companions, or None."""
    if args.strata is None:
        return None
    from gedepth_amd.depth.core import StrataSpec
    return StrataSpec(args.strata, not args.strata_no_ground, args.strata_ground_tol)


def report_strata(args, dataset, spec, rows):
    """The table after the usual summary, and ``--strata-out``."""
    dataset.evaluate_strata(rows, spec)
    if args.strata_out:
        os.makedirs(osp.dirname(osp.abspath(args.strata_out)), exist_ok=True)
        np.savez(args.strata_out, rows=rows, names=np.array(spec.names(dataset.min_depth, dataset.max_depth)), edges=np.array(spec.edges))
        print(f'writing strata sums to {args.strata_out}')


def prior_sweep(args):
    """The ``PriorSweep`` of ``--prior-sweep`` and its companions, or None."""
    if not args.prior_sweep:
        return None
    from gedepth_amd.depth.core import PriorSweep
    return PriorSweep((-1.0, -0.5, 0.5, 1.0) if args.sweep_pitch is None else args.sweep_pitch, args.sweep_height or (), not args.sweep_no_drop)


def report_sweep(args, dataset, sweep, rows):
    """The table after the usual summary, and ``--sweep-out``."""
    dataset.evaluate_sweep(rows, sweep)
    if args.sweep_out:
        os.makedirs(osp.dirname(osp.abspath(args.sweep_out)), exist_ok=True)
        np.savez(args.sweep_out, rows=rows, names=np.array(sweep.names), pitch_deg=np.array(sweep.pitch_deg),
                 height_scale=np.array(sweep.height_scale), cam_height=np.float64(sweep.cam_height))
        print(f'writing prior-sweep sums to {args.sweep_out}')


def error_maps(args):
    """The ``ErrorMaps`` of ``--error-dir`` and its companions, or None."""
    if args.error_dir is None:
        return None
    from gedepth_amd.depth.core import ErrorMaps
    return ErrorMaps(None if args.error_no_pictures else args.error_dir, args.error_tau, args.error_radius)


def report_errors(args, errors):
    """``summary.npz`` and ``mean_abs_rel.png`` into ``--error-dir``, and the mean abs-rel error per band of eight image rows."""
    errors.save(args.error_dir)
    mean, count = errors.rows(8)
    lines = [f'Error maps ({errors.frames} images; abs-rel per 8 image rows):', '    rows |  abs_rel |  returns']
    lines += [f'{8 * k:4d}-{min(8 * k + 7, 351):3d} | {m:8.4f} | {int(c):8d}' for k, (m, c) in enumerate(zip(mean, count))]
    print('\n'.join(lines))
    print(f'writing error maps to {args.error_dir}')


def run_dataset(args, cfg):
    """The reference's dataset route: (distributed) evaluation of cfg.data.test with --out / --format-only / --show / --show-dir."""
    from gedepth_amd.depth.apis.test import multi_gpu_test, single_gpu_test
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    from gedepth_amd.mmrt.ddp import init_dist
    from gedepth_amd.mmrt.runner import get_dist_info
    data_root = cfg.data.test.get('data_root')
    if not (data_root and osp.isdir(data_root)):
        sys.exit(f'tools/test.py: cfg.data.test.data_root = {data_root!r} is not a directory; the dataset route (--out, --format-only, '
                 '--show, --show-dir, --launcher pytorch) evaluates the test split there (set it with --options data.test.data_root=...)')
    eval_kwargs = DictAction.parse(args.eval_options)
    distributed = args.launcher == 'pytorch'
    if distributed:
        init_dist(cfg.get('dist_params', {}).get('backend', 'nccl'))
    dataset = build_dataset(cfg.data.test, dict(test_mode=True))
    loader = build_dataloader(dataset, 1, cfg.data.workers_per_gpu, dist=distributed, shuffle=False)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    if args.checkpoint:
        load_checkpoint(model, args.checkpoint, map_location='cpu')
    model = model.cuda().eval()
    model.cfg = cfg
    test = multi_gpu_test if distributed else single_gpu_test
    spec, rows, errors, sweep = strata_spec(args), None, error_maps(args), prior_sweep(args)
    own = {} if sweep is None else dict(prior_sweep=sweep)               # one device only (parse_args refuses it with --launcher pytorch)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=args.bf16):
        results = test(model, loader, pre_eval=args.eval is not None, format_only=args.format_only, format_args=eval_kwargs,
                       show=args.show, out_dir=args.show_dir, device_eval=args.device_eval, ply_dir=args.ply_dir,
                       ground_dir=args.ground_dir, eval_batch=args.eval_batch, scene_dir=args.scene_dir, strata=spec, errors=errors, **own)
    rank, _ = get_dist_info()
    if (spec is not None or sweep is not None) and results is not None:
        results, rows = results
    if rank == 0:
        if args.out:
            os.makedirs(osp.dirname(osp.abspath(args.out)), exist_ok=True)
            print(f'\nwriting results to {args.out}')
            with open(args.out, 'wb') as fh:
                pickle.dump(results, fh)
        if args.eval:
            dataset.evaluate(results, args.eval, **eval_kwargs)
            if sweep is not None:
                report_sweep(args, dataset, sweep, rows)
            if spec is not None:
                report_strata(args, dataset, spec, rows)
            if errors is not None:
                report_errors(args, errors)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def main():
    args = parse_args()
    cfg = Config.fromfile(args.config)
    if args.options:
        cfg.merge_from_dict(DictAction.parse(args.options))
    cfg.model.pretrained = None
    cfg.model.train_cfg = None
    if args.out or args.format_only or args.show or args.show_dir or args.ply_dir or args.ground_dir or args.scene_dir or \
            args.launcher == 'pytorch':
        return run_dataset(args, cfg)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    if args.checkpoint:
        load_checkpoint(model, args.checkpoint, map_location='cpu')
    model = model.cuda().eval()
    data_root = cfg.data.test.get('data_root')
    if args.synthetic <= 0 or (args.synthetic == 2 and data_root and osp.isdir(data_root) and args.eval):
        from gedepth_amd.depth.apis.test import single_gpu_test
        from gedepth_amd.depth.datasets import build_dataloader, build_dataset
        dataset = build_dataset(cfg.data.test, dict(test_mode=True))
        loader = build_dataloader(dataset, 1, cfg.data.workers_per_gpu, dist=False, shuffle=False)
        model.cfg = cfg
        spec, errors, sweep = strata_spec(args), error_maps(args), prior_sweep(args)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=args.bf16):
            results = single_gpu_test(model, loader, pre_eval=True, device_eval=args.device_eval, eval_batch=args.eval_batch, strata=spec,
                                      errors=errors, prior_sweep=sweep)
        if spec is not None or sweep is not None:
            results, rows = results
        dataset.evaluate(results)
        if sweep is not None:
            report_sweep(args, dataset, sweep, rows)
        if spec is not None:
            report_strata(args, dataset, spec, rows)
        if errors is not None:
            report_errors(args, errors)
        return
    res = []
    for i in range(args.synthetic):
        b = synthetic_batch(1, 352, 1120, seed=100 + i, device='cuda', valid_fraction=0.05)
        imgs, metas = [b['img']], [b['img_metas']]
        if args.flip_tta:
            m = dict(b['img_metas'][0], flip=True, flip_direction='horizontal')
            imgs.append(b['img'].flip(3)); metas.append([m])
        with torch.no_grad():
            pred = model(imgs, metas, return_loss=False, pe_ori_point=[None] * len(imgs))[0]
        gt = b['depth_gt'][0, 0].cpu().numpy()
        res.append(eval_metrics(gt, np.clip(pred[0], 1e-3, 80)))
    for k in res[0]:
        print(f'{k}: {np.nanmean([r[k] for r in res]):.4f}')


if __name__ == '__main__':
    main()
