#!/usr/bin/env python
"""Device time of the gradient accumulation kernel beside the pair of passes it replaces, and of a training iteration with and without
accumulation.

Kernel part (``--sizes``, default the Swin-T and the Swin-L arena): ``ge_grad_accum`` with ``first=0`` (12 B per element) with and without
the norm, and with ``first=1`` (8 B per element), alternated call by call in one process with the pair the norm-producing call replaces on
the same buffers — ``torch.add(acc, g, out=acc)`` followed by ``ge_sumsq(acc)``.  Each call is timed by a pair of device events, after
``--warmup`` untimed rounds; a repeat is ``--rounds`` alternated rounds and yields one median per variant, and ``--repeats`` repeats give the
spread of those medians, which is the margin any comparison between two variants has to clear.  GB/s are algorithmic bytes over the median,
to be read beside the 6.29 TB/s of a float4 copy on this chip.

Step part (``--step-rounds`` > 0): Swin-T vanilla, 8 x 352 x 1120, bf16, channels-last, eager: four iterations with ``cumulative_iters`` = 1
(an optimizer step each) and four with 4 (``accumulate`` each, one step) alternate on one model; wall clock around each block of four with
the device fenced, ms per iteration.

The last line is one JSON object."""
import argparse
import json
import os
import os.path as osp
import statistics
import sys
import time

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')        # as bench.py and tools/train.py start the runtime

import torch  # noqa: E402

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from gedepth_amd import hip  # noqa: E402
from gedepth_amd.accum_kernels import grad_accum  # noqa: E402

COPY_PEAK_GBS = 6290.0             # measured float4 copy on the MI355X


def kernel_part(n, rounds, warmup, repeats):
    acc = torch.randn(n, device='cuda')
    g = torch.randn(n, device='cuda') * 1e-3
    out = torch.zeros(1, device='cuda', dtype=torch.float64)

    def pair():
        torch.add(acc, g, out=acc)
        hip.call('ge_sumsq', hip.ptr(acc), n, hip.ptr(out), hip.stream())
    calls = {'first': (8, lambda: grad_accum(acc, g, True)),
             'add': (12, lambda: grad_accum(acc, g, False)),
             'add+norm': (12, lambda: grad_accum(acc, g, False, out)),
             'torch.add': (12, lambda: torch.add(acc, g, out=acc)),
             'torch.add, ge_sumsq': (16, pair)}
    medians = {name: [] for name in calls}
    for rep in range(repeats):
        spent = {name: [] for name in calls}
        for rnd in range(warmup + rounds):
            for name, (_, call) in calls.items():
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                call()
                end.record()
                end.synchronize()
                if rnd >= warmup:
                    spent[name].append(1e3 * start.elapsed_time(end))
        for name in calls:
            medians[name].append(statistics.median(spent[name]))
    assert bool(torch.isfinite(out).all())
    res = {}
    for name, (nbytes, _) in calls.items():
        med = statistics.median(medians[name])
        res[name] = dict(us_median=round(med, 2), us_medians_of_repeats=[round(m, 2) for m in medians[name]],
                         us_spread=round(max(medians[name]) - min(medians[name]), 2), bytes_per_element=nbytes,
                         GBps=round(n * nbytes / (med * 1e-6) / 1e9, 1), of_copy_peak=round(n * nbytes / (med * 1e-6) / 1e9 / COPY_PEAK_GBS, 3))
    return res


def step_part(rounds, warmup, n_accum=4, batch_size=8, H=352, W=1120):
    from gedepth_amd.depth.datasets.synthetic import synthetic_batch
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.depth.models.utils import to_channels_last
    from gedepth_amd.mmrt.config import Config
    from gedepth_amd.mmrt.optim import build_optimizer
    from gedepth_amd.mmrt.tuning import use_miopen_find_db, use_tuned_gemms
    torch.backends.cudnn.benchmark = bool(use_miopen_find_db())
    use_tuned_gemms('load')
    cfg = Config.fromfile(osp.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_v.py'))
    cfg.model.pretrained = None
    torch.manual_seed(1234)
    model = build_depther(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    model = model.to('cuda').train()
    to_channels_last(model)
    opt = build_optimizer(model, cfg.optimizer, cfg.optimizer_config.get('grad_clip'))
    batch = synthetic_batch(batch_size, H, W, seed=1234, device='cuda')

    def block(n):
        """Four iterations; n = 1: an optimizer step after each, n = 4: accumulate after each and one step."""
        for pos in range(n_accum):
            opt.zero_grad()
            with torch.autocast('cuda', dtype=torch.bfloat16):
                out = model.train_step(batch, opt)
            if n == 1:
                out['loss'].backward()
                opt.step()
            else:
                (out['loss'] / n).backward()
                opt.accumulate(last=pos == n - 1)
                if pos == n - 1:
                    opt.step()
    spent = {1: [], n_accum: []}
    for rnd in range(warmup + rounds):
        for n in spent:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            block(n)
            torch.cuda.synchronize()
            if rnd >= warmup:
                spent[n].append(1e3 * (time.perf_counter() - t0) / n_accum)
    return dict(workload=f'depthformer_swint_v, {batch_size} x {H} x {W}, bf16, nhwc, eager', arena=int(opt.arena.numel), rounds=rounds,
                ms_per_iteration_median={f'cumulative_iters={n}': round(statistics.median(v), 3) for n, v in spent.items()},
                ms_per_iteration_min={f'cumulative_iters={n}': round(min(v), 3) for n, v in spent.items()},
                ms_per_iteration_max={f'cumulative_iters={n}': round(max(v), 3) for n, v in spent.items()})


def main(argv=None):
    p = argparse.ArgumentParser(description='Device time of the gradient accumulation kernel and of an accumulated training iteration')
    p.add_argument('--sizes', type=int, nargs='*', default=[53_500_000, 277_135_808], help='arena sizes of the kernel part, in elements')
    p.add_argument('--rounds', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--step-rounds', type=int, default=10, help='blocks of four iterations per mode in the step part; 0 skips it')
    p.add_argument('--step-warmup', type=int, default=3)
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), 'tools/benchmark_accum.py measures the MI355X'
    hip.lib()
    res = dict(copy_peak_GBps=COPY_PEAK_GBS, rounds=args.rounds, repeats=args.repeats, kernel={})
    for n in args.sizes:
        res['kernel'][str(n)] = kernel_part(n, args.rounds, args.warmup, args.repeats)
        torch.cuda.empty_cache()
    if args.step_rounds > 0:
        res['step'] = step_part(args.step_rounds, args.step_warmup)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
