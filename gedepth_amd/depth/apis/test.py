"""Evaluation loops (depth/apis/test.py:32-232): run the model with ``return_loss=False`` over a data loader and either
keep the predictions or reduce them to per-image metric tuples on the fly (``pre_eval``).  With ``show`` / ``out_dir`` each image's map
also goes through the model's ``show_result`` (a colorized image, or the raw ``.npy`` under ``format_only``)."""
import os.path as osp

import torch
import torch.distributed as dist

from ...mmrt.runner import get_dist_info


def _to_device(data, device):
    out = {}
    for k, v in data.items():
        if k == 'img_metas':
            out[k] = v
        elif isinstance(v, list):
            out[k] = [t.to(device, non_blocking=True) if torch.is_tensor(t) else t for t in v]
        else:
            out[k] = v.to(device, non_blocking=True) if torch.is_tensor(v) else v
    return out


def replace_str(s):
    """Output name of an image under ``out_dir`` (depth/apis/test.py of the reference): a leading '/' stripped, else '/' -> '_'."""
    if s[0] == '/':
        return s[1:]
    return s.replace('/', '_')


def _show_batch(model, data, result_depth, show, out_dir, format_only):
    depther = getattr(model, 'module', model)
    for meta, depth in zip(data['img_metas'][0], result_depth):
        name = meta['ori_filename']
        if not out_dir:
            out_file = None
        elif format_only:
            out_file = osp.join(out_dir, name[:-4] + '.npy')
        else:
            out_file = osp.join(out_dir, replace_str(name))
        depther.show_result(name, [depth], show=show, out_file=out_file, format_only=format_only)


def single_gpu_test(model, data_loader, pre_eval=False, format_only=False, format_args=None, device=None, *, show=False,
                    out_dir=None):
    """Returns a list with one entry per image: the metric tuple (``pre_eval``) or the ``(1, H, W)`` depth map.  ``show`` / ``out_dir``:
    ``show_result`` of every image's map, written to ``out_dir/replace_str(ori_filename)`` (``format_only``: the raw map as
    ``out_dir/<ori_filename without extension>.npy``)."""
    model.eval()
    dataset = data_loader.dataset
    device = device or next(model.parameters()).device
    results, idx = [], 0
    loader_indices = data_loader.batch_sampler
    for batch_indices, data in zip(loader_indices, data_loader):
        with torch.no_grad():
            result = model(return_loss=False, **_to_device(data, device))
        result_depth = list(result)                 # the maps, before format_results / pre_eval replace them
        if format_only:
            result = dataset.format_results(result, indices=batch_indices, **(format_args or {}))
        if pre_eval:
            result, _ = dataset.pre_eval(result, indices=list(batch_indices))
        results.extend(result)
        idx += len(result)
        if show or out_dir:
            _show_batch(model, data, result_depth, show, out_dir, format_only)
    return results


def multi_gpu_test(model, data_loader, pre_eval=False, format_only=False, format_args=None, device=None, *, show=False, out_dir=None):
    """Each rank evaluates its shard of a non-shuffled DistributedSampler; rank 0 receives the results in dataset order.  ``show`` /
    ``out_dir`` as in ``single_gpu_test``: every rank writes the files of its own shard."""
    part = single_gpu_test(model, data_loader, pre_eval, format_only, format_args, device, show=show, out_dir=out_dir)
    rank, world = get_dist_info()
    if world == 1:
        return part
    gathered = [None] * world
    dist.all_gather_object(gathered, part)
    if rank != 0:
        return None
    ordered = []
    for i in range(max(len(g) for g in gathered)):
        for g in gathered:                          # DistributedSampler deals indices round-robin
            if i < len(g):
                ordered.append(g[i])
    return ordered[:len(data_loader.dataset)]
