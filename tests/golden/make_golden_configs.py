"""Record how the REFERENCE's own depthformer config files resolve through this repository's config loader.

    python tests/golden/make_golden_configs.py REFERENCE_ROOT        -> tests/golden/reference_configs.json

Each of the reference's ``configs/depthformer/{depthformer_v,depthformer_a,depthformer_v_ddad,depthformer_a_ddad}.py`` is loaded
byte-unchanged with ``gedepth_amd.mmrt.config.Config.fromfile`` (``_base_`` inheritance, ``_delete_``, the reference's own base
files) and the resolved sections that tests/test_boundary_cpu.py compares are stored as JSON.  Tuples are stored as
``{"__tuple__": [...]}`` so that the comparison keeps telling a tuple from a list.  The output is data only: the resolved settings.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NAMES = ['depthformer_v.py', 'depthformer_a.py', 'depthformer_a_ddad.py', 'depthformer_v_ddad.py']
KEYS = ['model', 'optimizer', 'optimizer_config', 'lr_config', 'runner', 'checkpoint_config', 'evaluation', 'log_config', 'dist_params',
        'workflow', 'data']
OUT = os.path.join(ROOT, 'tests', 'golden', 'reference_configs.json')


def tag(o):
    if isinstance(o, dict):
        assert all(isinstance(k, str) for k in o), o
        return {k: tag(v) for k, v in o.items()}
    if isinstance(o, tuple):
        return {'__tuple__': [tag(v) for v in o]}
    if isinstance(o, list):
        return [tag(v) for v in o]
    assert o is None or isinstance(o, (str, int, float, bool)), type(o)
    return o


def main():
    from gedepth_amd.mmrt.config import Config
    ref = sys.argv[1]
    out = {}
    for name in NAMES:
        d = Config.fromfile(os.path.join(ref, 'configs', 'depthformer', name)).to_dict()
        out[name] = {k: tag(d[k]) for k in KEYS}
    with open(OUT, 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=False)
        fh.write('\n')
    print(f'wrote {OUT}')


if __name__ == '__main__':
    main()
