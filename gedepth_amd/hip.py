"""ctypes binding of libgedepth_hip.so (C ABI: include/gedepth_hip.h, include/gedepth_eval.h for the KITTI evaluation entry points,
include/gedepth_ddad.h for the DDAD test protocol, include/gedepth_cloud.h for the point clouds and include/gedepth_ground.h for the ground
embedding's maps, include/gedepth_batch.h for the batched KITTI inference and evaluation, include/gedepth_scene.h for the scene clouds).

The header is the only statement of the ABI: ``SIGNATURES`` (name -> (restype, argtypes)) is parsed from it at import, so a new entry
point is declared there and nowhere else.  ``call(name, *args)`` launches an entry point that returns an error code and raises on a
non-zero one; size queries and predicates that return a value are called on ``lib()`` directly.  ``EVAL_SIGNATURES`` is the same table
for include/gedepth_eval.h, ``DDAD_SIGNATURES`` for include/gedepth_ddad.h, ``CLOUD_SIGNATURES`` for include/gedepth_cloud.h and
``GROUND_SIGNATURES`` for include/gedepth_ground.h, whose entry points stay outside the versioned ABI of gedepth_hip.h; ``HEADERS`` names the
five.  ``EXTRA_HEADERS`` is a second table of headers, parsed by the same loop: ``BATCH_SIGNATURES`` for include/gedepth_batch.h (the batched
KITTI front end, merge and metric sums; its ``GeBatchFrame`` struct is mirrored in gedepth_amd/batch_kernels.py).  ``SCENE_HEADERS`` is a
third: ``SCENE_SIGNATURES`` for include/gedepth_scene.h (the scene clouds; its ``GeSceneLayer`` struct is mirrored in
gedepth_amd/scene_kernels.py).  ``STRATA_HEADERS`` is a fourth: ``STRATA_SIGNATURES`` for include/gedepth_strata.h (the stratified
metric sums, wrapped in gedepth_amd/strata_kernels.py).  ``NECK_HEADERS`` is a fifth: ``NECK_SIGNATURES`` for include/gedepth_neck.h (the HAHI
neck's level-token kernels, wrapped in gedepth_amd/neck_kernels.py).  ``ERROR_HEADERS`` is a sixth: ``ERROR_SIGNATURES`` for
include/gedepth_error.h (the error images and the split-level error planes, wrapped in gedepth_amd/error_kernels.py).  ``ACCUM_HEADERS`` is a
seventh: ``ACCUM_SIGNATURES`` for include/gedepth_accum.h (the optimizer's gradient accumulation, wrapped in gedepth_amd/accum_kernels.py).
``DDAD_BATCH_HEADERS`` is an eighth: ``DDAD_BATCH_SIGNATURES`` for include/gedepth_ddad_batch.h (the batched DDAD front end and resized
metric sums, wrapped in gedepth_amd/ddad_batch_kernels.py; they take the ``GeBatchFrame`` of include/gedepth_batch.h).
``SWEEP_HEADERS`` is a ninth: ``SWEEP_SIGNATURES`` for include/gedepth_sweep.h (the prior sweep's front end, wrapped in
gedepth_amd/sweep_kernels.py, which mirrors its ``GePriorVariant`` struct).
``lib()`` binds the entry points of all nine tables.

There is deliberately NO fallback: if the shared library is missing, or a tensor is not a
contiguous CUDA(HIP) tensor of the expected dtype, the call raises.  Build the library with
``gedepth_amd/csrc/build.sh`` (or ``python -c 'import __graft_entry__ as g; g.build()'``).
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GE_LIB') or os.path.join(_HERE, 'csrc', 'libgedepth_hip.so')     # GE_LIB: a differently built library (A/B timing)
HEADERS = {'SIGNATURES': 'gedepth_hip.h', 'EVAL_SIGNATURES': 'gedepth_eval.h', 'DDAD_SIGNATURES': 'gedepth_ddad.h',
           'CLOUD_SIGNATURES': 'gedepth_cloud.h', 'GROUND_SIGNATURES': 'gedepth_ground.h'}      # table name -> its header under include/, in binding order
EXTRA_HEADERS = {'BATCH_SIGNATURES': 'gedepth_batch.h'}      # headers added after the five: same parsing, same binding
SCENE_HEADERS = {'SCENE_SIGNATURES': 'gedepth_scene.h'}      # and after those
STRATA_HEADERS = {'STRATA_SIGNATURES': 'gedepth_strata.h'}   # and after those
NECK_HEADERS = {'NECK_SIGNATURES': 'gedepth_neck.h'}         # and after those
ERROR_HEADERS = {'ERROR_SIGNATURES': 'gedepth_error.h'}      # and after those
ACCUM_HEADERS = {'ACCUM_SIGNATURES': 'gedepth_accum.h'}      # and after those
DDAD_BATCH_HEADERS = {'DDAD_BATCH_SIGNATURES': 'gedepth_ddad_batch.h'}      # and after those
SWEEP_HEADERS = {'SWEEP_SIGNATURES': 'gedepth_sweep.h'}      # and after those
GE_F32, GE_BF16 = 0, 1
GE_COLORIZE_VMIN_DATA, GE_COLORIZE_VMAX_DATA, GE_COLORIZE_EQUAL = 1, 2, 4      # ge_depth_colorize flags

_SCALARS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
            'uint64_t': ctypes.c_ulonglong, 'unsigned long long': ctypes.c_ulonglong}
_DECL = re.compile(r'\b(int|size_t)\s+(ge_\w+)\s*\(([^()]*)\)\s*;')


def parse_header(text):
    """C declarations ``int|size_t ge_*(...);`` -> {name: (restype, argtypes)}.  Every pointer is bound as c_void_p (device pointers are
    passed as integers, host arrays through ctypes.cast).  Strict: a parameter type outside ``_SCALARS`` raises and names the function, and
    so does a ``ge_`` name followed by ``(`` that is not part of a declaration this pattern reads."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    sigs = {}
    for res, name, params in _DECL.findall(text):
        args = []
        for p in ([] if params.strip() == 'void' else params.split(',')):
            if '*' in p:
                args.append(ctypes.c_void_p)
                continue
            ctype = ' '.join(w for w in p.split()[:-1] if w != 'const')          # the last word is the parameter's name
            if ctype not in _SCALARS:
                raise TypeError(f'{name}: parameter "{" ".join(p.split())}" has a type the ctypes binding does not map')
            args.append(_SCALARS[ctype])
        sigs[name] = (_SCALARS[res], args)
    stray = set(re.findall(r'\b(ge_\w+)\s*\(', text)) - set(sigs)
    if stray:
        raise TypeError(f'cannot parse the declaration of {", ".join(sorted(stray))}')
    return sigs


for _table, _header in {**HEADERS, **EXTRA_HEADERS, **SCENE_HEADERS, **STRATA_HEADERS, **NECK_HEADERS, **ERROR_HEADERS, **ACCUM_HEADERS,
                        **DDAD_BATCH_HEADERS, **SWEEP_HEADERS}.items():          # SIGNATURES, EVAL_SIGNATURES, ...: name -> (restype, argtypes)
    with open(os.path.join(os.path.dirname(_HERE), 'include', _header)) as _fh:
        globals()[_table] = parse_header(_fh.read())

_lib = None


class HipLibraryError(RuntimeError):
    pass


def lib():
    """Load (once) and return the shared library; raises HipLibraryError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise HipLibraryError(
                f'{LIB_PATH} is missing: the gfx950 HIP kernels are not built. '
                f'Run gedepth_amd/csrc/build.sh (hipcc --offload-arch=gfx950). There is no CPU/eager fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for table in (*HEADERS, *EXTRA_HEADERS, *SCENE_HEADERS, *STRATA_HEADERS, *NECK_HEADERS, *ERROR_HEADERS, *ACCUM_HEADERS,
                      *DDAD_BATCH_HEADERS, *SWEEP_HEADERS):
            for name, (res, args) in globals()[table].items():
                fn = getattr(handle, name)   # AttributeError here == ABI mismatch: fail loudly
                fn.restype, fn.argtypes = res, args
        _lib = handle
        if os.environ.get('GE_MSDA_MODE'):           # kernel-selection knob of the deformable attention (kernels.msda_mode), e.g.
            handle.ge_msda_mode(int(os.environ['GE_MSDA_MODE']))      # 60 = default without the bf16-tap-weight window forward
    return _lib


def is_built():
    return os.path.isfile(LIB_PATH)


def check(code, what):
    if code != 0:
        raise RuntimeError(f'{what} failed with code {code} '
                           f'({"bad argument" if code == 10001 else "unsupported" if code == 10002 else "hipError_t"})')


def call(name, *args):
    """Run entry point ``name`` (one that returns an error code; the stream is its last argument, as in the header) and raise on failure."""
    code = getattr(_lib or lib(), name)(*args)
    if code:
        check(code, name)


def dtype_code(t):
    if t.dtype == torch.float32:
        return GE_F32
    if t.dtype == torch.bfloat16:
        return GE_BF16
    raise TypeError(f'gedepth_amd kernels take float32 or bfloat16 tensors, got {t.dtype}')


def ptr(t, dtype=None, name='tensor'):
    """Device pointer of a contiguous HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f'{name}: gedepth_amd ops run on MI355X only; got a {t.device} tensor '
                           '(the CPU oracle lives in oracle/ and is test infrastructure)')
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be contiguous')
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream
