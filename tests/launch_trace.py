"""TEST-ONLY recorder of the C-ABI calls an evaluation makes, and the fixed tiny evaluations whose call sequences are pinned.

``trace()`` swaps the object ``sda_amd._lib.load()`` returns for a proxy that notes, before passing every call on, the symbol and
its arguments as ``_lib.SIGNATURES`` types them: integers and floats verbatim, every device / host address as false (null) or true (the
allocator may hand out other addresses on another day), a ``POINTER(struct)`` argument field by field in the same way.  The stream
(the trailing ``c_void_p`` of every launching symbol) is not noted.

``host_trace()`` does the same one level up for the host replay (tests/cpu_shim.py): the calls that reach the patched
``ops.conv_igemm``, ``ops.ln_stats``, ``ops.ln_bwd``, ``ops.conv_wgrad`` and ``ops.plane_sum``, tensors as (shape, strides, offset).

The fixtures (tests/golden/engine_trace_gpu.json, engine_trace_host.json) hold every distinct call once and each case as a list of
indices.  ``python -m tests.launch_trace --record gpu|host`` writes them (the device one needs an MI355X)."""
import contextlib
import ctypes
import json
import os
import sys

import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GPU_FIXTURE = os.path.join(GOLDEN, 'engine_trace_gpu.json')
HOST_FIXTURE = os.path.join(GOLDEN, 'engine_trace_host.json')


# ------------------------------------------------------------------------------------------ describing a call

def _is_pointer(tp) -> bool:
    return tp is ctypes.c_void_p or tp is ctypes.c_char_p or (isinstance(tp, type) and issubclass(tp, ctypes._Pointer))


def _field(tp, value):
    if isinstance(tp, type) and issubclass(tp, ctypes.Structure):
        return describe_struct(value)
    if isinstance(tp, type) and issubclass(tp, ctypes.Array):
        return [_field(tp._type_, v) for v in value]
    if _is_pointer(tp):
        return bool(value)
    return value


def describe_struct(s) -> list:
    """[struct name, field values in declaration order] (the names are in sda_amd._lib: the fixture stays small)."""
    return [type(s).__name__] + [_field(tp, getattr(s, name)) for name, tp in s._fields_]


def _argument(tp, arg):
    if isinstance(tp, type) and issubclass(tp, ctypes._Pointer):
        if arg is None:
            return False
        obj = getattr(arg, '_obj', None)                 # (ctypes.byref(desc))
        if obj is None and hasattr(arg, 'contents'):
            obj = arg.contents if arg else None
        if isinstance(obj, ctypes.Structure):
            return describe_struct(obj)
        return obj is not None
    if _is_pointer(tp):
        return bool(arg)
    return getattr(arg, 'value', arg)


def describe_call(name: str, argtypes, args) -> list:
    if argtypes and argtypes[-1] is ctypes.c_void_p and len(args) == len(argtypes):
        argtypes, args = argtypes[:-1], args[:-1]        # the stream
    return [name] + [_argument(tp, a) for tp, a in zip(argtypes, args)]


class TracedLib:
    def __init__(self, lib, log: list):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        from sda_amd._lib import SIGNATURES
        fn = getattr(self._lib, name)
        sig = SIGNATURES.get(name)
        if sig is None:
            return fn

        def call(*args):
            self._log.append(describe_call(name, sig[1], args))
            return fn(*args)
        return call


@contextlib.contextmanager
def trace():
    """-> the list every C-ABI call made inside the block is appended to."""
    from sda_amd import _lib
    real, log = _lib.load(), []
    _lib._lib = TracedLib(real, log)
    try:
        yield log
    finally:
        _lib._lib = real


def _host_value(v):
    if isinstance(v, ctypes.Structure):
        return describe_struct(v)
    if torch.is_tensor(v):
        return ['tensor', list(v.shape), list(v.stride()), v.storage_offset()]
    if isinstance(v, (tuple, list)):
        return [_host_value(e) for e in v]
    return v


HOST_OPS = ('conv_igemm', 'ln_stats', 'ln_bwd', 'conv_wgrad', 'plane_sum')


@contextlib.contextmanager
def host_trace(mp):
    """After cpu_shim.install(mp): -> the list the calls reaching the patched HOST_OPS are appended to."""
    from sda_amd import ops
    log = []

    def wrap(name, fn):
        def call(*args, **kwargs):
            log.append([name] + [_host_value(a) for a in args] + [[k, _host_value(v)] for k, v in sorted(kwargs.items())])
            return fn(*args, **kwargs)
        return call
    with mp.context() as m:
        for name in HOST_OPS:
            m.setattr(ops, name, wrap(name, getattr(ops, name)))
        yield log


# ------------------------------------------------------------------------------------------ the fixture form

def encode(traces: dict) -> dict:
    """{case: [call, ...]} -> {'calls': [distinct call, ...], 'cases': {case: [index, ...]}}."""
    calls, index, cases = [], {}, {}
    for case, log in traces.items():
        seq = []
        for call in log:
            key = json.dumps(call, sort_keys=True)
            if key not in index:
                index[key] = len(calls)
                calls.append(json.loads(key))
            seq.append(index[key])
        cases[case] = seq
    return dict(calls=calls, cases=cases)


def decode(fixture: dict, case: str) -> list:
    return [fixture['calls'][i] for i in fixture['cases'][case]]


def normal(log: list) -> list:
    """A recorded log as it reads after a round trip through JSON (tuples -> lists, keys sorted)."""
    return json.loads(json.dumps(log, sort_keys=True))


def _differing(a, b, where: str) -> list:
    """The differing leaves of two described values, struct fields by name."""
    from sda_amd import _lib
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        struct = getattr(_lib, a[0], None) if a and isinstance(a[0], str) and a[0] == b[0] else None
        names = [None] + [n for n, _ in struct._fields_] if struct is not None and len(a) == len(struct._fields_) + 1 else None
        out = []
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                out += _differing(x, y, f'{where}.{names[i]}' if names else f'{where}[{i}]')
        return out
    return [f'{where}: got {a!r}, recorded {b!r}']


def first_difference(got: list, want: list) -> str:
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f'call {i} ({a[0]} / recorded {b[0]}): ' + '; '.join(_differing(a, b, 'call'))
    if len(got) != len(want):
        return f'{len(got)} calls, recorded {len(want)}: {[c[0] for c in got]} vs {[c[0] for c in want]}'
    return ''


# ------------------------------------------------------------------------------------------ the pinned evaluations

_nets = {}


def _net(kind: str, padding: str, device):
    """The tiny nets: '2d' two-level (64, 128), '2d48' (48, 128) -- no Winograd and no f16 x 2 packing at level 0 --, '1d' two-level
    (32, 32) on the block1d route.  One block per level, 3-tap kernels, stride 2."""
    from sda_amd.score import ScoreUNet
    key = (kind, padding, str(device))
    if key not in _nets:
        torch.manual_seed(0)
        if kind == '1d':
            net = ScoreUNet(3, 0, embedding=16, hidden_channels=(32, 32), hidden_blocks=(1, 1), kernel_size=3, activation=nn.SiLU,
                            spatial=1, padding_mode=padding)
        else:
            net = ScoreUNet(2, 1, embedding=16, hidden_channels=(48 if kind == '2d48' else 64, 128), hidden_blocks=(1, 1),
                            kernel_size=3, activation=nn.SiLU, spatial=2, padding_mode=padding)
        _nets[key] = net.to(device)
    return _nets[key]


def _inputs(kind: str, per_image: bool, device):
    """Batch 2; shared time goes with a broadcast context channel, per-image time with one context block per image."""
    g = torch.Generator().manual_seed(1)
    if kind == '1d':
        x, c = torch.randn(2, 3, 64, generator=g), None
    else:
        x = torch.randn(2, 2, 32, 32, generator=g)
        c = torch.randn(*((2, 1, 32, 32) if per_image else (1, 32, 32)), generator=g)
    t = torch.tensor([0.3, 0.7]) if per_image else torch.tensor(0.3)
    cot = torch.randn(x.shape, generator=g)
    return [None if v is None else v.to(device) for v in (x, t, c, cot)]


def evaluate(kind: str, padding: str, per_image: bool, mode: str, device):
    """mode: 'fwd' (no_grad), 'vjp' (forward + input VJP), 'train:<route>' (training.parameter_gradients(wgrad=route), input and
    parameter gradients in one backward)."""
    from sda_amd import training
    net = _net(kind, padding, device)
    x, t, c, cot = _inputs(kind, per_image, device)
    net.zero_grad(set_to_none=True)
    if mode == 'fwd':
        with torch.no_grad():
            net(x, t, c)
        return
    xs = x.clone().requires_grad_(True)
    if mode == 'vjp':
        net(xs, t, c).backward(cot)
        return
    with training.parameter_gradients(wgrad=mode.split(':')[1]):
        net(xs, t, c).backward(cot)


# (case name, net, padding, per-image time, mode, multiply, (module name, attribute) switched off or None)
def gpu_cases() -> list:
    out = []
    for padding in ('circular', 'zeros'):
        for per_image in (False, True):
            tag = f'{padding}-{"per_image" if per_image else "shared"}'
            for mode in ('fwd', 'vjp', 'train:general', 'train:tiled_ht'):
                out.append((f'2d-{tag}-{mode}-f32', '2d', padding, per_image, mode, 'f32', None))
            for mode in ('fwd', 'vjp'):                  # (parameter gradients are formed with the fp32 multiply only)
                out.append((f'2d-{tag}-{mode}-f16x2', '2d', padding, per_image, mode, 'f16x2', None))
        for multiply, switches in (('f32', (('ops', 'PARITY4'), ('engine', 'PARITY_SPLIT'), ('ops', 'POOLED'))),
                                   ('f16x2', (('ops', 'H2_S2'), ('ops', 'H2_UP'), ('ops', 'H2_POOL')))):
            for sw in switches:
                out.append((f'2d-{padding}-shared-vjp-{multiply}-no_{sw[1]}', '2d', padding, False, 'vjp', multiply, sw))
        out.append((f'2d48-{padding}-shared-vjp-f32', '2d48', padding, False, 'vjp', 'f32', None))
        out.append((f'2d48-{padding}-shared-vjp-f16x2', '2d48', padding, False, 'vjp', 'f16x2', None))
        if padding == 'circular':
            out.append(('2d48-circular-per_image-train:tiled_ht-f32', '2d48', padding, True, 'train:tiled_ht', 'f32', None))
        for mode in ('fwd', 'vjp', 'train:general'):
            out.append((f'1d-{padding}-shared-{mode}-f32', '1d', padding, False, mode, 'f32', None))
    return out


def host_cases() -> list:
    out = [('2d-circular-shared-fwd-f32', '2d', 'circular', False, 'fwd', 'f32', None)]
    for padding in ('circular', 'zeros'):
        for split in (True, False):
            sw = None if split else ('engine', 'PARITY_SPLIT')
            tail = '' if split else '-no_PARITY_SPLIT'
            for kind, per_image in (('2d', False), ('2d', True), ('1d', False)):
                if per_image and not split:
                    continue                             # (the time rows do not meet the heads' VJP)
                tag = f'{kind}-{padding}-{"per_image" if per_image else "shared"}'
                for mode in ('vjp', 'train:general'):
                    out.append((f'{tag}-{mode}-f32{tail}', kind, padding, per_image, mode, 'f32', sw))
    return out


def run_case(case, device, mp, tracer, warm_up: bool = True) -> list:
    """Warm up (packings, report slots: not on the host replay, whose log holds no packing call), then trace the same evaluation.
    mp: a pytest MonkeyPatch; tracer: ``trace`` or ``lambda: host_trace(mp)``."""
    from sda_amd import engine, ops
    _name, kind, padding, per_image, mode, multiply, switch = case
    prev = ops.set_multiply(multiply)
    try:
        with mp.context() as m:
            if switch is not None:
                m.setattr(dict(ops=ops, engine=engine)[switch[0]], switch[1], False)
            if warm_up:
                evaluate(kind, padding, per_image, mode, device)
            with tracer() as log:
                evaluate(kind, padding, per_image, mode, device)
        return normal(log)
    finally:
        ops.set_multiply(prev)


PROFILE_CASES = ('2d-circular-shared-vjp-f32', '2d-circular-shared-train:general-f32')


def run_profile(case, device, mp) -> dict:
    """The same evaluation under ops.ConvProfile(): everything it records but the times."""
    from sda_amd import ops
    _name, kind, padding, per_image, mode, multiply, _switch = case
    prev = ops.set_multiply(multiply)
    try:
        evaluate(kind, padding, per_image, mode, device)
        prof = ops.ConvProfile()
        with mp.context() as m:
            m.setattr(ops, 'conv_profile', prof)
            evaluate(kind, padding, per_image, mode, device)
        s, ms = prof.summary(), prof.mem_summary()
        return normal(dict(launches=s['launches'], total_flops=s['total_flops'],
                           families={k: dict(launches=v['launches'], flops=v['flops']) for k, v in s['families'].items()},
                           family_bytes=prof.family_bytes,
                           mem={k: dict(launches=v['launches'], bytes=v['bytes']) for k, v in ms.items()}))
    finally:
        ops.set_multiply(prev)


def record(which: str):
    import pytest
    mp = pytest.MonkeyPatch()
    try:
        if which == 'gpu':
            dev = torch.device('cuda')
            fixture = encode({c[0]: run_case(c, dev, mp, trace) for c in gpu_cases()})
            by_name = {c[0]: c for c in gpu_cases()}
            fixture['profile'] = {name: run_profile(by_name[name], dev, mp) for name in PROFILE_CASES}
            path = GPU_FIXTURE
        else:
            from tests import cpu_shim
            cpu_shim.install(mp)
            fixture = encode({c[0]: run_case(c, torch.device('cpu'), mp, lambda: host_trace(mp), warm_up=False) for c in host_cases()})
            path = HOST_FIXTURE
    finally:
        mp.undo()
    with open(path, 'w') as f:
        json.dump(fixture, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print(f'{path}: {len(fixture["cases"])} cases, {len(fixture["calls"])} distinct calls, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    if len(sys.argv) != 3 or sys.argv[1] != '--record' or sys.argv[2] not in ('gpu', 'host'):
        sys.exit('usage: python -m tests.launch_trace --record gpu|host')
    record(sys.argv[2])
