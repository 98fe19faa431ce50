"""The route of every 2-D convolution, pinned (``ops/conv.py`` ``conv2d`` / ``conv2d_act``).

No GPU: the entry points are driven with stand-in tensors (meta-device tensors of a Tensor
subclass that says ``is_cuda``) and every sink they can reach — the three k10 autograd
Functions, ``pad``, ``F.conv2d``, ``SNWeight.materialize`` and ``bias_act`` — is replaced by a
recorder that notes its arguments and hands back a stand-in of the result's shape. The ordered
sink events of every case are compared with ``tests/data/conv_routes.json``. The tracing sits
at the sinks, so it does not depend on how the dispatch in between is written:

    python tests/test_conv_routes_cpu.py --record

rewrites the table from whatever ``ops/conv.py`` is in the tree.
"""
import contextlib
import functools
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, 'tests', 'data', 'conv_routes.json')

_CL = torch.channels_last
_DT = {torch.bfloat16: 'bf16', torch.float32: 'f32', torch.float16: 'f16'}
N = 2  # batch of every case

# ---- the full product, through conv2d (cin 192 stands for a 192-channel buffer marked
# mark_zero_tail(., 185) and a 185-channel weight; written '192m')
CIN = [3, 6, 16, 32, 64, 185, '192m']
COUT = [3, 8, 16, 24, 64, 128]
KERNEL = [1, 3, 4, 7]
STRIDE = [1, 2]
PADDING = [0, 1, 3]
MAP = [8, 64]
MODE = ['zeros', 'reflect', 'replicate', 'circular']
SN = [0, 1]
RES = ['none', 'fusible', 'fp32']
FULL_AXES = [('cin', CIN), ('cout', COUT), ('k', KERNEL), ('stride', STRIDE), ('padding', PADDING),
             ('map', MAP), ('mode', MODE), ('sn', SN), ('res', RES)]

# ---- the reduced shape list (cin, cout, k, stride, padding, map): every kind, both sides of
# every threshold the predicates have, crossed with the variants below
SHAPES = [
    # thin inputs (tap-pack and its refusals)
    (3, 64, 7, 1, 3, 64), (3, 64, 3, 1, 1, 64), (3, 64, 4, 2, 1, 64), (6, 64, 3, 1, 1, 64),
    (6, 24, 7, 1, 3, 64), (3, 64, 7, 1, 3, 8), (16, 64, 3, 1, 1, 64), (3, 3, 3, 1, 1, 64),
    (3, 8, 7, 1, 3, 64), (6, 128, 4, 2, 1, 64), (3, 16, 4, 2, 1, 8), (6, 64, 1, 1, 0, 64),
    # thin outputs (tap-split and its refusals)
    (64, 3, 3, 1, 1, 64), (32, 3, 3, 1, 1, 64), (64, 8, 3, 1, 1, 64), (64, 3, 7, 1, 3, 64),
    (185, 3, 3, 1, 1, 64), ('192m', 3, 3, 1, 1, 64), (64, 3, 3, 1, 1, 8), (64, 3, 1, 1, 0, 64),
    (64, 8, 4, 2, 1, 64), (32, 8, 1, 1, 0, 8),
    # k10 / MIOpen
    (64, 64, 3, 1, 1, 64), (64, 64, 3, 1, 1, 8), (64, 128, 3, 2, 1, 64), (64, 128, 4, 2, 1, 64),
    (32, 64, 3, 1, 1, 64), (16, 16, 3, 1, 1, 64), (64, 24, 3, 1, 1, 64), (64, 16, 3, 1, 1, 64),
    (185, 64, 3, 1, 1, 64), ('192m', 64, 4, 2, 1, 64), ('192m', 128, 3, 1, 1, 8),
    (185, 128, 3, 1, 1, 8), (64, 64, 1, 1, 0, 64), (64, 128, 1, 1, 0, 8), (64, 64, 7, 1, 3, 64),
    (64, 64, 7, 1, 3, 8), (64, 64, 3, 1, 0, 64), (64, 64, 3, 1, 3, 64), (16, 24, 3, 1, 1, 64),
    (185, 24, 4, 2, 1, 8), (16, 128, 7, 2, 3, 64), (32, 128, 3, 1, 1, 8), (185, 64, 1, 2, 0, 64),
    (64, 64, 3, 2, 0, 8), (32, 24, 3, 1, 1, 64), (185, 16, 3, 1, 1, 8),
]
# variant -> what differs from the base case (bf16 channels-last input, bf16 weight, groups 1,
# dilation 1, every switch at its default)
VARIANTS = ['act0.2', 'act1.0', 'groups2', 'dilation2', 'fp32', 'fp32_autocast', 'graph_routing',
            'deterministic', 'fused_pad_off', 'residual_epilogue_off', 'eager', 'not_nhwc']


class Fake(torch.Tensor):
    """A meta-device tensor that says it lives on the GPU. (``shape`` / ``dtype`` / ``dim`` are
    answered here and the results of other calls re-wrapped by hand: the general
    ``Tensor.__torch_function__`` costs more than the dispatch under test.)"""
    is_cuda = True

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if getattr(func, '__name__', '') in ('add', '__add__', '__radd__', 'add_', '__iadd__') \
                and _REC is not None:
            _REC.append(['add'] + [_enc(a, 'y') for a in args])
        with torch._C.DisableTorchFunctionSubclass():
            ret = func(*args, **(kwargs or {}))
        return ret.as_subclass(Fake) if type(ret) is torch.Tensor else ret

    def _cached(self, name):
        v = self.__dict__.get('_fake_' + name)
        if v is None:
            with torch._C.DisableTorchFunctionSubclass():
                v = self.__dict__['_fake_' + name] = getattr(torch.Tensor, name).__get__(self)
        return v

    shape = property(lambda self: self._cached('shape'))
    dtype = property(lambda self: self._cached('dtype'))

    def dim(self):
        return len(self.shape)


def fake(shape, dtype=torch.bfloat16, cl=True):
    t = torch.empty(tuple(shape), dtype=dtype, device='meta')
    if cl and t.dim() == 4:
        t = t.contiguous(memory_format=_CL)
    return t.as_subclass(Fake)


_REC = None  # the event list of the running case
_RESIDUAL = None  # its residual (recognised at the sinks by identity)


_SYM = None  # the running case's dimension names, see _symbols


def _symbols(xc, cw, cout, k, stride, padding, hw, groups, dilation):
    """{role: per dimension [(value, name)]}: a recorded shape names each extent after the
    case's own (first match, by the tensor's role: activation 'x', weight 'w', output 'y'), and
    the stride and padding after the case's, so that cases of different sizes on the same route
    share one event list. Given the case, the names decode to the numbers again: nothing is
    lost."""
    ho = (hw + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    cin = [(xc, 'cx'), (cw, 'cw'), (cw // groups, 'cg'), ((cw + 31) // 32 * 32, 'c32'),
           ((cw + 63) // 64 * 64, 'c64')]
    return {'x': ([(N, 'n')], cin, [(hw, 'h'), (hw + 2 * padding, 'hp')]),
            'w': ([(cout, 'co')], cin, [(k, 'k')]),
            'y': ([(N, 'n')], [(cout, 'co')], [(ho, 'ho')]),
            's': [stride, stride], 'p': [padding, padding]}


def _scal(name, v):
    """A stride / padding argument: the case's own by name, anything else as it is."""
    v = _pair(v)
    return name if v == _SYM[name] else v


def _enc(a, role='x'):
    from imaginaire_amd.ops.conv import SNWeight
    if isinstance(a, SNWeight):
        return 'SN' + _enc(a.W, 'w')
    if torch.is_tensor(a):
        sym = _SYM[role] if a.dim() == 4 else (_SYM['w'][0],)
        dims = [dict(reversed(sym[min(i, 2)])).get(v, str(v)) for i, v in enumerate(a.shape)]
        s = '%s[%s]:%s' % ('R' if a is _RESIDUAL else 'T', ','.join(dims),
                           _DT.get(a.dtype, a.dtype))
        vc = getattr(a, '_iamd_valid_channels', None)
        if vc is not None:
            s += ':v' + dict(reversed(_SYM['x'][1])).get(vc, str(vc))
        if a.dim() == 4 and not a.is_contiguous(memory_format=_CL):
            s += ':strided'
        return s
    return a


def _pair(v):
    return [v, v] if isinstance(v, int) else [int(t) for t in v]


def _out(x, w, stride, padding, dilation, dtype=None):
    st, pd, dl = _pair(stride), _pair(padding), _pair(dilation)
    hw = [(x.shape[2 + i] + 2 * pd[i] - dl[i] * (w.shape[2 + i] - 1) - 1) // st[i] + 1
          for i in range(2)]
    if min(hw) <= 0:
        raise RuntimeError('conv: output size %s' % hw)
    return fake((x.shape[0], w.shape[0], hw[0], hw[1]), dtype or x.dtype)


def _k10(x, w, bias, stride, padding, dilation, slope, res=None, sw=None, pmode=0):
    _REC.append(['k10', _enc(x), _enc(w, 'w'), _enc(bias), _scal('s', stride), _scal('p', padding),
                 _pair(dilation), slope, _enc(res, 'y'), _enc(sw), pmode])
    return _out(x, w, stride, padding, dilation, torch.bfloat16)


def _tappack(x, w, bias, stride, padding, dilation, slope, pmode=0):
    _REC.append(['tappack', _enc(x), _enc(w, 'w'), _enc(bias), _scal('s', stride),
                 _scal('p', padding), _pair(dilation), slope, pmode])
    return _out(x, w, stride, padding, dilation, torch.bfloat16)


def _tapsplit(x, w, bias, padding, dilation):
    _REC.append(['tapsplit', _enc(x), _enc(w, 'w'), _enc(bias), _scal('p', padding),
                 _pair(dilation)])
    return _out(x, w, 1, padding, dilation, torch.bfloat16)


def _miopen(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    # (F.conv2d reads an int and a pair alike: recorded as pairs)
    _REC.append(['miopen', _enc(x), _enc(weight, 'w'), _enc(bias), _scal('s', stride),
                 _scal('p', padding), _pair(dilation), groups])
    return _out(x, weight, stride, padding, dilation)


def _pad(x, pad_lrtb, mode):
    _REC.append(['pad', _enc(x), [_scal('p', pad_lrtb[2:]), _scal('p', pad_lrtb[:2])], mode])
    return fake((x.shape[0], x.shape[1], x.shape[2] + pad_lrtb[2] + pad_lrtb[3],
                 x.shape[3] + pad_lrtb[0] + pad_lrtb[1]), x.dtype)


def _materialize(self):
    _REC.append(['materialize', _enc(self)])
    return fake(self.shadow.shape, self.shadow.dtype)


def _bias_act(x, bias=None, slope=1.0):
    _REC.append(['bias_act', _enc(x, 'y'), _enc(bias), slope])
    return x


class _StubExt(object):
    @staticmethod
    def pad_channels_cast(t, c, dtype):
        return fake((t.shape[0], c, t.shape[2], t.shape[3]), dtype)


def _raiser(name):
    def f(*a, **k):
        raise AssertionError('%s was called' % name)
    return f


@contextlib.contextmanager
def harness(sinks=None):
    """Stand-in extension, no stream capture, and the sinks replaced (by the recorders, or by
    ``sinks``: one callable factory name -> replacement); everything is restored on exit."""
    from imaginaire_amd.ops import _ext, bias_act, conv as C
    rec = dict(k10=_k10, tappack=_tappack, tapsplit=_tapsplit, miopen=_miopen, pad=_pad,
               materialize=_materialize, bias_act=_bias_act)
    if sinks is not None:
        rec = {k: sinks(k) for k in rec}
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv('IMAGINAIRE_AMD_EAGER', raising=False)
        mp.setenv('IMAGINAIRE_AMD_MFMA_CONV', '1')
        mp.setattr(_ext, '_EXT', _StubExt)
        mp.setattr(_ext, '_ERR', None)
        mp.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
        mp.setattr(C._MfmaConv2d, 'apply', staticmethod(rec['k10']))
        mp.setattr(C._TapPackConv2d, 'apply', staticmethod(rec['tappack']))
        mp.setattr(C._TapSplitConv2d, 'apply', staticmethod(rec['tapsplit']))
        mp.setattr(C, 'pad', rec['pad'])
        mp.setattr(C.F, 'conv2d', rec['miopen'])
        mp.setattr(C.SNWeight, 'materialize', rec['materialize'])
        mp.setattr(bias_act, 'bias_act', rec['bias_act'])
        # the switches the variants flip, at their defaults (whatever the environment says)
        mp.setattr(C, '_CONV_LOG', None)
        mp.setattr(C, '_FUSED_PAD', True)
        mp.setattr(C, '_RESIDUAL_EPILOGUE', True)
        mp.setattr(C, '_TAPPACK', True)
        mp.setattr(C, '_TAPSPLIT', True)
        mp.setattr(C, '_TAPPACK_MIN_PIX', 2048)
        mp.setattr(C, '_MFMA_MIN_BLOCKS', 16)
        det = torch.are_deterministic_algorithms_enabled()
        routing, C._GRAPH_ROUTING[0] = C._GRAPH_ROUTING[0], 0
        ac = (torch.is_autocast_enabled('cuda'), torch.get_autocast_dtype('cuda'))
        torch.use_deterministic_algorithms(False)
        torch.set_autocast_enabled('cuda', False)
        try:
            yield C, mp
        finally:
            C._GRAPH_ROUTING[0] = routing
            torch.use_deterministic_algorithms(det)
            torch.set_autocast_enabled('cuda', ac[0])
            torch.set_autocast_dtype('cuda', ac[1])


@functools.lru_cache(maxsize=None)
def _x(cin, hw, dtype, cl):
    from imaginaire_amd.ops.conv import mark_zero_tail
    if cin == '192m':
        return mark_zero_tail(fake((N, 192, hw, hw), dtype, cl), 185)
    return fake((N, cin, hw, hw), dtype, cl)


@functools.lru_cache(maxsize=None)
def _w(wshape, sn, dtype):
    from imaginaire_amd.ops.conv import SNWeight
    if not sn:
        return fake(wshape, dtype)
    return SNWeight(fake(wshape, torch.float32), fake(wshape, torch.bfloat16),
                    fake(wshape[:1], torch.float32), fake((wshape[1] * wshape[2] * wshape[3],),
                                                          torch.float32),
                    fake((), torch.float32), None, None)


_cached_fake = functools.lru_cache(maxsize=None)(fake)


def operands(cin, cout, k, stride, padding, hw, sn=0, res='none', groups=1, dilation=1,
             xdtype=torch.bfloat16, wdtype=torch.bfloat16, cl=True):
    """(x, weight, bias, residual) stand-ins of one case (shared between cases: nothing
    writes to them)."""
    x = _x(cin, hw, xdtype, cl)
    weight = _w((cout, (185 if cin == '192m' else cin) // groups, k, k), sn, wdtype)
    r = None
    if res != 'none':
        ho = max(1, (hw + 2 * padding - dilation * (k - 1) - 1) // stride + 1)
        r = _cached_fake((N, cout, ho, ho),
                         torch.bfloat16 if res == 'fusible' else torch.float32)
    return x, weight, _cached_fake((cout,), torch.float32), r


def run_case(C, entry, shape, mode='zeros', sn=0, res='none', groups=1, dilation=1,
             xdtype=torch.bfloat16, wdtype=torch.bfloat16, cl=True, slope=1.0):
    """The sink events of one call, in order."""
    global _REC, _RESIDUAL, _SYM
    cin, cout, k, stride, padding, hw = shape
    _SYM = _symbols(192 if cin == '192m' else cin, 185 if cin == '192m' else cin, cout, k,
                    stride, padding, hw, groups, dilation)
    x, weight, bias, r = operands(cin, cout, k, stride, padding, hw, sn, res, groups, dilation,
                                  xdtype, wdtype, cl)
    _REC, _RESIDUAL = [], r
    try:
        if entry == 'conv2d':
            C.conv2d(x, weight, bias, stride, padding, dilation, groups, mode, residual=r)
        else:
            C.conv2d_act(x, weight, bias, stride, padding, dilation, slope)
    except RuntimeError as e:
        _REC.append(['raise', type(e).__name__])
    events, _REC, _RESIDUAL = _REC, None, None
    return events


def full_cases():
    return itertools.product(*[v for _, v in FULL_AXES])


def variant_cases(variant):
    """The (shape, mode, sn, res) combinations a variant runs."""
    shapes = SHAPES
    if variant == 'groups2':
        shapes = [s for s in SHAPES if s[0] != '192m' and s[0] % 2 == 0 and s[1] % 2 == 0]
    if variant.startswith('act'):  # conv2d_act has neither a padding mode nor a residual
        return [(s, 'zeros', sn, 'none') for s in shapes for sn in SN]
    return list(itertools.product(shapes, MODE, SN, RES))


@contextlib.contextmanager
def variant_scope(C, mp, variant):
    """Keyword arguments of :func:`run_case` for ``variant``, its switches set while inside."""
    kw = dict(entry='conv2d')
    with mp.context() as m:
        if variant.startswith('act'):
            kw.update(entry='conv2d_act', slope=float(variant[3:]))
        elif variant == 'groups2':
            kw.update(groups=2)
        elif variant == 'dilation2':
            kw.update(dilation=2)
        elif variant in ('fp32', 'fp32_autocast'):
            kw.update(xdtype=torch.float32, wdtype=torch.float32)
        elif variant == 'graph_routing':
            C._GRAPH_ROUTING[0] = 1
        elif variant == 'fused_pad_off':
            m.setattr(C, '_FUSED_PAD', False)
        elif variant == 'residual_epilogue_off':
            m.setattr(C, '_RESIDUAL_EPILOGUE', False)
        elif variant == 'eager':
            m.setenv('IMAGINAIRE_AMD_EAGER', '1')
        elif variant == 'not_nhwc':
            kw.update(cl=False)
        if variant == 'fp32_autocast':
            torch.set_autocast_enabled('cuda', True)
            torch.set_autocast_dtype('cuda', torch.bfloat16)
        if variant == 'deterministic':
            torch.use_deterministic_algorithms(True)
        try:
            yield kw
        finally:
            C._GRAPH_ROUTING[0] = 0
            torch.set_autocast_enabled('cuda', False)
            torch.use_deterministic_algorithms(False)


def trace_all():
    """{'full': [events per case of the full product, in order], variant: [...]}."""
    out = {}
    with harness() as (C, mp):
        out['full'] = [run_case(C, 'conv2d', c[:6], c[6], c[7], c[8]) for c in full_cases()]
        for v in VARIANTS:
            with variant_scope(C, mp, v) as kw:
                out[v] = [run_case(C, kw['entry'], s, mode, sn, res,
                                   **{k: a for k, a in kw.items() if k != 'entry'})
                          for s, mode, sn, res in variant_cases(v)]
    return out


def spec():
    """What the table's rows stand for: the axes, in enumeration order."""
    return {'batch': N, 'full_axes': [[n, list(v)] for n, v in FULL_AXES],
            'shapes': [list(s) for s in SHAPES], 'variants': VARIANTS,
            'variant_axes': [['shape', 'SHAPES'], ['mode', MODE], ['sn', SN], ['res', RES]]}


def _block(name):
    """Cases per shape (the inner axes): the table interns such blocks too, since most shapes
    share the pattern of their 24 modes x weights x residuals with many others."""
    return len(SN) if name.startswith('act') else len(MODE) * len(SN) * len(RES)


def write_table(traced):
    """Write {name: [events per case]} interned at three levels: distinct events, distinct
    event lists (of event ids), distinct per-shape blocks (of list ids)."""
    events, lists, blocks, routes = {}, {}, {}, {}
    for name, rows in traced.items():
        ids = [lists.setdefault(
            tuple(events.setdefault(json.dumps(e), len(events)) for e in ev), len(lists))
            for ev in rows]
        n = _block(name)
        routes[name] = [blocks.setdefault(tuple(ids[i:i + n]), len(blocks))
                        for i in range(0, len(ids), n)]
    dump = functools.partial(json.dumps, separators=(',', ':'))
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, 'w') as f:
        f.write('{"spec": %s,\n"events": [\n%s\n],\n"lists": %s,\n"blocks": %s,\n'
                '"routes": {\n%s\n}}\n' % (
                    json.dumps(spec()), ',\n'.join(events), dump([list(k) for k in lists]),
                    dump([list(k) for k in blocks]),
                    ',\n'.join('%s: %s' % (json.dumps(k), dump(v)) for k, v in routes.items())))
    return sum(len(v) for v in traced.values()), len(lists)


def record():
    return write_table(trace_all())


def load_table():
    """{'spec', 'events': the distinct event lists, 'routes': {name: [index into events]}}."""
    with open(TABLE) as f:
        t = json.load(f)
    t['events'] = [[t['events'][i] for i in ids] for ids in t.pop('lists')]
    blocks = t.pop('blocks')
    t['routes'] = {k: [i for b in v for i in blocks[b]] for k, v in t['routes'].items()}
    return t


def _describe(name, i):
    if name == 'full':
        return dict(zip([n for n, _ in FULL_AXES], list(full_cases())[i]))
    return dict(zip(('shape', 'mode', 'sn', 'res'), variant_cases(name)[i]), variant=name)


@pytest.fixture(scope='module')
def traced():
    return trace_all()


def test_routes_match_the_recorded_table(traced):
    table = load_table()
    assert table['spec'] == json.loads(json.dumps(spec())), 'the case axes changed: re-record'
    assert set(table['routes']) == set(traced)
    bad = []
    for name, rows in traced.items():
        want = table['routes'][name]
        assert len(want) == len(rows), name
        for i, (ev, w) in enumerate(zip(rows, want)):
            if json.loads(json.dumps(ev)) != table['events'][w]:
                bad.append((name, i, ev, table['events'][w]))
    msg = '\n'.join('%s\n  got      %s\n  recorded %s' % (_describe(n, i), g, w)
                    for n, i, g, w in bad[:10])
    assert not bad, '%d of %d routes differ from the table:\n%s' % (
        len(bad), sum(len(r) for r in traced.values()), msg)


def _classes(name, events):
    """The route classes one case's recorded events fall into."""
    out = set()
    names = [e[0] for e in events]
    kinds = [n for n in names if n in ('k10', 'tappack', 'tapsplit', 'miopen')]
    for e in events:
        if e[0] == 'k10':
            pm, res, sn = e[10], e[8] is not None, e[9] is not None
            out.add('k10 pad mode %d' % pm)
            if sn:
                out.add('k10 SN-fused')
            if res:
                out.add('k10 fused residual')
            if res and pm:
                out.add('k10 pad mode and fused residual')
        elif e[0] == 'tappack':
            out.add('tappack with pad mode' if e[8] else 'tappack without pad mode')
        elif e[0] == 'tapsplit':
            out.add('tapsplit')
        elif e[0] == 'miopen':
            out.add('miopen plain' if e[1].split(',')[1] == 'cx' else 'miopen padded to 32')
            if name.startswith('act'):
                out.add('conv2d_act fallback')
        elif e[0] == 'add' and any(isinstance(a, str) and a.startswith('R') for a in e[1:]):
            out.add('residual added outside')
    for first in ('pad', 'materialize'):
        if first in names:
            for kd in kinds:
                if names.index(kd) > names.index(first):
                    out.add('%s then %s' % (first, kd))
    return out


CLASSES = ['k10 pad mode 0', 'k10 pad mode 1', 'k10 pad mode 2', 'k10 SN-fused',
           'k10 fused residual', 'k10 pad mode and fused residual', 'tappack without pad mode',
           'tappack with pad mode', 'tapsplit', 'miopen plain', 'miopen padded to 32',
           'pad then k10', 'pad then tappack', 'pad then tapsplit', 'pad then miopen',
           'materialize then k10', 'materialize then tappack', 'materialize then tapsplit',
           'materialize then miopen', 'residual added outside', 'conv2d_act fallback']


def class_counts(table):
    counts = dict.fromkeys(CLASSES, 0)
    for name, rows in table['routes'].items():
        for w in rows:
            for c in _classes(name, table['events'][w]):
                counts[c] += 1
    return counts


def test_table_is_not_hollow():
    counts = class_counts(load_table())
    short = {c: n for c, n in counts.items() if n < 20}
    assert not short, 'route classes with fewer than 20 recorded cases: %s' % short


def test_route_is_pure():
    """The planner launches and allocates nothing: every sink raises, and so does any
    allocation through the extension."""
    class NoExt(object):
        def __getattr__(self, name):
            raise AssertionError('the extension was asked for %s' % name)

    from imaginaire_amd.ops import _ext
    with harness(sinks=_raiser) as (C, mp):
        mp.setattr(_ext, '_EXT', NoExt())
        kinds = set()
        for shape, mode, sn, res in [
                ((3, 64, 7, 1, 3, 64), 'reflect', 1, 'none'),
                ((64, 64, 3, 1, 1, 64), 'reflect', 1, 'fusible'),
                ((64, 64, 3, 1, 1, 64), 'zeros', 0, 'fp32'),
                ((64, 3, 3, 1, 1, 64), 'replicate', 0, 'none'),
                (('192m', 64, 4, 2, 1, 64), 'circular', 1, 'fusible'),
                ((185, 128, 3, 1, 1, 8), 'zeros', 0, 'none'),
                ((64, 64, 7, 1, 3, 8), 'reflect', 1, 'fusible')]:
            x, weight, bias, r = operands(*shape, sn=sn, res=res)
            plan = C._route(x, weight, (shape[3],) * 2, (shape[4],) * 2, (1, 1), 1, mode, r)
            assert isinstance(plan, tuple) and plan == C._route(
                x, weight, (shape[3],) * 2, (shape[4],) * 2, (1, 1), 1, mode, r)
            kinds.add(plan.kind)
        assert kinds == {'tappack', 'tapsplit', 'k10', 'miopen'}


if __name__ == '__main__':
    if '--record' in sys.argv[1:]:
        print('recorded %d cases, %d distinct event lists -> %s' % (record() + (TABLE,)))
    else:
        sys.exit(pytest.main([__file__] + sys.argv[1:]))
