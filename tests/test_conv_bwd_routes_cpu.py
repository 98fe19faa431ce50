"""Every backward of ``ops/conv.py``, pinned at the extension boundary.

No GPU: the real ``forward`` and ``backward`` static methods of the four conv Functions (and
``conv_transpose2d`` as it is) run on the stand-in tensors of ``test_conv_routes_cpu`` against a
stub extension that records every call (name, shapes, dtypes, scalars) and hands back a stand-in
of the result's shape. ``torch.ops.aten.convolution_backward``, ``F.conv_transpose2d``,
``_dgrad_weight``, ``_take_grad_dest``, the side stream (``wait_stream``, enter / exit,
``record_stream``), the tuner's pending tables and the ``_Logged`` rows are recorded too; calls
made on the side stream carry ``@side``. The ordered events of every case are compared with
``tests/data/conv_bwd_routes.json``. The tracing sits below the dispatch, so it does not depend
on how the backward is written:

    python tests/test_conv_bwd_routes_cpu.py --record

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
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from test_conv_routes_cpu import Fake, fake, harness  # noqa: E402,F401

TABLE = os.path.join(ROOT, 'tests', 'data', 'conv_bwd_routes.json')
_CL = torch.channels_last
_DT = {torch.bfloat16: 'bf16', torch.float32: 'f32', torch.float16: 'f16', torch.bool: 'bool'}
N = 2
BF, F32 = torch.bfloat16, torch.float32

# ---- k10 shapes (cin, cout, k, stride, padding, dilation, map): a case on each side of every
# threshold of the backward (batch 2; the comments name what each pair separates)
K10 = [
    (64, 64, 3, 1, 1, 1, 8), (64, 64, 3, 1, 1, 1, 64),        # dblocks 1 / 64; SN dot ratio
    (64, 64, 3, 1, 3, 1, 64),                                  # negative transposed padding
    (64, 64, 3, 1, 2, 2, 64),                                  # dilated: flip
    (64, 128, 4, 2, 1, 1, 128), (64, 128, 4, 2, 1, 1, 256),    # _STRIDED_DGRAD_MIN_PIX
    (64, 128, 4, 2, 1, 1, 32), (64, 128, 4, 2, 1, 1, 64),      # 16 s^2 blocks (min_pix0)
    (64, 3, 3, 1, 1, 1, 64), (64, 16, 3, 1, 1, 1, 64),         # thin output
    (64, 16, 7, 1, 3, 1, 64), (64, 16, 1, 1, 0, 1, 64),        # 784 > 512; one tap
    (32, 64, 3, 1, 1, 1, 64), (30, 24, 3, 1, 1, 1, 64),        # stored / cropped channels
    (64, 64, 3, 3, 1, 1, 64), (64, 64, 1, 1, 0, 1, 256),       # stride 3; 1x1
    (64, 64, 3, 1, 1, 1, 32), (64, 64, 3, 1, 1, 1, 48),        # exactly 16 blocks; SN ratio 8
]
K10_FEW = [K10[i] for i in (0, 1, 3, 4, 5, 8, 13)]
K10_FULL = [K10[i] for i in (1, 4, 8)]
K10_WG = [K10[i] for i in (0, 1, 4)]  # (the weight-gradient switches run on these)
K10_S1 = [K10[i] for i in (0, 1, 2, 9, 12, 13, 15)]  # stride 1, dilation 1: the flipped weight
NEEDS = [n for n in itertools.product((True, False), repeat=3) if any(n)]
NEEDS_W = [n for n in NEEDS if n[1]]
NEEDS_MAIN = [(True, True, True), (True, False, False), (False, True, True)]
WKIND = [(0, 'bf16'), (0, 'param'), (1, 'param')]  # (sn, weight: bf16 tensor / fp32 Parameter)
TAPPACK = [
    (3, 64, 7, 1, 3, 1, 64), (3, 64, 3, 1, 1, 1, 64), (6, 64, 3, 1, 1, 1, 64),
    (16, 64, 3, 1, 1, 1, 64), (3, 64, 4, 2, 1, 1, 64), (6, 128, 4, 2, 1, 1, 64),
    (16, 24, 3, 2, 1, 1, 64), (3, 64, 3, 1, 2, 2, 64), (3, 64, 3, 2, 1, 2, 64),
    (3, 64, 3, 2, 3, 1, 64), (3, 16, 3, 1, 1, 1, 64),
]
TAPPACK_FEW = [TAPPACK[i] for i in (0, 4)]  # (the full product runs on these)
TAPSPLIT = [(64, 3, 3, 1, 1, 1, 64), (32, 3, 3, 1, 1, 1, 64), (64, 8, 3, 1, 1, 1, 64),
            (64, 3, 3, 1, 2, 2, 64), (30, 3, 7, 1, 3, 1, 64)]
PERSAMPLE = [(64, 64, 3, 1, 1, 1, 32), (32, 24, 3, 1, 1, 1, 32), (64, 64, 1, 1, 0, 1, 32),
             (16, 64, 3, 1, 2, 2, 32)]
DECONV = [(64, 64, 4, 2, 1, 32), (64, 32, 4, 2, 1, 32), (64, 20, 4, 2, 1, 32),
          (8, 8, 4, 2, 1, 32), (64, 64, 3, 2, 1, 32), (64, 64, 4, 4, 0, 32),
          (64, 64, 4, 2, 1, 8), (128, 64, 4, 2, 1, 64)]

_REC = None
_SIDE = [False]
_TAGS = {}


def _enc(a):
    if torch.is_tensor(a):
        s = '%s[%s]:%s' % (_TAGS.get(id(a), 'T'), ','.join(str(v) for v in a.shape),
                           _DT.get(a.dtype, a.dtype))
        if a.dim() == 4 and not a.is_contiguous(memory_format=_CL):
            s += ':strided'
        return s
    if isinstance(a, (list, tuple)):
        return [_enc(v) for v in a]
    if isinstance(a, torch.dtype):
        return _DT.get(a, str(a))
    if isinstance(a, _Stream):
        return a.name
    return a


def _ev(name, *args):
    _REC.append([name + ('@side' if _SIDE[0] else '')] + [_enc(a) for a in args])


def _tag(t, tag):
    _TAGS[id(t)] = tag
    _KEEP.append(t)
    return t


_KEEP = []  # (tagged tensors stay alive through their case: ids are not reused)


def _hw(h, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


class _Stream(object):
    def __init__(self, name):
        self.name = name

    def wait_stream(self, other):
        _ev('wait_stream', self, other)


_MAIN, _SIDE_STREAM = _Stream('main'), _Stream('side')


@contextlib.contextmanager
def _on_stream(st):
    _ev('enter', st)
    was, _SIDE[0] = _SIDE[0], st is _SIDE_STREAM
    try:
        yield
    finally:
        _SIDE[0] = was
        _ev('exit', st)


def _record_stream(t, st):
    _ev('record_stream', t, st)


class _LoggedRec(object):
    def __init__(self, kind, path, flops, desc):
        self.row = (kind, path, flops, desc)

    def __enter__(self):
        _ev('log', *self.row)
        return self

    def __exit__(self, *exc):
        _ev('endlog')
        return False


class Ext(object):
    """The stub extension: every function the conv backwards can reach."""
    v2 = False

    def __getattr__(self, name):
        raise AssertionError('the stub extension has no %s' % name)

    def pad_channels_cast(self, t, c, dtype):
        _ev('pad_channels_cast', t, c, dtype)
        return fake((t.shape[0], c, t.shape[2], t.shape[3]), dtype)

    def conv2d_mfma(self, x, w, bias, sh, sw, ph, pw, dh, dw, slope, nb, ncv=-1, res=None,
                    sig=None, pmode=0):
        _ev('conv2d_mfma', x, w, bias, sh, sw, ph, pw, dh, dw, slope, nb, ncv, res, sig, pmode)
        return fake((x.shape[0], ncv if ncv > 0 else w.shape[0] // nb,
                     _hw(x.shape[2], w.shape[2], sh, ph, dh),
                     _hw(x.shape[3], w.shape[3], sw, pw, dw)), BF)

    def conv2d_dgrad_mfma(self, dy, wb, ph, pw, ncv, sig):
        _ev('conv2d_dgrad_mfma', dy, wb, ph, pw, ncv, sig)
        return fake((dy.shape[0], ncv if ncv > 0 else wb.shape[1],
                     dy.shape[2] + wb.shape[2] - 1 - 2 * ph,
                     dy.shape[3] + wb.shape[3] - 1 - 2 * pw), BF)

    def conv2d_dgrad_strided(self, dy, wb, s, ph, pw, H, W, ncv, ascale):
        _ev('conv2d_dgrad_strided', dy, wb, s, ph, pw, H, W, ncv, ascale)
        return fake((dy.shape[0], ncv if ncv > 0 else wb.shape[1], H, W), BF)

    def conv_weight_flip_t(self, w, s=1, kh0=0, kw0=0, nb=1):
        _ev('conv_weight_flip_t', w, s, kh0, kw0, nb)
        return fake((w.shape[1] * nb, w.shape[0] // nb, -(-(w.shape[2] - kh0) // s),
                     -(-(w.shape[3] - kw0) // s)), BF)

    def conv_phase_scatter(self, out, dx, *a):
        _ev('conv_phase_scatter', out, dx, *a)

    def bias_act_bwd(self, y, dy, slope):
        _ev('bias_act_bwd', y, dy, slope)
        return fake(dy.shape, BF), fake((dy.shape[1],), F32)

    def im2col_pack(self, x, kh, kw, sh, sw, ph, pw, dh, dw, kp, pmode=0):
        _ev('im2col_pack', x, kh, kw, sh, sw, ph, pw, dh, dw, kp, pmode)
        return fake((x.shape[0], kp, _hw(x.shape[2], kh, sh, ph, dh),
                     _hw(x.shape[3], kw, sw, pw, dw)), BF)

    def conv2d_wgrad_mfma(self, dy, xb, kh, kw, sh, sw, ph, pw, dh, dw, cout, cin, bf16_out, nb,
                          variant=0, sn=None, dest=None, pmode=0):
        _ev('conv2d_wgrad_mfma', dy, xb, kh, kw, sh, sw, ph, pw, dh, dw, cout, cin, bf16_out,
            nb, variant, sn, dest, pmode)
        return fake((cout if cout > 0 else nb * dy.shape[1], cin if cin > 0 else xb.shape[1],
                     kh, kw), BF if bf16_out else F32)

    def conv2d_wgrad_v2_eligible(self, dy, xb, *a):
        _ev('conv2d_wgrad_v2_eligible', dy, xb, *a)
        return self.v2

    def sn_dot_partials(self, dx, xb, sig):
        _ev('sn_dot_partials', dx, xb, sig)
        return _tag(fake((64,), F32), 'DOT')

    def pad_nhwc_bwd(self, dy, h, w, l, r, t, b, mode):
        _ev('pad_nhwc_bwd', dy, h, w, l, r, t, b, mode)
        return fake((dy.shape[0], dy.shape[1], h, w), dy.dtype)

    def pad_nhwc_fwd(self, x, l, r, t, b, mode):
        _ev('pad_nhwc_fwd', x, l, r, t, b, mode)
        return fake((x.shape[0], x.shape[1], x.shape[2] + t + b, x.shape[3] + l + r), x.dtype)

    def conv_tap_sum(self, z, bias, cout, kh, kw, ph, pw, dh, dw):
        _ev('conv_tap_sum', z, bias, cout, kh, kw, ph, pw, dh, dw)
        return fake((z.shape[0], cout, _hw(z.shape[2], kh, 1, ph, dh),
                     _hw(z.shape[3], kw, 1, pw, dw)), BF)

    def conv_tap_gather(self, dy, cz, kh, kw, ph, pw, dh, dw, H, W):
        _ev('conv_tap_gather', dy, cz, kh, kw, ph, pw, dh, dw, H, W)
        return fake((dy.shape[0], cz, H, W), BF)


def _conv_backward(dy, x, w, bias_sizes, stride, padding, dilation, transposed, out_pad, groups,
                   mask):
    _ev('aten.convolution_backward', dy, x, w, bias_sizes, stride, padding, dilation, transposed,
        out_pad, groups, mask)
    return (fake(x.shape, x.dtype) if mask[0] else None,
            fake(w.shape, w.dtype) if mask[1] else None, None)


def _conv_transpose2d(x, w, bias=None, stride=1, padding=0, output_padding=0, groups=1,
                      dilation=1):
    _ev('F.conv_transpose2d', x, w, bias, stride, padding, output_padding, groups, dilation)
    p2 = (lambda v: (v, v) if isinstance(v, int) else tuple(v))
    st, pd = p2(stride), p2(padding)
    return fake((x.shape[0], w.shape[1], (x.shape[2] - 1) * st[0] - 2 * pd[0] + w.shape[2],
                 (x.shape[3] - 1) * st[1] - 2 * pd[1] + w.shape[3]), x.dtype)


def _key_fields(key):
    """A weight-gradient tuning key as the flat list the tuple form holds (a key with named
    fields: the nine shape fields, then its sn and pad-mode marks where set)."""
    if hasattr(key, '_fields'):
        d = key._asdict()
        key = tuple(key[:9]) + ((d['sn'],) if d['sn'] else ()) + \
            (('pm%d' % d['pmode'],) if d['pmode'] else ())
    return [_enc(k) for k in key]


class _Choices(dict):
    """A tuner table seeded with one choice for every key (or none), recording what is filed."""
    def __init__(self, name, choice=None):
        dict.__init__(self)
        self.name, self.choice = name, choice

    def get(self, key, default=None):
        return self.choice if self.choice is not None else default

    def __contains__(self, key):
        return self.choice is not None or dict.__contains__(self, key)

    def setdefault(self, key, value):
        _ev(self.name, _key_fields(key), value)
        return dict.setdefault(self, key, value)

    def __setitem__(self, key, value):
        _ev(self.name, _key_fields(key))
        dict.__setitem__(self, key, value)


_CASE = {'wflip': False, 'dest': True}  # what the two lookups below answer in the running case


def _dgrad_weight(wb):
    _ev('_dgrad_weight', wb)
    if not _CASE['wflip']:
        return None
    return _tag(fake((wb.shape[1], wb.shape[0]) + tuple(wb.shape[2:]), BF), 'F')


def _take_grad_dest(p, shape):
    _ev('_take_grad_dest', p is not None, shape)
    return _tag(fake(shape, F32), 'D') if (p is not None and _CASE['dest']) else None


class Ctx(object):
    def __init__(self, needs):
        self.needs_input_grad = tuple(needs)
        self.saved_tensors = ()

    def save_for_backward(self, *ts):
        self.saved_tensors = ts


DEFAULTS = dict(_OVERLAP_BWD='0', _OVERLAP_SMALL_PIX=8192, _SN_DOT_RATIO=8.0, _MFMA_WGRAD='1',
                _STRIDED_DGRAD=True, _STRIDED_DGRAD_MIN_PIX=131072, _STRIDED_ONE_LAUNCH=True,
                _MFMA_MIN_DGRAD_BLOCKS=16, _TAPPACK=True, _DECONV_FORCE=None,
                _DECONV_MIN_PIX=4096, _PS_DEBUG=0, _PS_CHECK=False, _CONV_LOG=None)


@contextlib.contextmanager
def bwd_harness(ext=None):
    """The routes harness with the stub extension and every recorder below the backwards."""
    with harness() as (C, mp), torch.no_grad():  # (as inside autograd.Function.apply)
        from imaginaire_amd.ops import _ext
        X = ext if ext is not None else Ext()
        mp.setattr(_ext, '_EXT', X)
        for k, v in DEFAULTS.items():
            mp.setattr(C, k, v)
        mp.setattr(C, '_BWD_SIDE', {})
        mp.setattr(C, '_TEST_FLIP_WGRAD', [0, 0])
        mp.setattr(C, '_Logged', _LoggedRec)
        mp.setattr(C, '_dgrad_weight', _dgrad_weight)
        mp.setattr(C, '_take_grad_dest', _take_grad_dest)
        mp.setattr(C, '_WGRAD_CHOICE', _Choices('choice'))
        mp.setattr(C, '_WGRAD_PENDING', _Choices('wgrad_pending'))
        mp.setattr(C, '_DECONV_CHOICE', _Choices('deconv_choice'))
        mp.setattr(C, '_DECONV_PENDING', _Choices('deconv_pending'))
        mp.setattr(torch.ops.aten, 'convolution_backward', _conv_backward)
        mp.setattr(C.F, 'conv_transpose2d', _conv_transpose2d)
        mp.setattr(torch.cuda, 'current_device', lambda: 0)
        mp.setattr(torch.cuda, 'Stream', lambda device=None: _SIDE_STREAM)
        mp.setattr(torch.cuda, 'current_stream', lambda device=None: _MAIN)
        mp.setattr(torch.cuda, 'stream', _on_stream)
        mp.setattr(torch.Tensor, 'record_stream', _record_stream, raising=False)
        yield C, mp, X


_cfake = functools.lru_cache(maxsize=None)(fake)


def _begin():
    global _REC
    _REC = []
    _TAGS.clear()
    del _KEEP[:]
    _SIDE[0] = False


def _end(C, outs):
    global _REC
    _ev('return', *outs)
    if C._TEST_FLIP_WGRAD[0]:
        _ev('flip_counter', C._TEST_FLIP_WGRAD[1])
    ev, _REC = _REC, None
    return ev


def run_k10(C, shape, pmode=0, sn=0, wkind='bf16', slope=1.0, needs=(True, True, True),
            xdtype=BF, res=None, wflip=False, dest=True):
    """The events of one ``_MfmaConv2d`` forward + backward."""
    cin, cout, k, s, p, d, hw = shape
    _begin()
    x = _cfake((N, cin, hw, hw), xdtype)
    if wkind == 'param':
        W = torch.nn.Parameter(fake((cout, cin, k, k), F32))
    else:
        W = _cfake((cout, cin, k, k), BF)
    sw = None
    if sn:
        sw = C.SNWeight(W, _cfake((cout, cin, k, k), BF), _cfake((cout,), F32),
                        _cfake((cin * k * k,), F32), _tag(fake((), F32), 'SIG'), None, None)
    ho = _hw(hw, k, s, p, d)
    r = None if res is None else _tag(fake((N, cout, ho, ho), res), 'R')
    _CASE.update(wflip=wflip, dest=dest)
    ctx = Ctx(tuple(needs) + (False,) * 4 + (r is not None, False, False))
    C._MfmaConv2d.forward(ctx, x, W, _cfake((cout,), F32), (s, s), (p, p), (d, d), slope, r, sw,
                          pmode)
    _ev('backward')
    return _end(C, C._MfmaConv2d.backward(ctx, _tag(fake((N, cout, ho, ho), BF), 'DY')))


def run_tappack(C, shape, pmode=0, slope=1.0, needs=(True, True, True), xdtype=BF, wdtype=BF):
    cin, cout, k, s, p, d, hw = shape
    _begin()
    ctx = Ctx(tuple(needs) + (False,) * 5)
    C._TapPackConv2d.forward(ctx, _cfake((N, cin, hw, hw), xdtype), _cfake((cout, cin, k, k), wdtype),
                             _cfake((cout,), F32), (s, s), (p, p), (d, d), slope, pmode)
    _ev('backward')
    ho = _hw(hw, k, s, p, d)
    return _end(C, C._TapPackConv2d.backward(ctx, _tag(fake((N, cout, ho, ho), BF), 'DY')))


def run_tapsplit(C, shape, needs=(True, True, True), dydtype=BF):
    cin, cout, k, s, p, d, hw = shape
    _begin()
    ctx = Ctx(tuple(needs) + (False,) * 2)
    C._TapSplitConv2d.forward(ctx, _cfake((N, cin, hw, hw), BF), _cfake((cout, cin, k, k), BF),
                              _cfake((cout,), F32), (p, p), (d, d))
    _ev('backward')
    ho = _hw(hw, k, 1, p, d)
    return _end(C, C._TapSplitConv2d.backward(ctx, _tag(fake((N, cout, ho, ho), dydtype), 'DY')))


def run_persample(C, shape, needs=(True, True, True), bias=True):
    cin, cout, k, s, p, d, hw = shape
    _begin()
    ctx = Ctx(tuple(needs) + (False,) * 2)
    C._MfmaConvPerSample.forward(ctx, _cfake((N, cin, hw, hw), BF),
                                 _cfake((N, cout, cin, k, k), BF),
                                 _cfake((N, cout), F32) if bias else None, (p, p), (d, d))
    _ev('backward')
    ho = _hw(hw, k, 1, p, d)
    return _end(C, C._MfmaConvPerSample.backward(ctx, _tag(fake((N, cout, ho, ho), BF), 'DY')))


def run_deconv(C, shape, bias=True):
    """``conv_transpose2d`` and, where it files a tuning entry, both of that entry's candidates."""
    cin, cout, k, s, p, hw = shape
    _begin()
    y = C.conv_transpose2d(_cfake((N, cin, hw, hw), BF), fake((cin, cout, k, k), BF),
                           _cfake((cout,), F32) if bias else None, s, p)
    outs = [y]
    for fns in dict.values(C._DECONV_PENDING):
        for name, fn in sorted(fns().items()):
            _ev('candidate', name)
            outs.append(fn())
    dict.clear(C._DECONV_PENDING)
    return _end(C, outs)


def _pm_ok(shape, pm):
    return not pm or (shape[1] > 16 and shape[4] > 0)


TTT = (True, True, True)


def _k10_block(shapes, needs=NEEDS, slopes=(1.0, 0.2)):
    """A reduced product of ``shapes`` with pad mode, weight kind, slope and the needed gradients.
    What interacts is crossed in full: on K10_FULL (k10, MIOpen, thin) at zero padding every need
    subset meets both slopes and every weight kind. Under a pad mode (fold, SN dot on the folded
    dx) and on the other shapes (a threshold each) the identity slope meets NEEDS_MAIN, and on
    K10_FEW the leaky slope the case that needs everything."""
    return [dict(shape=s, pmode=pm, sn=sn, wkind=wk, slope=sl, needs=nd)
            for s in shapes for pm in (0, 1, 2) if _pm_ok(s, pm) for sn, wk in WKIND
            for sl in slopes for nd in needs
            if (s in K10_FULL and pm == 0) or
            (sl == 1.0 and nd in NEEDS_MAIN and (pm < 2 or s in K10_FULL) and
             (pm == 0 or wk == 'param')) or
            (s in K10_FEW and nd == TTT and wk == 'param' and pm < 2)]


def _set(**kw):
    def f(C, mp, X):
        for k, v in kw.items():
            if k == 'graph':
                C._GRAPH_ROUTING[0] = v
            elif k == 'v2':
                X.v2 = v
            elif k == 'seed':
                mp.setattr(C, '_WGRAD_CHOICE', _Choices('choice', v))
            elif k == 'deconv_seed':
                mp.setattr(C, '_DECONV_CHOICE', _Choices('deconv_choice', v))
            else:
                mp.setattr(C, k, v)
    return f


def groups():
    """[(name, runner, switches, [case keyword dicts])] in enumeration order."""
    out = [('k10', run_k10, _set(), _k10_block(K10)),
           ('k10 wflip', run_k10, _set(), [dict(c, wflip=True) for c in _k10_block(K10_S1)]),
           ('k10 fp32 input', run_k10, _set(),
            [dict(c, xdtype=F32) for c in _k10_block(K10_FEW, slopes=(1.0,))
             if c['pmode'] or c['shape'] == K10[13]]),
           ('k10 graph', run_k10, _set(graph=1),
            [dict(c, wflip=wf) for c in _k10_block(K10, NEEDS[:2]) for wf in (False, True)
             if not wf or c['shape'] in K10_S1]),
           ('k10 no dest', run_k10, _set(), [dict(c, dest=False) for c in
                                             _k10_block(K10_FEW, NEEDS_W[:2], (1.0,))]),
           ('k10 min_pix0', run_k10, _set(_STRIDED_DGRAD_MIN_PIX=0), _k10_block(K10[4:8])),
           ('k10 strided off', run_k10, _set(_STRIDED_DGRAD=False),
            _k10_block(K10[4:6], NEEDS[:2])),
           ('k10 phase loop', run_k10, _set(_STRIDED_ONE_LAUNCH=False, _STRIDED_DGRAD_MIN_PIX=0),
            _k10_block(K10[4:8] + K10[14:15], NEEDS[:2])),
           ('k10 tappack off', run_k10, _set(_TAPPACK=False), _k10_block(K10[8:12])),
           ('k10 sn ratio 0', run_k10, _set(_SN_DOT_RATIO=0.0), _k10_block(K10[:2])),
           ('k10 flip counter', run_k10, _set(_TEST_FLIP_WGRAD=[10 ** 9, 0]),
            _k10_block(K10_FEW, NEEDS[:1], (1.0,)))]
    for res in (BF, F32):
        out.append(('k10 residual %s' % _DT[res], run_k10, _set(),
                    [dict(c, res=res) for c in _k10_block(K10_FEW[:2], NEEDS[:2], (1.0,))]))
    for ov in ('1', 'bias', 'small'):
        out.append(('k10 overlap ' + ov, run_k10, _set(_OVERLAP_BWD=ov),
                    _k10_block(K10 if ov == 'small' else K10_FEW)))
    out.append(('k10 overlap small graph', run_k10, _set(_OVERLAP_BWD='small', graph=1),
                _k10_block(K10_FEW, NEEDS[:2])))
    out.append(('k10 overlap conv log', run_k10, _set(_OVERLAP_BWD='1', _CONV_LOG=[]),
                _k10_block(K10_FEW, NEEDS[:1], (1.0,))))
    for mode, seed, v2, graph in itertools.product(('1', '0', 'auto'),
                                                    (None, 'k11', 'k11v2', 'miopen'),
                                                    (False, True), (0, 1)):
        if (mode, seed, v2, graph) == ('1', None, False, 0) or (graph and seed == 'k11'):
            continue
        out.append(('k10 wgrad %s %s v2=%d graph=%d' % (mode, seed, v2, graph), run_k10,
                    _set(_MFMA_WGRAD=mode, seed=seed, v2=v2, graph=graph),
                    _k10_block(K10_WG, NEEDS_W[:1], (1.0,))))
    tp = [dict(shape=s, pmode=pm, slope=sl, needs=nd, xdtype=xd, wdtype=wd)
          for s in TAPPACK for pm in (0, 1, 2) if _pm_ok(s, pm) for sl in (1.0, 0.2)
          for nd in NEEDS for xd, wd in ((BF, BF), (F32, F32), (BF, F32))
          if (s in TAPPACK_FEW and xd == wd == BF) or
          (pm < 2 and sl == 1.0 and nd in NEEDS_MAIN and (xd == wd or nd == TTT))]
    out.append(('tappack', run_tappack, _set(), tp))
    out.append(('tappack switches', run_tappack,
                _set(_STRIDED_DGRAD=False, _MFMA_MIN_DGRAD_BLOCKS=10 ** 6, _MFMA_WGRAD='0',
                     _OVERLAP_BWD='1'), tp[::3]))
    out.append(('tappack phase loop', run_tappack, _set(_STRIDED_ONE_LAUNCH=False),
                [c for c in tp[::3] if c['shape'][3] > 1]))
    out.append(('tappack flip counter', run_tappack, _set(_TEST_FLIP_WGRAD=[10 ** 9, 0]),
                tp[::21]))
    out.append(('tapsplit', run_tapsplit, _set(),
                [dict(shape=s, needs=nd, dydtype=dt) for s in TAPSPLIT[:4] for nd in NEEDS
                 for dt in (BF, F32)]))
    out.append(('persample', run_persample, _set(),
                [dict(shape=s, needs=nd, bias=b) for s in PERSAMPLE for nd in NEEDS
                 for b in (True, False) if b or not nd[2]]))
    for force, seed, one, graph in itertools.product((None, 'k10s', 'miopen'),
                                                     (None, 'k10s', 'miopen'), (True, False),
                                                     (0, 1)):
        out.append(('deconv force=%s seed=%s one=%d graph=%d' % (force, seed, one, graph),
                    run_deconv, _set(_DECONV_FORCE=force, deconv_seed=seed,
                                     _STRIDED_ONE_LAUNCH=one, graph=graph),
                    [dict(shape=s, bias=b) for s in DECONV for b in (True, False)]))
    return out


def trace_all():
    """{group name: [events per case]}."""
    out = {}
    for name, run, switches, cases in groups():
        with bwd_harness() as (C, mp, X):
            try:
                switches(C, mp, X)
                out[name] = [run(C, **kw) for kw in cases]
            finally:
                C._GRAPH_ROUTING[0] = 0
    return out


def _plain(v):
    return json.loads(json.dumps(v, default=lambda o: _enc(o)))


def spec():
    """What the table's rows stand for: every group's cases, in enumeration order, hashed (the
    list itself is this file's)."""
    import hashlib
    cases = [[name, _plain(cs)] for name, _, _, cs in groups()]
    return {'batch': N, 'groups': [[n, len(c)] for n, c in cases],
            'cases_sha1': hashlib.sha1(json.dumps(cases).encode()).hexdigest()}


def write_table(traced):
    """{name: [events per case]} interned: distinct atoms (an event's name and each of its
    arguments), distinct events (of atom ids) and distinct event lists (of event ids), both written
    as [b, p, s, ids...], see _delta, and
    per group the list id of every case (as differences)."""
    atoms, events, lists, routes = {}, {}, {}, {}
    for name, rows in traced.items():
        routes[name] = [lists.setdefault(tuple(events.setdefault(
            tuple(atoms.setdefault(json.dumps(a), len(atoms)) for a in e), len(events))
            for e in ev), len(lists)) for ev in rows]
    dump = functools.partial(json.dumps, separators=(',', ':'))
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, 'w') as f:
        f.write('{"spec": %s,\n"atoms": [\n%s\n],\n"events": %s,\n"lists": %s,\n'
                '"routes": {\n%s\n}}\n' % (
                    json.dumps(spec()), _wrap(list(atoms)), dump(_delta(list(events))),
                    dump(_delta(list(lists))),
                    ',\n'.join('%s: %s' % (json.dumps(k), dump([b - a for a, b in zip([0] + v, v)]))
                              for k, v in routes.items())))
    return sum(len(v) for v in traced.values()), len(lists)


def _wrap(items, width=116):
    lines = ['']
    for it in items:
        if lines[-1] and len(lines[-1]) + len(it) + 2 > width:
            lines.append('')
        lines[-1] += (', ' if lines[-1] else '') + it
    return ',\n'.join(lines)


def _delta(lists, back=256):
    """Each list as [b, p, s, ids...]: the first p and last s ids of the list b places before it
    (the closest of the ``back`` before it) around its own."""
    out = []
    for i, cur in enumerate(lists):
        best = (0, -1, 0, 0)
        for b in range(1, min(back, i) + 1):
            prev, p, s = lists[i - b], 0, 0
            while p < min(len(prev), len(cur)) and prev[p] == cur[p]:
                p += 1
            while s < min(len(prev), len(cur)) - p and prev[-1 - s] == cur[-1 - s]:
                s += 1
            best = max(best, (p + s, -b, p, s))
        out.append([-best[1], best[2], best[3]] + list(cur[best[2]:len(cur) - best[3]]))
    return out


def _undelta(rows):
    out = []
    for i, row in enumerate(rows):
        b, p, s = row[:3]
        prev = out[i - b] if i else []
        out.append(prev[:p] + row[3:] + prev[len(prev) - s:])
    return out


def load_table():
    """{'spec', 'events': the distinct event lists, 'routes': {group: [index into events]}}."""
    with open(TABLE) as f:
        t = json.load(f)
    atoms = t.pop('atoms')
    events = [[atoms[a] for a in e] for e in _undelta(t['events'])]
    t['events'] = [[events[i] for i in ids] for ids in _undelta(t.pop('lists'))]
    t['routes'] = {k: list(itertools.accumulate(v)) for k, v in t['routes'].items()}
    return t


@pytest.fixture(scope='module')
def traced():
    return trace_all()


def test_backwards_match_the_recorded_table(traced):
    table = load_table()
    assert table['spec'] == spec(), 'the case lists changed: re-record'
    assert set(table['routes']) == set(traced)
    cases = {name: cs for name, _, _, cs in groups()}
    bad, total = [], 0
    for name, rows in traced.items():
        want = table['routes'][name]
        assert len(want) == len(rows), name
        total += len(rows)
        for i, (ev, w) in enumerate(zip(rows, want)):
            if _plain(ev) != table['events'][w]:
                bad.append((name, cases[name][i], _plain(ev), table['events'][w]))
    msg = '\n'.join('%s %s\n  got      %s\n  recorded %s' % b for b in bad[:6])
    assert not bad, '%d of %d backward traces differ from the table:\n%s' % (len(bad), total, msg)


def _classes(name, ev):
    """The backward classes one case's recorded events fall into."""
    out = set()
    names = [e[0] for e in ev]
    if 'backward' not in names:  # conv_transpose2d
        first = [e for e in ev if e[0] in ('conv2d_dgrad_strided', 'conv_phase_scatter',
                                           'F.conv_transpose2d')]
        if first:
            out.add({'conv2d_dgrad_strided': 'deconv one launch',
                     'conv_phase_scatter': 'deconv phase loop',
                     'F.conv_transpose2d': 'deconv miopen'}[first[0][0]])
        return out
    bwd = ev[names.index('backward'):]
    bn = [e[0] for e in bwd]
    logs = [e for e in bwd if e[0].startswith('log')]
    dg = [e for e in logs if e[1] == 'dgrad']
    fam = name.split(' ')[0]
    if fam == 'k10':
        kind = 'none'
        if dg:
            path = dg[0][2]
            i = bwd.index(dg[0])
            nxt = bwd[i + 1][0].split('@')[0]
            kind = {'k10p': 'thin', 'k10s': 'k10s', 'miopen': 'miopen'}.get(path) or (
                'bt' if nxt == 'conv2d_dgrad_mfma' else
                'wflip' if str(bwd[i + 1][2]).startswith('F[') else 'flip')
        elif any(e[0] == 'log' and e[2] == 'k11' and 'thin-out' in e[4] for e in bwd):
            kind = 'thin'
        out.add('k10 dgrad ' + kind)
        if dg:
            out.add('fold' if 'pad_nhwc_bwd' in bn else 'no fold')
        side = [n for n in bn if n.endswith('@side') and not n.startswith(('log', 'endlog'))]
        if 'overlap' in name:
            out.add('side none' if not side else 'side bias only'
                    if all(n.startswith('bias_act_bwd') for n in side) else 'side weight')
        for e in bwd:
            nm = e[0].split('@')[0]
            if nm == 'conv2d_wgrad_mfma' and e[16] is not None:
                out.add('sn shortcut taken' if len(e[16]) == 5 else 'sn shortcut refused')
            if nm == 'conv2d_wgrad_mfma' and not any('thin-out' in str(l[4]) for l in logs):
                out.add('wgrad k11 v%d' % e[15])
                out.add('dest handed out' if e[17] is not None else 'no dest')
            if nm == 'aten.convolution_backward' and e[-1] == [False, True, False]:
                out.add('wgrad miopen')
            if nm == 'wgrad_pending':
                out.add('wgrad pending')
    elif fam == 'tappack' and dg:
        out.add('tappack dgrad ' + dg[0][2])
    elif fam == 'tappack' and 'aten.convolution_backward' in bn:
        out.add('tappack dgrad miopen')
    return out


CLASSES = ['k10 dgrad ' + k for k in ('none', 'thin', 'wflip', 'bt', 'flip', 'k10s', 'miopen')] + \
    ['tappack dgrad ' + k for k in ('k10', 'k10s', 'miopen')] + \
    ['fold', 'no fold', 'sn shortcut taken', 'sn shortcut refused', 'side none',
     'side bias only', 'side weight', 'wgrad miopen', 'wgrad k11 v0', 'wgrad k11 v1',
     'wgrad k11 v2', 'wgrad pending', 'dest handed out', 'no dest', 'deconv one launch',
     'deconv phase loop', 'deconv miopen']


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
    assert not short, 'backward classes with fewer than 20 recorded cases: %s' % short


def test_planners_are_pure():
    """``_bwd_route`` and ``_wgrad_choice`` launch and allocate nothing: the extension, MIOpen
    and the side stream all raise."""
    class NoExt(object):
        def __getattr__(self, name):
            raise AssertionError('the extension was asked for %s' % name)

    def no(*a, **k):
        raise AssertionError('a sink was called')

    with bwd_harness(NoExt()) as (C, mp, X):
        for nm in ('_dgrad_weight', '_take_grad_dest', '_bwd_side_stream', '_Logged', '_wgrad',
                   '_strided_dgrad', '_flip_t'):
            mp.setattr(C, nm, no)
        mp.setattr(torch.ops.aten, 'convolution_backward', no)
        kinds = set()
        for (cin, cout, k, s, p, d, hw), pm, sn, ov in [
                (K10[0], 0, True, '0'), (K10[1], 1, True, 'small'), (K10[1], 0, False, '1'),
                (K10[3], 0, False, 'bias'), (K10[5], 2, False, '0'), (K10[8], 0, False, '0')]:
            mp.setattr(C, '_OVERLAP_BWD', ov)
            ho = _hw(hw, k, s, p, d)
            for wflip in (False, True):
                args = ((N, cout, ho, ho), (N, 64, hw, hw), (64, 64, k, k), (s, s), (p, p),
                        (d, d), pm, 1.0, True, True, True, sn, cin, cout, wflip)
                r = C._bwd_route(*args)
                assert isinstance(r, tuple) and r == C._bwd_route(*args)
                kinds.add(r.dgrad)
        assert kinds == {'miopen', 'wflip', 'bt', 'flip', 'k10s', 'thin'}
        t = fake((N, 64, 8, 8))
        key = C._wgrad_key(t, t, fake((64, 64, 3, 3)), (1, 1), (1, 1), (1, 1), 64, 64, BF,
                           (None,) * 5, 1)
        assert key.sn == 'sndx' and key.pmode == 1 and key[:6] == (
            (N, 64, 8, 8), (N, 64, 8, 8), (64, 64, 3, 3), (1, 1), (1, 1), (1, 1))
        assert C._wgrad_choice(key, '1', ('k11',), False, False) == ('k11', 0, False)
        assert C._wgrad_choice(key, '0', ('k11',), False, False) == ('miopen', 'miopen', False)
        assert C._wgrad_choice(key, '0', ('k11', 'k11v2'), True, False) == ('k11', 0, True)


if __name__ == '__main__':
    if '--record' in sys.argv[1:]:
        print('recorded %d cases, %d distinct event lists -> %s' % (
            write_table(trace_all()) + (TABLE,)))
    elif '--counts' in sys.argv[1:]:
        print(json.dumps(class_counts(load_table()), indent=1))
    else:
        sys.exit(pytest.main([__file__] + sys.argv[1:]))
