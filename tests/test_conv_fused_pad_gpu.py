"""Reflect / replicate padding read in place by the conv loaders (``pad_mode`` of conv2d_mfma /
conv2d_wgrad_mfma / im2col_pack, ``ops/conv.py`` ``_FUSED_PAD``).

A conv over x with padding (ph, pw) and ``pad_mode`` 1 (reflect) / 2 (replicate) must produce
what the zero-padding conv produces on ``F.pad(x, (pw, pw, ph, ph), mode)`` at padding 0, with no
padded tensor made. Every kernel case is checked twice: against the fp32 PyTorch result on the
padded input (the criteria of tests/test_conv_rw_gpu.py and of the k11 tests in
tests/test_kernels_gpu.py) and bitwise against the same forced kernel run on the explicitly
padded operand (``pad_nhwc_fwd``): the two launches see the same M, k-steps and split, so they
accumulate the same values in the same order. Reference: the ``padding_mode='reflect'``
convolutions of the reference's layers/conv.py (cuDNN on a padded copy there)."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
MODES = {'reflect': 1, 'replicate': 2}

# tile (IMAGINAIRE_AMD_CONV_V: 1, 4, 5, 6 = row-window),
# (B, Cin, Cout, H, W, KH, KW, stride, pad), dilation
FWD_CASES = [
    ('1', (2, 64, 64, 9, 11, 3, 3, 1, 1), 1),
    ('1', (1, 64, 128, 8, 8, 4, 4, 2, 1), 1),
    ('1', (1, 128, 64, 6, 7, 7, 7, 1, 3), 1),    # pad 3 on 6 rows: corners reflect in both axes
    ('1', (1, 64, 64, 10, 10, 3, 3, 1, 2), 2),   # dilation 2
    ('4', (1, 64, 128, 16, 16, 3, 3, 1, 1), 1),  # 16 segments per block
    ('4', (1, 64, 128, 2, 256, 3, 3, 1, 1), 1),  # a full-row segment on a 2-row image
    ('4', (1, 128, 128, 8, 32, 5, 5, 1, 2), 1),
    ('4', (1, 64, 128, 15, 15, 4, 4, 1, 2), 1),  # the KW = 4 build
    ('5', (1, 64, 256, 8, 32, 3, 3, 1, 1), 1),
    ('5', (1, 64, 256, 8, 32, 5, 5, 1, 2), 1),
    ('6', (1, 128, 128, 16, 100, 7, 7, 1, 3), 1),
    ('6', (2, 64, 128, 33, 47, 4, 4, 2, 1), 1),  # the stride-2 de-interleaved window
    ('6', (1, 64, 64, 9, 9, 3, 3, 2, 1), 1),
    ('6', (2, 64, 64, 32, 64, 3, 3, 1, 1), 1),
    ('6n', (1, 128, 64, 16, 32, 3, 3, 1, 1), 1),  # Cout 64, K = 1152: the narrow variant
    ('1w', (3, 64, 64, 9, 11, 3, 3, 1, 1), 1),   # v1 256-pixel blocks (IMAGINAIRE_AMD_CONV_BM)
    ('1w', (2, 64, 128, 17, 9, 4, 4, 2, 1), 1),
]
SPLITK_CASES = [
    ('1', (2, 64, 64, 9, 11, 3, 3, 1, 1), 1),
    ('4', (1, 128, 128, 8, 32, 5, 5, 1, 2), 1),
    ('6', (1, 128, 128, 16, 100, 7, 7, 1, 3), 1),
]


def _inputs(case, seed=5):
    B, cin, cout, H, W, kh, kw, s, p = case
    torch.manual_seed(seed)
    x = torch.randn(B, cin, H, W, device='cuda').to(torch.bfloat16).contiguous(memory_format=CL)
    # asymmetric weights: catches row / column swaps in the fragment maps
    w = (torch.randn(cout, cin, kh, kw, device='cuda') / (cin * kh * kw) ** 0.5 +
         torch.arange(cout, device='cuda').view(-1, 1, 1, 1) * 1e-3)
    w = w.to(torch.bfloat16).contiguous(memory_format=CL)
    b = torch.randn(cout, device='cuda') * 0.1
    return x, w, b


def _run(X, x, w, b, s, p, d, pm, tile, splitk=None, res=None):
    """``tile``: the forced k10 tile; '6n' also requires the narrow row-window variant to have
    run, '1w' forces v1's 256-pixel blocks."""
    os.environ['IMAGINAIRE_AMD_CONV_V'] = tile[0]
    if splitk:
        os.environ['IMAGINAIRE_AMD_CONV_SPLITK'] = splitk
    if tile == '1w':
        os.environ['IMAGINAIRE_AMD_CONV_BM'] = '256'
    try:
        y = X.conv2d_mfma(x, w, b, s, s, p, p, d, d, 0.2, 1, -1, res, None, pad_mode=pm)
        var = X.conv_last_variant()
        if var == 6:
            assert X.conv_last_rw_narrow() == (tile == '6n'), tile
    finally:
        os.environ.pop('IMAGINAIRE_AMD_CONV_V')
        os.environ.pop('IMAGINAIRE_AMD_CONV_SPLITK', None)
        os.environ.pop('IMAGINAIRE_AMD_CONV_BM', None)
    return y, var


def _check_forward(tile, case, d, mode, splitk=None):
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    B, cin, cout, H, W, kh, kw, s, p = case
    pm = MODES[mode]
    x, w, b = _inputs(case)
    y, var = _run(X, x, w, b, s, p, d, pm, tile, splitk)
    assert var == int(tile[0]), 'tile %s did not take %s (variant %d)' % (tile, case, var)
    ref = F.leaky_relu(F.conv2d(F.pad(x.float(), (p, p, p, p), mode=mode), w.float(), b, s, 0, d),
                       0.2)
    assert y.shape == ref.shape
    err = (y.float() - ref).abs().max().item()
    assert err <= 1e-2 * max(1.0, ref.abs().max().item()), err
    xp = X.pad_nhwc_fwd(x, p, p, p, p, pm - 1)
    assert tuple(xp.shape) == (B, cin, H + 2 * p, W + 2 * p)
    y0, var0 = _run(X, xp, w, b, s, 0, d, 0, tile, splitk)
    assert var0 == int(tile[0]), (case, var0)
    assert torch.equal(y, y0)


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('tile,case,d', FWD_CASES)
def test_forward_matches_fp32_and_padded_operand(tile, case, d, mode):
    _check_forward(tile, case, d, mode)


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('tile,case,d', SPLITK_CASES)
def test_forward_splitk(tile, case, d, mode):
    _check_forward(tile, case, d, mode, splitk='2')


@pytest.mark.parametrize('mode', sorted(MODES))
def test_im2col_pack_gathers_padding(mode):
    """A 3-channel 7x7 pad-3 stem on a 12x20 image: the packed operand equals the packing of the
    padded image, and the 1x1 GEMM on it matches the fp32 conv."""
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.ops import conv as C
    X = _ext.ext()
    pm = MODES[mode]
    torch.manual_seed(9)
    x = torch.randn(1, 3, 12, 20, device='cuda')
    w = torch.randn(64, 3, 7, 7, device='cuda') / 147 ** 0.5
    b = torch.randn(64, device='cuda') * 0.1
    col = X.im2col_pack(x, 7, 7, 1, 1, 3, 3, 1, 1, 192, pad_mode=pm)
    xp = F.pad(x, (3, 3, 3, 3), mode=mode)
    col0 = X.im2col_pack(xp, 7, 7, 1, 1, 0, 0, 1, 1, 192)
    assert tuple(col.shape) == (1, 192, 12, 20)
    assert torch.equal(col, col0)
    y = X.conv2d_mfma(col, C._pack_taps(w, 192, 64), b, 1, 1, 0, 0, 1, 1, 1.0)
    ref = F.conv2d(xp.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), b)
    err = (y.float() - ref).abs().max().item()
    assert err <= 1e-2 * max(1.0, ref.abs().max().item()), err


# kernel, (B, Cin, Cout, H, W, KH, KW, stride, pad): k11 generic / ROWS (multi-tap off) /
# multi-tap / v2 (variant 2, shapes conv2d_wgrad_v2_eligible takes)
WGRAD_CASES = [
    ('generic', (2, 64, 64, 9, 11, 3, 3, 1, 1)),
    ('generic', (1, 64, 128, 8, 8, 4, 4, 2, 1)),
    ('rows', (1, 64, 64, 4, 64, 3, 3, 1, 1)),
    ('mt', (1, 64, 128, 4, 64, 3, 3, 1, 1)),
    ('mt', (1, 64, 64, 4, 64, 5, 5, 1, 2)),
    ('mt', (1, 64, 64, 4, 64, 7, 7, 1, 3)),
    ('v2', (1, 128, 128, 16, 16, 3, 3, 1, 1)),
    ('v2', (1, 128, 128, 8, 32, 5, 5, 1, 2)),
]


K11_KERNELS = {'generic': 0, 'rows': 1, 'mt': 2, 'v2': 3}


def _wgrad(X, kind, dy, x, kh, kw, s, p, pm):
    if kind == 'rows':
        os.environ['IMAGINAIRE_AMD_WGRAD_MT'] = '0'
    try:
        g = X.conv2d_wgrad_mfma(dy, x, kh, kw, s, s, p, p, 1, 1, -1, -1, False, 1,
                                2 if kind == 'v2' else 1, None, None, pad_mode=pm)
        assert X.wgrad_last_kernel() == K11_KERNELS[kind], (kind, X.wgrad_last_kernel())
        return g
    finally:
        os.environ.pop('IMAGINAIRE_AMD_WGRAD_MT', None)


def _wgrad_inputs(case, seed=14):
    B, cin, cout, H, W, kh, kw, s, p = case
    torch.manual_seed(seed)
    x = torch.randn(B, cin, H, W, device='cuda').to(torch.bfloat16).contiguous(memory_format=CL)
    Ho, Wo = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
    dy = torch.randn(B, cout, Ho, Wo, device='cuda').to(torch.bfloat16).contiguous(
        memory_format=CL)
    return x, dy


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('kind,case', WGRAD_CASES)
def test_wgrad_matches_fp32_and_padded_operand(kind, case, mode):
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    B, cin, cout, H, W, kh, kw, s, p = case
    pm = MODES[mode]
    x, dy = _wgrad_inputs(case)
    xp = X.pad_nhwc_fwd(x, p, p, p, p, pm - 1)
    if kind == 'v2':
        assert X.conv2d_wgrad_v2_eligible(dy, x, kh, kw, s, s, 1, 1, pad_mode=pm)
        assert X.conv2d_wgrad_v2_eligible(dy, xp, kh, kw, s, s, 1, 1)
    got = _wgrad(X, kind, dy, x, kh, kw, s, p, pm)
    ref = torch.nn.grad.conv2d_weight(F.pad(x.float(), (p, p, p, p), mode=mode),
                                      (cout, cin, kh, kw), dy.float(), s, 0)
    scale = max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    assert err <= 2e-3 * scale, err
    got0 = _wgrad(X, kind, dy, xp, kh, kw, s, 0, 0)
    assert torch.equal(got, got0)


# ---- autograd / layer level ---------------------------------------------------------------

def _block(kind, padding_mode='reflect'):
    from imaginaire_amd.layers import Conv2dBlock, Res2dBlock
    kw = dict(padding_mode=padding_mode, weight_norm_type='spectral',
              activation_norm_type='instance')
    if kind == 'res':
        return Res2dBlock(64, 64, **kw)
    return Conv2dBlock(64, 64, 4, 2, 1, nonlinearity='leakyrelu', **kw)


def _pair_of_blocks(kind, padding_mode='reflect'):
    from imaginaire_amd.layers import spectral_norm as snm
    torch.manual_seed(41)
    a = _block(kind, padding_mode).cuda().to(memory_format=CL)
    b = _block(kind, padding_mode).cuda().to(memory_format=CL)
    b.load_state_dict(a.state_dict())
    n = snm.install_batched_spectral_norm(a)
    assert n >= 1 and snm.install_batched_spectral_norm(b) == n
    return a, b


def _step(net, x, g, saved=None):
    xi = x.clone().requires_grad_(True)

    def pack(t):
        if saved is not None:
            saved.append(tuple(t.shape))
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = net(xi)
    y.backward(g.to(y.dtype))
    grads = {n: p.grad.clone() for n, p in net.named_parameters()}
    return y.detach(), xi.grad, grads


@pytest.fixture
def sn_shadow():
    from imaginaire_amd.layers import spectral_norm as snm
    old = snm._SN_SHADOW, snm._SN_FUSED
    snm._SN_SHADOW, snm._SN_FUSED = True, True
    yield
    snm._SN_SHADOW, snm._SN_FUSED = old


@pytest.mark.parametrize('dot_ratio', [0.0, 1e9])
@pytest.mark.parametrize('kind', ['res', 'down'])
def test_layers_fused_equal_pad_then_conv(monkeypatch, sn_shadow, kind, dot_ratio):
    """Reflect-padded spectral-norm + instance-norm blocks (64 -> 64 at 16 x 16, bf16 autocast):
    no ``pad`` call with the switch on, and bitwise the outputs / dx / db of pad-then-conv; dW
    bitwise when <G, W> comes from the k11 epilogue on both sides (``dot_ratio`` 0: the same
    pinned k11 kernel), else to the k11 fp32 criterion (the data-gradient identity sums the
    folded dx against x instead of dx against the padded x)."""
    from imaginaire_amd.ops import conv as C
    monkeypatch.setattr(C, '_SN_DOT_RATIO', dot_ratio)
    calls = []
    orig_pad = C.pad

    def counting_pad(*a, **k):
        calls.append(1)
        return orig_pad(*a, **k)
    monkeypatch.setattr(C, 'pad', counting_pad)
    on, off = _pair_of_blocks(kind)
    torch.manual_seed(42)
    x = torch.randn(32, 64, 16, 16, device='cuda').contiguous(memory_format=CL)
    monkeypatch.setattr(C, '_FUSED_PAD', True)
    saved_on = []
    hw = 16 if kind == 'res' else 8
    g = torch.randn(32, 64, hw, hw, device='cuda').contiguous(memory_format=CL)
    y1, dx1, g1 = _step(on, x, g, saved_on)
    assert len(calls) == 0, 'the fused path padded %d times' % len(calls)
    monkeypatch.setattr(C, '_FUSED_PAD', False)
    saved_off = []
    y0, dx0, g0 = _step(off, x, g, saved_off)
    assert len(calls) >= 1
    # the conv input is saved at its unpadded size (pad-then-conv saves the padded copy)
    padded = [s for s in saved_off if len(s) == 4 and s[2:] == (18, 18)]
    assert padded and not [s for s in saved_on if len(s) == 4 and s[2:] == (18, 18)]
    assert [s for s in saved_on if len(s) == 4 and s[1:] == (64, 16, 16)]
    assert torch.equal(y1, y0)
    assert torch.equal(dx1, dx0)
    assert set(g1) == set(g0)
    for n in g1:
        if g1[n].dim() == 4 and dot_ratio != 0.0:
            scale = max(1.0, g0[n].abs().max().item())
            err = (g1[n].float() - g0[n].float()).abs().max().item()
            assert err <= 2e-3 * scale, (n, err)
        else:
            assert torch.equal(g1[n], g0[n]), n


def _conv_args(mode, cin=64, cout=64, hw=16, B=32, seed=43):
    torch.manual_seed(seed)
    x = torch.randn(B, cin, hw, hw, device='cuda').contiguous(memory_format=CL)
    w = (torch.randn(cout, cin, 3, 3, device='cuda') / (cin * 9) ** 0.5).contiguous(
        memory_format=CL)
    b = torch.randn(cout, device='cuda') * 0.1
    return x, w, b


@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
def test_conv2d_fused_equals_pad_then_conv_with_grads(monkeypatch, mode):
    """ops.conv.conv2d on plain weights, both modes: y, dx, dW, db bitwise equal to
    pad-then-conv (the same k10 / k11 kernels on both sides), no ``pad`` call when fused."""
    from imaginaire_amd.ops import conv as C
    calls = []
    orig_pad = C.pad
    monkeypatch.setattr(C, 'pad', lambda *a, **k: (calls.append(1), orig_pad(*a, **k))[1])
    x, w, b = _conv_args(mode)
    g = torch.randn(32, 64, 16, 16, device='cuda').contiguous(memory_format=CL)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(C, '_FUSED_PAD', fused)
        calls.clear()
        xi, wi, bi = (t.clone().requires_grad_(True) for t in (x, w, b))
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = C.conv2d(xi, wi, bi, 1, 1, 1, 1, mode)
        y.backward(g.to(y.dtype))
        assert (len(calls) == 0) == fused
        outs.append((y.detach(), xi.grad, wi.grad, bi.grad))
    ref = F.conv2d(F.pad(x.to(torch.bfloat16).float(), (1, 1, 1, 1), mode=mode),
                   w.to(torch.bfloat16).float(), b)
    err = (outs[0][0].float() - ref).abs().max().item()
    assert err <= 1e-2 * max(1.0, ref.abs().max().item()), err
    for name, a, c in zip(('y', 'dx', 'dw', 'db'), outs[0], outs[1]):
        assert torch.equal(a, c), name


def test_conv2d_residual_epilogue_with_reflect(monkeypatch):
    """``conv2d(..., padding_mode='reflect', residual=r)`` adds r in the k10 epilogue and equals
    the pad-then-conv result plus r bitwise (store_chunk rounds the conv output to bf16, adds,
    rounds again: the bf16 conv followed by a bf16 add)."""
    from imaginaire_amd.ops import conv as C
    x, w, b = _conv_args('reflect')
    r = torch.randn(32, 64, 16, 16, device='cuda').to(torch.bfloat16).contiguous(memory_format=CL)
    seen = []
    orig = C._MfmaConv2d

    class Spy(orig):
        @staticmethod
        def forward(ctx, *a):
            seen.append((len(a) > 7 and a[7] is not None, a[9] if len(a) > 9 else 0))
            return orig.forward(ctx, *a)
    monkeypatch.setattr(C, '_MfmaConv2d', Spy)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        monkeypatch.setattr(C, '_FUSED_PAD', True)
        y1 = C.conv2d(x, w, b, 1, 1, 1, 1, 'reflect', residual=r)
        assert seen == [(True, 1)], seen   # the residual rode in the fused-pad k10 launch
        monkeypatch.setattr(C, '_FUSED_PAD', False)
        y0 = C.conv2d(x, w, b, 1, 1, 1, 1, 'reflect') + r
    assert y1.dtype == torch.bfloat16 and torch.equal(y1, y0)


def test_circular_keeps_pad_then_conv(monkeypatch):
    from imaginaire_amd.ops import conv as C
    calls = []
    orig_pad = C.pad
    monkeypatch.setattr(C, 'pad', lambda *a, **k: (calls.append(1), orig_pad(*a, **k))[1])
    monkeypatch.setattr(C, '_FUSED_PAD', True)
    x, w, b = _conv_args('circular')
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = C.conv2d(x, w, b, 1, 1, 1, 1, 'circular')
    assert len(calls) == 1
    ref = F.conv2d(F.pad(x.to(torch.bfloat16).float(), (1, 1, 1, 1), mode='circular'),
                   w.to(torch.bfloat16).float(), b)
    err = (y.float() - ref).abs().max().item()
    assert err <= 1e-2 * max(1.0, ref.abs().max().item()), err


def test_tappack_stem_fused(monkeypatch):
    """A reflect-padded 7x7 RGB stem (the tap-packed path): im2col_pack gathers the padding, no
    ``pad`` call, and y / dx / dW / db equal pad-then-conv bitwise."""
    from imaginaire_amd.ops import conv as C
    calls = []
    orig_pad = C.pad
    monkeypatch.setattr(C, 'pad', lambda *a, **k: (calls.append(1), orig_pad(*a, **k))[1])
    torch.manual_seed(44)
    x = torch.randn(1, 3, 48, 48, device='cuda').contiguous(memory_format=CL)
    w = torch.randn(64, 3, 7, 7, device='cuda') / 147 ** 0.5
    b = torch.randn(64, device='cuda') * 0.1
    g = torch.randn(1, 64, 48, 48, device='cuda').contiguous(memory_format=CL)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(C, '_FUSED_PAD', fused)
        calls.clear()
        xi, wi, bi = (t.clone().requires_grad_(True) for t in (x, w, b))
        with torch.autocast('cuda', dtype=torch.bfloat16):
            assert C.tappack_eligible(xi, wi, (1, 1), (3, 3), (1, 1), 1)
            y = C.conv2d(xi, wi, bi, 1, 3, 1, 1, 'reflect')
        y.backward(g.to(y.dtype))
        assert (len(calls) == 0) == fused
        outs.append((y.detach(), xi.grad, wi.grad, bi.grad))
    for name, a, c in zip(('y', 'dx', 'dw', 'db'), outs[0], outs[1]):
        assert torch.equal(a, c), name


def test_sn_tappack_stem_fused(monkeypatch, sn_shadow):
    """A spectrally normalised reflect-padded 7x7 RGB stem: the materialised weight goes to the
    tap-packed path, which gathers the padding — no ``pad`` call, results equal pad-then-conv."""
    from imaginaire_amd.layers import Conv2dBlock
    from imaginaire_amd.layers import spectral_norm as snm
    from imaginaire_amd.ops import conv as C
    calls = []
    orig_pad = C.pad
    monkeypatch.setattr(C, 'pad', lambda *a, **k: (calls.append(1), orig_pad(*a, **k))[1])
    torch.manual_seed(46)
    mk = lambda: Conv2dBlock(3, 64, 7, 1, 3, padding_mode='reflect',
                             weight_norm_type='spectral').cuda().to(memory_format=CL)
    on, off = mk(), mk()
    off.load_state_dict(on.state_dict())
    assert snm.install_batched_spectral_norm(on) == snm.install_batched_spectral_norm(off) == 1
    x = torch.randn(1, 3, 48, 48, device='cuda').contiguous(memory_format=CL)
    g = torch.randn(1, 64, 48, 48, device='cuda').contiguous(memory_format=CL)
    monkeypatch.setattr(C, '_FUSED_PAD', True)
    y1, dx1, g1 = _step(on, x, g)
    assert len(calls) == 0
    monkeypatch.setattr(C, '_FUSED_PAD', False)
    y0, dx0, g0 = _step(off, x, g)
    assert len(calls) >= 1
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n


# ---- LDS poison ---------------------------------------------------------------------------

@pytest.mark.parametrize('tile,case,d', [FWD_CASES[0], FWD_CASES[4], FWD_CASES[8], FWD_CASES[10]])
def test_fused_k10_never_reads_unwritten_lds(tile, case, d):
    """Bitwise the same output after the LDS of every CU was filled with NaN bits."""
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    x, w, b = _inputs(case, seed=8)
    s, p = case[7], case[8]
    y0, _ = _run(X, x, w, b, s, p, d, 1, tile)
    X.lds_poison()
    y1, var = _run(X, x, w, b, s, p, d, 1, tile)
    torch.cuda.synchronize()
    assert var == int(tile[0])
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(y0, y1)


@pytest.mark.parametrize('kind,case', [WGRAD_CASES[3], WGRAD_CASES[6]])
def test_fused_k11_never_reads_unwritten_lds(kind, case):
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    kh, kw, s, p = case[5:]
    x, dy = _wgrad_inputs(case, seed=16)
    g0 = _wgrad(X, kind, dy, x, kh, kw, s, p, 1)
    X.lds_poison()
    g1 = _wgrad(X, kind, dy, x, kh, kw, s, p, 1)
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all()
    assert torch.equal(g0, g1)


# ---- graph --------------------------------------------------------------------------------

def test_graph_replay_of_reflect_resblock(monkeypatch, sn_shadow):
    """Forward + backward of the reflect Res2dBlock captured on one stream after warm-up: two
    replays equal the eager result bitwise (the buffers the spectral norm's power iteration
    advances are put back before each run)."""
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.ops import conv as C
    from imaginaire_amd.utils.cuda_graph import graph_routing
    X = _ext.ext()
    monkeypatch.setattr(C, '_FUSED_PAD', True)
    calls = []
    orig_pad = C.pad
    monkeypatch.setattr(C, 'pad', lambda *a, **k: (calls.append(1), orig_pad(*a, **k))[1])
    net, _ = _pair_of_blocks('res')
    torch.manual_seed(45)
    x = torch.randn(32, 64, 16, 16, device='cuda').contiguous(memory_format=CL).requires_grad_(True)
    g = torch.randn(32, 64, 16, 16, device='cuda').to(torch.bfloat16).contiguous(memory_format=CL)
    params = list(net.parameters())

    def step():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = net(x)
        gr = torch.autograd.grad(y, [x] + params, g, allow_unused=True)
        return (y,) + tuple(t for t in gr if t is not None)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with graph_routing(), torch.cuda.stream(s):
        for _ in range(2):  # warm-up
            step()
        snap = {n: b.clone() for n, b in net.named_buffers()}

        def restore():
            with torch.no_grad():
                for n, b in net.named_buffers():
                    b.copy_(snap[n])
        restore()
        eager = [t.clone() for t in step()]
        restore()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            outs = step()
        X.flush_deferred_uploads()
        for _ in range(2):
            restore()
            graph.replay()
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(outs, eager)):
                assert torch.equal(a, b), i
    torch.cuda.current_stream().wait_stream(s)
    assert len(calls) == 0


# ---- host checks (no launch) ----------------------------------------------------------------

def test_host_checks():
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    case = (2, 64, 64, 3, 11, 3, 3, 1, 1)
    x, w, b = _inputs(case)
    with pytest.raises(RuntimeError, match='reflect padding'):   # ph >= H: one reflection only
        X.conv2d_mfma(x, w.new_zeros(64, 64, 7, 7).contiguous(memory_format=CL), b, 1, 1, 3, 3,
                      1, 1, 1.0, pad_mode=1)
    dy = torch.zeros(2, 64, 3, 11, device='cuda', dtype=torch.bfloat16).contiguous(
        memory_format=CL)
    with pytest.raises(RuntimeError, match='reflect padding'):
        X.conv2d_wgrad_mfma(dy, x, 7, 7, 1, 1, 3, 3, 1, 1, pad_mode=1)
    with pytest.raises(RuntimeError, match='nb == 1'):           # per-sample launches
        X.conv2d_mfma(x, torch.cat([w, w]).contiguous(memory_format=CL), None, 1, 1, 1, 1, 1, 1,
                      1.0, 2, pad_mode=1)
    with pytest.raises(RuntimeError, match='pad_mode'):
        X.conv2d_mfma(x, w, b, 1, 1, 1, 1, 1, 1, 1.0, pad_mode=3)
    x32 = x[:, :32].contiguous(memory_format=CL)                 # the Cin = 32 pair mode
    w32 = w[:, :32].contiguous(memory_format=CL)
    with pytest.raises(RuntimeError, match='Cin % 64'):
        X.conv2d_mfma(x32, w32, b, 1, 1, 1, 1, 1, 1, 1.0, pad_mode=2)


def test_forced_v3_runs_v1_with_pad_mode():
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    case = (1, 64, 256, 16, 16, 3, 3, 1, 1)
    x, w, b = _inputs(case)
    y0, var0 = _run(X, x, w, b, 1, 1, 1, 0, '3')
    assert var0 == 3
    y, var = _run(X, x, w, b, 1, 1, 1, 1, '3')
    assert var == 1
    ref = F.leaky_relu(F.conv2d(F.pad(x.float(), (1, 1, 1, 1), mode='reflect'), w.float(), b),
                       0.2)
    err = (y.float() - ref).abs().max().item()
    assert err <= 1e-2 * max(1.0, ref.abs().max().item()), err


def test_default_routing_sends_v3_shapes_to_v1_with_pad_mode():
    """A shape the default routing gives to v3 (Cout 256, 45 k-steps, an unsplit 256-tile grid;
    dilation 2 keeps it off v4 / v5 / row-window): with a padding mode it runs v1, bitwise equal
    to v1 on the padded operand."""
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    case = (1, 320, 256, 256, 256, 3, 3, 1, 2)
    x, w, b = _inputs(case)
    _, var0 = _run(X, x, w, b, 1, 2, 2, 0, '0')
    assert var0 == 3
    y, var = _run(X, x, w, b, 1, 2, 2, 1, '0')
    assert var == 1
    y1, var1 = _run(X, X.pad_nhwc_fwd(x, 2, 2, 2, 2, 0), w, b, 1, 0, 2, 0, '1')
    assert var1 == 1 and torch.equal(y, y1)
