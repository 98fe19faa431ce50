"""Reflect / replicate padding read in place by the k14 average pool (``avgpool_pad_fwd`` /
``avgpool_pad_bwd`` in csrc/pool.hip, ``avg_pool2d(..., padding_mode=)`` in ops/pool.py).

``avg_pool2d(x, k, s, p, padding_mode=m)`` must compute ``avg_pool2d(pad(x, (p,)*4, m), k, s)``
with no padded tensor made: the forward bitwise (same taps in the same order, same divisor), the
backward against the fp32 PyTorch result on an NCHW copy (PyTorch-ROCm's channels-last pool
backward is wrong, see ``test_avg_pool_nhwc`` in tests/test_kernels_gpu.py). The backward is not
compared bitwise with pad-then-pool, which rounds the padded gradient before folding it.
Reference: the ``ReflectionPad2d(1), AvgPool2d(3, stride=2)`` downsamplers of the reference's
discriminators/funit.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# (B, C, H, W, k, s, p)
CASES = [
    (2, 24, 19, 26, 3, 2, 1),   # FUNIT's geometry on odd sizes
    (1, 8, 2, 3, 3, 2, 1),      # H = p + 1: one pixel takes both reflections
    (1, 185, 7, 5, 3, 2, 1),    # the V = 1 path
    (2, 16, 5, 9, 5, 3, 2),
    (1, 8, 4, 4, 4, 1, 3),      # pad 3 on 4 pixels, stride 1
    (1, 24, 3, 3, 2, 2, 1),
    (1, 8, 9, 6, 3, 1, 2),
]


def _raise(*a, **k):
    raise AssertionError('a padding kernel ran on the fused path')


def _close(out, ref, dtype, what):
    """fp32: test_avg_pool_nhwc's atol = rtol = 1e-5. bf16: |err| <= 2^-8 |ref| + 1e-5, one
    rounding of an fp32-accumulated value (half an ulp: 2^-9 of the binade's top, 2^-8 of its
    bottom) with the fp32 summation noise of kernel and reference in the absolute term."""
    out = out.float()
    err = (out - ref).abs()
    rel = 1e-5 if dtype == torch.float32 else 2.0 ** -8
    bound = rel * ref.abs() + 1e-5
    print('%s: max |err| %.3e, max err / bound %.3f' % (what, err.max().item(),
                                                        (err / bound).max().item()))
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(v) for v in c))
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
def test_fused_pool_matches_pad_then_pool(monkeypatch, mode, dtype, case):
    from imaginaire_amd.ops import _ext, pool as P
    from imaginaire_amd.ops.conv import pad
    B, C, H, W, k, s, p = case
    X = _ext.ext()
    monkeypatch.setattr(P, '_FUSED_PAD', True)
    torch.manual_seed(11)
    x = torch.randn(B, C, H, W, device='cuda').to(dtype).contiguous(
        memory_format=CL).requires_grad_(True)

    # the fp32 reference on an NCHW copy, and the upstream gradient after its cast to dtype
    xr = x.detach().float().contiguous().requires_grad_(True)
    yr = F.avg_pool2d(F.pad(xr, (p,) * 4, mode=mode), k, s)
    g = torch.randn_like(yr).to(dtype)
    yr.backward(g.float())
    g = g.contiguous(memory_format=CL)

    # 1. the fused path ran: its grad_fn, and no padding kernel forward or backward
    with monkeypatch.context() as mp:
        mp.setattr(X, 'pad_nhwc_fwd', _raise)
        mp.setattr(X, 'pad_nhwc_bwd', _raise)
        y = P.avg_pool2d(x, k, s, p, padding_mode=mode)
        assert 'AvgPoolPadNHWC' in type(y.grad_fn).__name__
        (dx,) = torch.autograd.grad(y, x, g, retain_graph=True)
        (dx2,) = torch.autograd.grad(y, x, g)
        torch.cuda.synchronize()
    assert y.shape == yr.shape and y.dtype == dtype and dx.shape == x.shape and dx.dtype == dtype
    assert y.is_contiguous(memory_format=CL) and dx.is_contiguous(memory_format=CL)

    # 2. forward bitwise the existing kernel on the explicitly padded copy
    xp = pad(x.detach(), (p,) * 4, mode)
    assert xp.shape[2:] == (H + 2 * p, W + 2 * p)
    ye = P.avg_pool2d(xp.requires_grad_(True), k, s)
    assert type(ye.grad_fn).__name__.startswith('_AvgPoolNHWC')
    assert torch.equal(y, ye)

    # 3. forward and gradient against fp32
    _close(y.detach(), yr.detach(), dtype, 'forward')
    _close(dx, xr.grad, dtype, 'x.grad')

    # 4. determinism
    assert torch.equal(dx, dx2)


def test_zeros_mode_is_unchanged():
    from imaginaire_amd.ops import pool as P
    torch.manual_seed(12)
    x = torch.randn(2, 16, 19, 26, device='cuda').to(torch.bfloat16).contiguous(
        memory_format=CL).requires_grad_(True)
    y0 = P.avg_pool2d(x, 3, 2, 1)
    y1 = P.avg_pool2d(x, 3, 2, 1, padding_mode='zeros')
    assert type(y1.grad_fn).__name__.startswith('_AvgPoolNHWC')
    assert torch.equal(y0, y1)
    with pytest.raises(ValueError):
        P.avg_pool2d(x, 3, 2, 1, padding_mode='circular')


def _count_pads(monkeypatch, X):
    calls = {'fwd': 0, 'bwd': 0}
    fwd, bwd = X.pad_nhwc_fwd, X.pad_nhwc_bwd

    def cfwd(*a, **k):
        calls['fwd'] += 1
        return fwd(*a, **k)

    def cbwd(*a, **k):
        calls['bwd'] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(X, 'pad_nhwc_fwd', cfwd)
    monkeypatch.setattr(X, 'pad_nhwc_bwd', cbwd)
    return calls


@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
def test_switch_off_pads_then_pools(monkeypatch, mode):
    from imaginaire_amd.ops import _ext, pool as P
    calls = _count_pads(monkeypatch, _ext.ext())
    torch.manual_seed(13)
    x = torch.randn(2, 24, 19, 26, device='cuda').to(torch.bfloat16).contiguous(
        memory_format=CL).requires_grad_(True)
    monkeypatch.setattr(P, '_FUSED_PAD', True)
    y_on = P.avg_pool2d(x, 3, 2, 1, padding_mode=mode)
    assert calls == {'fwd': 0, 'bwd': 0}
    monkeypatch.setattr(P, '_FUSED_PAD', False)
    y_off = P.avg_pool2d(x, 3, 2, 1, padding_mode=mode)
    assert type(y_off.grad_fn).__name__.startswith('_AvgPoolNHWC')
    y_off.backward(torch.ones_like(y_off))
    assert calls == {'fwd': 1, 'bwd': 1}
    assert torch.equal(y_on, y_off)


def test_funit_res_discriminator_on_equals_off(monkeypatch):
    from imaginaire_amd.discriminators.funit import ResDiscriminator
    from imaginaire_amd.ops import _ext, pool as P
    calls = _count_pads(monkeypatch, _ext.ext())
    torch.manual_seed(14)
    net = ResDiscriminator(num_layers=3, num_filters=8, num_classes=4).cuda()
    images = torch.randn(2, 3, 32, 32, device='cuda')
    labels = torch.tensor([1, 3], device='cuda')
    out, n = {}, {}
    for fused in (True, False):
        monkeypatch.setattr(P, '_FUSED_PAD', fused)
        calls['fwd'] = 0
        with torch.no_grad():
            out[fused] = net(images, labels)
        n[fused] = calls['fwd']
    assert torch.equal(out[True][0], out[False][0])  # logits
    assert torch.equal(out[True][1], out[False][1])  # features
    assert n[False] - n[True] == 2, n  # one padded copy per downsample
