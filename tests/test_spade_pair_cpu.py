"""The paired SPADE norms and the γ|β conv bias-gradient hand-over, without a GPU.

Off the HIP path ``fused_norm_act_pair`` is the nearest upsampling followed by two ordinary
``fused_norm_act`` calls, and a residual block called with ``pre_upsample`` upsamples its input
itself: both must reproduce the block's earlier forward / backward exactly. The holder logic
(``BiasGradHolder``, ``ops.conv._held_bias_grad``) is plain Python and is tested with the k2
bias pass stubbed out.
"""
import copy
import types

import torch

from imaginaire_amd.layers import Res2dBlock
from imaginaire_amd.ops import conv as nhwc_conv
from imaginaire_amd.ops.norm import BiasGradHolder, _NormCfg, fused_norm_act, fused_norm_act_pair
from imaginaire_amd.ops.resize import interpolate


def _block(cin, cout, norm='batch'):
    params = types.SimpleNamespace(
        num_filters=8, kernel_size=3, cond_dims=5, separate_projection=True,
        activation_norm_type=norm, weight_norm_type='')
    torch.manual_seed(3)
    return Res2dBlock(cin, cout, kernel_size=3, padding=1, bias=[True, True, False],
                      weight_norm_type='', activation_norm_type='spatially_adaptive',
                      activation_norm_params=params, skip_activation_norm=True,
                      nonlinearity='leakyrelu', order='NACNAC')


def _grads(mod):
    return [None if p.grad is None else p.grad.clone() for p in mod.parameters()]


def test_pre_upsample_equals_upsample_then_block():
    """``block(x, seg, pre_upsample=2)`` against ``block(upsample(x), seg)``: outputs, every
    gradient and the running statistics, bit for bit (learned and identity shortcut)."""
    for cin, cout in ((16, 8), (8, 8)):
        old, new = _block(cin, cout), None
        new = copy.deepcopy(old)
        torch.manual_seed(5)
        x = torch.randn(2, cin, 3, 5)
        seg = torch.randn(2, 5, 12, 20)
        go = torch.randn(2, cout, 6, 10)
        xo = x.clone().requires_grad_(True)
        yo = old(interpolate(xo, scale_factor=2.0, mode='nearest'), seg)
        yo.backward(go)
        xn = x.clone().requires_grad_(True)
        yn = new(xn, seg, pre_upsample=2)
        yn.backward(go)
        assert yo.shape == (2, cout, 6, 10)
        assert torch.equal(yo, yn)
        assert torch.equal(xo.grad, xn.grad)
        for a, b in zip(_grads(old), _grads(new)):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        for (k, a), b in zip(old.state_dict().items(), new.state_dict().values()):
            assert torch.equal(a, b), k


def test_pair_reference_is_upsample_and_two_norms():
    torch.manual_seed(7)
    N, C, h, w = 2, 8, 3, 5
    for up in (1, 2):
        x = torch.randn(N, C, h, w)
        gb0 = torch.randn(N, 2 * C, h * up, w * up) * 0.3
        gbs = torch.randn(N, 2 * C, h * up, w * up) * 0.3
        go0 = torch.randn(N, C, h * up, w * up)
        gos = torch.randn(N, C, h * up, w * up)
        runs = []
        for pair in (True, False):
            leaves = [t.clone().requires_grad_(True) for t in (x, gb0, gbs)]
            rm = [torch.zeros(C), torch.zeros(C)]
            rv = [torch.ones(C), torch.ones(C)]
            nb = [torch.tensor(0), torch.tensor(0)]
            if pair:
                cfg = _NormCfg('batch', True, 0.1, 1e-5, 1.0, None)
                y0, ys = fused_norm_act_pair(
                    leaves[0], up, leaves[1], leaves[2], (0.2, 1.0), cfg,
                    running=tuple((rm[i], rv[i], nb[i]) for i in range(2)))
            else:
                xu = interpolate(leaves[0], scale_factor=float(up), mode='nearest') \
                    if up != 1 else leaves[0]
                y0 = fused_norm_act(xu, 'batch', gb=leaves[1], running_mean=rm[0],
                                    running_var=rv[0], momentum=0.1, slope=0.2,
                                    num_batches=nb[0])
                ys = fused_norm_act(xu, 'batch', gb=leaves[2], running_mean=rm[1],
                                    running_var=rv[1], momentum=0.1, slope=1.0,
                                    num_batches=nb[1])
            torch.autograd.backward([y0, ys], [go0, gos])
            runs.append([y0, ys] + [t.grad for t in leaves] + rm + rv + nb)
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        assert int(runs[0][-1]) == 1


def test_generator_runs_with_pre_upsample(tmp_path):
    """The unit-test SPADE generator builds and runs; its 'a' blocks get the map before its
    upsampling and give the sizes they gave."""
    import os
    from imaginaire_amd.config import Config
    from imaginaire_amd.generators.spade import Generator
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config(os.path.join(root, 'configs', 'unit_test', 'spade.yaml'))
    torch.manual_seed(0)
    net = Generator(cfg.gen, cfg.data)
    seen = []
    g = net.spade_generator
    for name in ('up_0a', 'up_1a', 'up_2a'):
        getattr(g, name).register_forward_hook(
            lambda m, args, kwargs, out, name=name: seen.append(
                (name, tuple(args[0].shape[2:]), kwargs.get('pre_upsample'),
                 tuple(out.shape[2:]))), with_kwargs=True)
    data = {'label': torch.randn(1, 14, 256, 256), 'images': torch.randn(1, 3, 256, 256)}
    out = net(data)
    assert out['fake_images'].shape == (1, 3, 256, 256)
    assert torch.isfinite(out['fake_images']).all()
    assert seen == [('up_0a', (16, 16), 2, (32, 32)), ('up_1a', (32, 32), 2, (64, 64)),
                    ('up_2a', (64, 64), 2, (128, 128))]


def test_holder_hand_over_and_fallback(monkeypatch):
    calls = []

    def fake_bias_grad(t):
        calls.append(t)
        return t.float().sum((0, 2, 3))

    monkeypatch.setattr(nhwc_conv, '_bias_grad', fake_bias_grad)
    dy = torch.randn(2, 6, 3, 4)
    sums = torch.arange(6.0)
    used0 = BiasGradHolder.used

    h = BiasGradHolder()
    h.fill(sums, dy)
    assert nhwc_conv._held_bias_grad(h, dy, dy) is sums and not calls
    assert BiasGradHolder.used == used0 + 1
    # taken once: the holder is empty afterwards, the conv sums itself
    assert torch.equal(nhwc_conv._held_bias_grad(h, dy, dy), dy.sum((0, 2, 3)))
    assert len(calls) == 1

    # no holder, an empty one, another tensor, a tensor changed since, another channel count
    for holder, arg in ((None, dy), (BiasGradHolder(), dy)):
        assert torch.equal(nhwc_conv._held_bias_grad(holder, arg, arg), arg.sum((0, 2, 3)))
    h.fill(sums, dy)
    other = dy.clone()
    assert torch.equal(nhwc_conv._held_bias_grad(h, other, other), other.sum((0, 2, 3)))
    h.fill(sums, dy)
    dy.add_(1.0)
    assert torch.equal(nhwc_conv._held_bias_grad(h, dy, dy), dy.sum((0, 2, 3)))
    h.fill(sums[:4], dy)
    assert torch.equal(nhwc_conv._held_bias_grad(h, dy, dy), dy.sum((0, 2, 3)))
    assert len(calls) == 6 and BiasGradHolder.used == used0 + 1


def test_conv2d_ignores_the_holder_off_the_k10_route():
    """On the CPU no k10 Function runs: the holder stays untouched and nothing is left behind
    for a later conv to pick up."""
    h = BiasGradHolder()
    x = torch.randn(1, 4, 5, 5)
    w = torch.randn(6, 4, 3, 3, requires_grad=True)
    b = torch.zeros(6, requires_grad=True)
    y = nhwc_conv.conv2d(x, w, b, 1, 1, bias_grad=h)
    y.sum().backward()
    assert h.db is None and nhwc_conv._HELD_BIAS_GRAD.holder is None
    assert torch.allclose(b.grad, torch.full((6,), 25.0))
