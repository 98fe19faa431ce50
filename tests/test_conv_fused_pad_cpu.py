"""CPU side of the fused reflect / replicate padding (``ops/conv.py`` ``_FUSED_PAD``): tensors
that never reach the HIP loaders still go through pad-then-conv, and the switch parses its
environment variable."""
import importlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('mode', ['reflect', 'replicate', 'circular'])
@pytest.mark.parametrize('stride,k,p', [(1, 3, 1), (2, 4, 1), (1, 7, 3)])
def test_cpu_conv2d_matches_padded_reference(mode, stride, k, p):
    from imaginaire_amd.ops import conv as C
    torch.manual_seed(3)
    x = torch.randn(2, 8, 9, 11, requires_grad=True)
    w = torch.randn(24, 8, k, k, requires_grad=True)
    b = torch.randn(24)
    y = C.conv2d(x, w, b, stride, p, 1, 1, mode)
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    ref = F.conv2d(F.pad(xr, (p, p, p, p), mode=mode), wr, b, stride)
    assert torch.allclose(y, ref, atol=1e-5, rtol=1e-5)
    r = torch.randn_like(ref)
    yr = C.conv2d(x, w, b, stride, p, 1, 1, mode, residual=r)
    assert torch.allclose(yr, ref + r, atol=1e-5, rtol=1e-5)
    g = torch.randn_like(ref)
    y.backward(g)
    ref.backward(g)
    assert torch.allclose(x.grad, xr.grad, atol=1e-4, rtol=1e-4)
    assert torch.allclose(w.grad, wr.grad, atol=1e-4, rtol=1e-4)


def test_fused_pad_mode_is_zero_off_the_gpu():
    from imaginaire_amd.ops import conv as C
    x, w = torch.randn(1, 64, 8, 8), torch.randn(64, 64, 3, 3)
    assert C._route(x, w, (1, 1), (1, 1), (1, 1), 1, 'reflect').pmode == 0


@pytest.mark.parametrize('value,expect', [(None, True), ('0', False)])
def test_switch_parses_environment(value, expect):
    env = dict(os.environ)
    env.pop('IMAGINAIRE_AMD_CONV_FUSED_PAD', None)
    if value is not None:
        env['IMAGINAIRE_AMD_CONV_FUSED_PAD'] = value
    out = subprocess.run(
        [sys.executable, '-c',
         'from imaginaire_amd.ops import conv; print(conv._FUSED_PAD)'],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == str(expect)


def test_switch_default_in_process():
    from imaginaire_amd.ops import conv as C
    if 'IMAGINAIRE_AMD_CONV_FUSED_PAD' not in os.environ:
        assert importlib.import_module('imaginaire_amd.ops.conv')._FUSED_PAD is True
    assert C._FUSED_PAD_MODES == {'reflect': 1, 'replicate': 2}
