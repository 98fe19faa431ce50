"""k11 weight gradient: the restaged (LDS, 16-byte row stores) epilogue and the finished output
of a single slab, against the dword epilogue + slab + wgrad_finalize path of the same build
(IMAGINAIRE_AMD_WGRAD_EPILOGUE=0) bit for bit, and against PyTorch's fp32 weight gradient.
Every case runs with the switch at 0, unset (the default: restaged where the kernel finishes dW)
and 1 (restaged everywhere)."""
import contextlib
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# name: (Cin, H, W, Cout, k, stride, pad, variant, kernel id of wgrad_last_kernel)
SHAPES = {
    # one-tap generic (Wo % 64 != 0)
    'gen_3x3_64': (64, 12, 20, 64, 3, 1, 1, 1, 0),
    'gen_1x1_128': (64, 12, 20, 128, 1, 1, 0, 1, 0),
    'gen_3x3_128x128': (128, 12, 20, 128, 3, 1, 1, 1, 0),   # 64 KB tile = the whole ring
    # one-tap ROWS (Wo = 64)
    'rows_4x4s2_128': (128, 8, 128, 128, 4, 2, 1, 1, 1),
    # multi-tap
    'mt_3x3_128x64': (64, 4, 64, 128, 3, 1, 1, 1, 2),
    'mt_3x3_64x64': (64, 4, 64, 64, 3, 1, 1, 1, 2),
    'mt_5x5_64': (64, 4, 64, 64, 5, 1, 2, 1, 2),
    'mt_7x7_64': (64, 4, 64, 64, 7, 1, 3, 1, 2),
    # v2 (variant 2)
    'v2_3x3_bc128_seg64': (128, 4, 64, 128, 3, 1, 1, 2, 3),
    'v2_3x3_bc128_seg32': (128, 8, 32, 128, 3, 1, 1, 2, 3),
    'v2_3x3_bc128_seg16': (128, 16, 16, 128, 3, 1, 1, 2, 3),
    'v2_3x3_bc64': (64, 4, 64, 128, 3, 1, 1, 2, 3),
    'v2_5x5': (128, 4, 64, 128, 5, 1, 2, 2, 3),
}
# name: (out_cout, out_cin, out_bf16, sn elements, sentinel elements around dst or None,
#        finished by the k11 kernel itself at S == 1 unless the switch is 0)
VARIANTS = {
    'fp32': (-1, -1, False, 0, None, True),   # (the uncropped fp32 slab is dW: direct before too)
    'dst': (-1, -1, False, 0, 64, True),
    'bf16': (-1, -1, True, 0, None, True),
    'bf16_crop40x36': (40, 36, True, 0, None, True),
    'bf16_dst2': (-1, -1, True, 0, 2, True),   # base 4-byte aligned: scalar bf16 stores
    'crop40x36': (40, 36, False, 0, None, True),       # 4-element stores
    'crop40x36_dst': (40, 36, False, 0, 64, True),
    'crop40x36_dst2': (40, 36, False, 0, 2, True),     # base 8-byte aligned: scalar stores
    'crop_cin3': (-1, 3, False, 0, None, True),        # out_cin 3: scalar stores
    'sn5': (-1, -1, False, 5, None, True),    # <G, W> given as 512 partials
    'sn5_dst': (-1, -1, False, 5, 64, True),
    'sn4': (-1, -1, False, 4, None, False),   # <G, W> from this launch's epilogue: two passes
}
PAD_MODE_CASES = [('mt_3x3_128x64', 'crop40x36'), ('mt_3x3_128x64', 'sn5'),
                  ('v2_3x3_bc128_seg32', 'bf16'), ('v2_3x3_bc128_seg32', 'sn5')]
SENTINEL = -12288.0  # (exact in bf16 too)


@contextlib.contextmanager
def _switch(value):
    old = os.environ.get('IMAGINAIRE_AMD_WGRAD_EPILOGUE')
    if value is None:
        os.environ.pop('IMAGINAIRE_AMD_WGRAD_EPILOGUE', None)
    else:
        os.environ['IMAGINAIRE_AMD_WGRAD_EPILOGUE'] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('IMAGINAIRE_AMD_WGRAD_EPILOGUE', None)
        else:
            os.environ['IMAGINAIRE_AMD_WGRAD_EPILOGUE'] = old


@functools.lru_cache(maxsize=None)
def _operands(shape, B, pad_mode):
    """dy, x (bf16, channels-last) and PyTorch's fp32 weight gradient of them (computed once per
    shape and shared; nothing writes to them)."""
    cin, H, W, cout, k, s, p, _, _ = SHAPES[shape]
    g = torch.Generator(device='cuda').manual_seed(1234)
    x = torch.randn(B, cin, H, W, device='cuda', generator=g).to(torch.bfloat16).contiguous(
        memory_format=CL)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(B, cout, Ho, Wo, device='cuda', generator=g).to(torch.bfloat16).contiguous(
        memory_format=CL)
    if pad_mode:
        xp = torch.nn.functional.pad(x.float(), (p, p, p, p), mode='reflect')
        ref = torch.nn.grad.conv2d_weight(xp, (cout, cin, k, k), dy.float(), s, 0)
    else:
        ref = torch.nn.grad.conv2d_weight(x.float(), (cout, cin, k, k), dy.float(), s, p)
    return dy, x, ref


def _call_args(shape, variant, dy, x, pad_mode):
    """(positional arguments after dy, x; the dst buffer or None; (rows, columns, k, guard) of
    the output; a function mapping the fp32 gradient G to the expected output)"""
    cin, H, W, cout, k, s, p, var, _ = SHAPES[shape]
    oc, oi, bf16, nsn, guard, _ = VARIANTS[variant]
    sn, buf = None, None
    roc, roi = (cout if oc < 0 else oc), (cin if oi < 0 else oi)
    expect = lambda G: G[:roc, :roi]  # noqa: E731
    if nsn:
        g = torch.Generator(device='cuda').manual_seed(99)
        shadow = (torch.randn(cout, cin, k, k, device='cuda', generator=g) / (cin * k * k) ** 0.5
                  ).to(torch.bfloat16).contiguous(memory_format=CL)
        u = torch.nn.functional.normalize(torch.randn(cout, device='cuda', generator=g), dim=0)
        v = torch.nn.functional.normalize(torch.randn(cin * k * k, device='cuda', generator=g),
                                          dim=0)
        sigma = torch.tensor([1.7], device='cuda')
        sn = [shadow, u, v, sigma]
        if nsn == 5:
            parts = torch.randn(512, device='cuda', generator=g) * 0.05
            sn.append(parts)

        def expect(G):  # noqa: E306
            dot = sn[4].double().sum() if len(sn) == 5 else (G.double() * shadow.double()).sum()
            uv = u.double()[:, None, None, None] * v.double().view(cin, k, k)[None]
            return (G.double() / 1.7 - dot / 1.7 ** 2 * uv).float()
    if guard is not None:
        n = roc * roi * k * k
        buf = torch.full((n + 2 * guard,), SENTINEL, device='cuda',
                         dtype=torch.bfloat16 if bf16 else torch.float32)
    args = (k, k, s, s, p, p, 1, 1, oc, oi, bf16, 1, var, sn)
    return args, buf, (roc, roi, k, guard), expect


def _dst_of(buf, dims):
    if buf is None:
        return None
    roc, roi, k, guard = dims
    return buf.as_strided((roc, roi, k, k), (k * k * roi, 1, k * roi, roi), guard)


def _run(ext, shape, variant, B, pad_mode, switch):
    dy, x, _ = _operands(shape, B, pad_mode)
    args, buf, dims, _ = _call_args(shape, variant, dy, x, pad_mode)
    with _switch(switch):
        plan = ext.conv2d_wgrad_plan(dy, x, *args, _dst_of(buf, dims), pad_mode)
        out = ext.conv2d_wgrad_mfma(dy, x, *args, _dst_of(buf, dims), pad_mode)
        assert ext.wgrad_last_kernel() == plan['kernel']
    return out, buf, plan


def _check(shape, variant, B, pad_mode=0):
    from imaginaire_amd.ops import _ext
    ext = _ext.ext()
    dy, x, ref = _operands(shape, B, pad_mode)
    args, _, dims, expect = _call_args(shape, variant, dy, x, pad_mode)
    bf16 = VARIANTS[variant][2]
    old, old_buf, old_plan = _run(ext, shape, variant, B, pad_mode, '0')
    new, new_buf, plan = _run(ext, shape, variant, B, pad_mode, None)
    # restaged everywhere (the default restages only what it finishes)
    allr, allr_buf, allr_plan = _run(ext, shape, variant, B, pad_mode, '1')
    # the path the shape is named for
    assert plan['kernel'] == old_plan['kernel'] == SHAPES[shape][8]
    assert plan['S'] == old_plan['S'] and plan['tiles'] == old_plan['tiles']
    assert (plan['S'] == 1) == (B == 1), plan
    finished = B == 1 and VARIANTS[variant][5]
    direct = B == 1 and variant in ('fp32', 'dst')
    assert old_plan['epilogue'] == 'dword' and allr_plan['epilogue'] == 'restaged'
    assert plan['epilogue'] == ('restaged' if finished and not direct else 'dword'), plan
    assert plan['finished_in_kernel'] == allr_plan['finished_in_kernel'] == finished, plan
    assert allr_plan['S'] == plan['S'] and allr_plan['kernel'] == plan['kernel']
    assert old_plan['finished_in_kernel'] == (B == 1 and variant in ('fp32', 'dst')), old_plan
    # bitwise against the old path
    assert new.dtype == old.dtype and new.shape == old.shape
    assert new.is_contiguous(memory_format=CL)
    assert torch.equal(new, old)
    assert allr.dtype == old.dtype and torch.equal(allr, old)
    # against fp32: the bound tests/test_kernels_gpu.py applies to k11 (2e-3 of the largest
    # reference value). A bf16 output is the fp32 result of the same call cast to bf16: that fp32
    # result takes the bound, and the bf16 output must equal its cast exactly.
    f32 = new
    if bf16:
        with _switch('0'):
            f32 = ext.conv2d_wgrad_mfma(dy, x, *args[:10], False, *args[11:], None, pad_mode)
        assert f32.dtype == torch.float32 and new.dtype == torch.bfloat16
        assert torch.equal(new, f32.to(torch.bfloat16))
    assert f32.dtype == torch.float32
    want = expect(ref)
    scale = max(1.0, want.abs().max().item())
    err = (f32 - want).abs().max().item()
    bound = 2e-3 * scale
    print('%s %s B=%d pad_mode=%d: err %.3e bound %.3e' % (shape, variant, B, pad_mode, err,
                                                           bound))
    assert err <= bound
    # no write outside dst
    for buf, out in ((old_buf, old), (new_buf, new), (allr_buf, allr)):
        if buf is not None:
            roc, roi, k, guard = dims
            assert torch.all(buf[:guard] == SENTINEL) and torch.all(buf[-guard:] == SENTINEL)
            assert torch.equal(buf[guard:-guard].view(roc, k, k, roi).permute(0, 3, 1, 2), out)
            assert torch.equal(out, old)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_single_slab(shape, variant):
    """Batch 1 (S == 1): every case but the 4-element sn is finished by the k11 kernel."""
    _check(shape, variant, 1)


@pytest.mark.parametrize('variant', ['fp32', 'crop40x36_dst', 'crop40x36_dst2', 'bf16', 'bf16_dst2', 'sn5', 'sn4'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_split_k(shape, variant):
    """Batch 8 (S > 1): slabs (dword epilogue; restaged with the switch at 1), summed by
    wgrad_finalize."""
    _check(shape, variant, 8)


@pytest.mark.parametrize('shape,variant', PAD_MODE_CASES)
def test_reflect_padding(shape, variant):
    _check(shape, variant, 1, pad_mode=1)


def test_switch_read_per_call():
    """The switch is read on every call, not once per process."""
    from imaginaire_amd.ops import _ext
    ext = _ext.ext()
    seen = [_run(ext, 'mt_3x3_64x64', 'bf16', 1, 0, sw)[2]['epilogue']
            for sw in ('0', None, '0', '1')]
    assert seen == ['dword', 'restaged', 'dword', 'restaged']
    with _switch('2'), pytest.raises(RuntimeError, match='must be 0 or 1'):
        ext.conv2d_wgrad_plan(*_operands('mt_3x3_64x64', 1, 0)[:2], 3, 3, 1, 1, 1, 1, 1, 1)
