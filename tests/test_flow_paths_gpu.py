"""The optical-flow kernels on every host route: k6 cost volume and k8 channel norm
(``csrc/correlation.hip``), k7 Resample2d and k9 flow warp (``csrc/flow_warp.hip``).

Every k6 case first asserts, through the extension's read-only ``correlation_plan``, that its
shape, dtype and environment still reach the forward and backward kernel it is named for (all
four forward kernels, both ``S2`` instantiations of the two MFMA kernels, all three backward
kernels, the dynamic-LDS bytes where a gate is meant), then compares forward and both gradients
with a float64 oracle. The H*W*C >= 2^31 gate of the MFMA forward is not tested: it needs 4 GB
inputs.

Oracles. They are written here from the formulas, in float64, on the inputs rounded to the dtype
the kernel receives (``_leaf64``); gradients are float64 autograd, except the warp's flow
gradient, which is the tap-difference formula masked by grid_sample's border rule (zero where
the sample position s <= 0 or s >= size - 1). The one thing the warps' oracles take in fp32 is
the sample position s = float32(x) + float32(flow): that is the ops' definition (grid_sample
works in fp32 too), and floor / clamp of the same fp32 number give the same taps as the kernel.

Tolerance. One rule, applied to every element (no share of elements is let off):

    |got - ref| <= u |ref| + n 2^-24 S

  * ref is the float64 result for the very inputs the kernel read, so the kernel's error is the
    rounding of its result plus the rounding of its fp32 arithmetic.
  * u |ref|: the result's rounding. u = 2^-8 for a bf16 result: bf16 keeps 8 significant bits,
    so one rounding to nearest moves a value by at most 2^-8 of it, and every bf16 result here
    is rounded exactly once from an fp32 value (outputs by the kernel, gradients by the
    wrapper). u = 2^-21 for an fp32 result (a few ulp for 1/C, sqrtf and the products of the
    tap weights).
  * n 2^-24 S: the kernel forms the element as a sum of n products in fp32. Summing n terms
    t_i in ANY order, each partial sum rounded to nearest (relative error <= 2^-24), is off by at
    most (n - 1) 2^-24 sum |t_i| to first order; S = sum |t_i|. The order does not enter, so the
    bound holds for the LDS-tiled loops, for float atomics and for MFMA alike (a bf16 x bf16
    product is exact in fp32). n counts the terms of that element plus 4 for the arithmetic
    that makes the weights ((1 - wx)(1 - wy), 1 / C, ...).
  * S is the same oracle evaluated on |inputs| (and |grad_out|): every term of the sum becomes
    its absolute value. For k8, sqrt(sum x^2) of |x| is the norm itself, and a relative error e
    of the sum is e / 2 of its root. For the warps' flow gradients the terms are differences of
    taps, g_c (v01 - v00)(1 - wy) ...; their absolute sum is at most
    4 * window * sum_c |g_c| * max |img|, which is used as S (window = kernel_size^2 for k7).
  * term counts: k6 forward kernel_size^2 C, k6 gradients D^2 kernel_size^2; k9 / k7 output 4
    taps per window position, their image gradient the number of taps that land on the pixel
    (counted by the oracle), their flow gradient 4 taps per channel and window position; k8
    C terms.

Each check prints ``err/bound <kernel> <result dtype> <what> <max ratio>``. A bf16 result sits
near ratio 1 by construction (the rounding of a value just above a power of two is the whole of
u |ref|); an fp32 result shows how much of the worst-case summation bound the kernel uses.

GPU tests carry ``@gpu``; ``tests/test_flow_oracles_cpu.py`` checks the oracles themselves
without a GPU.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
BF16, FP32 = torch.bfloat16, torch.float32
_U = {BF16: 2.0 ** -8, FP32: 2.0 ** -21}
_EPS = 2.0 ** -24
_NAME = {BF16: 'bf16', FP32: 'fp32'}


def _leaf64(t, dtype=None):
    """float64 leaf of ``t`` as the kernel sees it (rounded to ``dtype`` first)."""
    t = t.detach()
    if dtype is not None:
        t = t.to(dtype)
    return t.double().requires_grad_(True)


def _check(got, ref, n, S, kernel, what):
    """The module's tolerance rule on every element; prints the largest err / bound."""
    assert got.shape == ref.shape, (kernel, what, got.shape, ref.shape)
    got64, ref = got.detach().double(), ref.detach()
    assert bool(torch.isfinite(got64).all()), '%s %s: not finite' % (kernel, what)
    err = (got64 - ref).abs()
    bound = _U[got.dtype] * ref.abs() + n * _EPS * S
    worst = float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())
    print('err/bound %s %s %s %.4f' % (kernel, _NAME[got.dtype], what, worst))
    bad = err > bound
    assert not bool(bad.any()), '%s %s: %d of %d beyond the bound, max err/bound %.3f' % (
        kernel, what, int(bad.sum()), bad.numel(), worst)


# ---- k6: cost volume ----------------------------------------------------------------------
def _corr_out_size(size, pad, ks, md, s1):
    return -(-(size + 2 * pad - 2 * ((ks - 1) // 2 + md)) // s1)


def _corr_ref64(a, b, pad, ks, md, s1, s2):
    """out[n, (tj+R) D + ti+R, oy, ox] = 1 / (ks^2 C) * sum over the ks^2 window and C of
    A[y1 + j, x1 + i] * B[y1 + j + tj s2, x1 + i + ti s2], (y1, x1) = (oy, ox) s1 + md in the
    frame zero-padded by ``pad``; whatever lies outside that frame is zero as well."""
    n, c, h, w = a.shape
    kr, R = (ks - 1) // 2, md // s2
    oh, ow = _corr_out_size(h, pad, ks, md, s1), _corr_out_size(w, pad, ks, md, s1)
    m = pad + kr + R * s2 + 1  # no tap leaves a buffer padded this far
    ap, bp = F.pad(a, [m] * 4), F.pad(b, [m] * 4)
    y0, x0 = md + m - pad, md + m - pad  # buffer index of padded-frame centre (oy, ox) = (0, 0)

    def win(t, y, x):
        return t[:, :, y:y + (oh - 1) * s1 + 1:s1, x:x + (ow - 1) * s1 + 1:s1]
    outs = []
    for tj in range(-R, R + 1):
        for ti in range(-R, R + 1):
            acc = 0.
            for j in range(-kr, kr + 1):
                for i in range(-kr, kr + 1):
                    acc = acc + (win(ap, y0 + j, x0 + i) *
                                 win(bp, y0 + j + tj * s2, x0 + i + ti * s2)).sum(1)
            outs.append(acc)
    return torch.stack(outs, 1) / (ks * ks * c)


# (id, dtype, N, C, H, W, (pad, ks, md, s1, s2), fwd, S2 template, bwd, bwd LDS bytes or None)
_K6_ROWS = [
    ('band33-s1', BF16, 2, 64, 7, 37, (16, 1, 16, 1, 1), 'mfma_diag', 1, 'k1', None),
    ('band33-s2', BF16, 2, 64, 7, 37, (32, 1, 32, 1, 2), 'mfma_diag', 2, 'k1', 66048),
    ('d35', BF16, 2, 64, 7, 37, (17, 1, 17, 1, 1), 'generic', 0, 'k1', None),
    ('md-odd', BF16, 2, 32, 5, 19, (3, 1, 3, 1, 2), 'mfma_diag', 2, 'elem', None),
    ('pad-lt-md', BF16, 2, 64, 9, 21, (2, 1, 4, 1, 1), 'mfma_diag', 1, 'k1', None),
    ('pad-gt-md', BF16, 2, 64, 9, 21, (6, 1, 4, 1, 2), 'mfma_diag', 2, 'k1', None),
    ('c352', BF16, 2, 352, 5, 20, (4, 1, 4, 1, 2), 'mfma', 2, 'elem', None),
    ('c704', BF16, 2, 704, 5, 20, (4, 1, 4, 1, 1), 'mfma', 1, 'k1', None),
    ('flownetc', BF16, 2, 128, 6, 100, (20, 1, 20, 1, 2), 'mfma_diag', 2, 'k1', None),
    ('pixel', BF16, 2, 64, 1, 1, (4, 1, 4, 1, 2), 'mfma_diag', 2, 'k1', None),
    ('f-pad-lt-md', FP32, 2, 64, 9, 21, (2, 1, 4, 1, 1), 'k1', 0, 'k1', None),
    ('f-tail', FP32, 2, 40, 9, 21, (6, 1, 4, 1, 2), 'k1', 0, 'elem', None),
    ('f-s1-2', FP32, 2, 33, 9, 40, (4, 1, 4, 2, 1), 'k1', 0, 'elem', None),
    ('f-d25', FP32, 2, 64, 5, 40, (12, 1, 12, 1, 1), 'generic', 0, 'k1', None),
    ('f-lds82k', FP32, 1, 64, 5, 40, (32, 1, 32, 1, 1), 'generic', 0, 'k1', 82432),
    ('f-lds-gate', FP32, 1, 64, 3, 40, (40, 1, 40, 1, 1), 'generic', 0, 'elem', None),
    ('f-ks3', FP32, 2, 7, 9, 11, (4, 3, 3, 2, 2), 'generic', 0, 'elem', None),
    ('f-pad0-ks3', FP32, 2, 3, 6, 8, (0, 3, 1, 1, 1), 'generic', 0, 'elem', None),
    ('f-pixel', FP32, 2, 64, 1, 1, (4, 1, 4, 1, 1), 'k1', 0, 'k1', None),
]
_K6_BY_ID = {r[0]: r for r in _K6_ROWS}
_K6_SIZES = {'pad-lt-md': (5, 17), 'pad-gt-md': (13, 25), 'f-s1-2': (5, 20), 'f-lds-gate': (3, 40)}
_K6_ENV = ('IMAGINAIRE_AMD_CORR_MFMA', 'IMAGINAIRE_AMD_CORR_DIAG', 'IMAGINAIRE_AMD_CORR_BWD_TILED')
# (row id, environment, fwd, bwd, bwd LDS bytes or None)
_K6_EXTRA = [
    ('band33-s1', {'IMAGINAIRE_AMD_CORR_DIAG': '0'}, 'mfma', 'k1', None),
    ('band33-s2', {'IMAGINAIRE_AMD_CORR_DIAG': '0'}, 'mfma', 'k1', 66048),
    ('pad-lt-md', {'IMAGINAIRE_AMD_CORR_DIAG': '0'}, 'mfma', 'k1', None),
    ('pad-gt-md', {'IMAGINAIRE_AMD_CORR_DIAG': '0'}, 'mfma', 'k1', None),
    ('pad-lt-md', {'IMAGINAIRE_AMD_CORR_MFMA': '0'}, 'k1', 'k1', None),
    ('band33-s1', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'mfma_diag', 'k1r', 62336),
    # the 64 KB gate of the register-blocked kernel refuses this one
    ('band33-s2', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'mfma_diag', 'k1', 66048),
    ('d35', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'generic', 'k1r', 64928),
    ('pad-lt-md', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'mfma_diag', 'k1r', 33824),
    ('pad-gt-md', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'mfma_diag', 'k1r', 30624),
    ('c704', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'mfma', 'k1r', 33824),
    ('flownetc', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'mfma_diag', 'k1r', 54304),
    ('pixel', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '2'}, 'mfma_diag', 'k1r', 30624),
    ('pad-lt-md', {'IMAGINAIRE_AMD_CORR_BWD_TILED': '0'}, 'mfma_diag', 'elem', None),
]


@functools.lru_cache(maxsize=None)
def _k6_case(row_id, dtype_b=None):
    """Inputs, float64 reference and the |.| sums S of one row, made once and left unchanged:
    the environment variants of a row share them."""
    _, dtype, N, C, H, W, params, _, _, _, _ = _K6_BY_ID[row_id]
    g = torch.Generator().manual_seed(1000 + [r[0] for r in _K6_ROWS].index(row_id))
    a = torch.randn(N, C, H, W, generator=g).cuda().to(dtype).contiguous(
        memory_format=torch.channels_last)
    b = torch.randn(N, C, H, W, generator=g).cuda().to(dtype_b or dtype)
    ar, br = _leaf64(a), _leaf64(b, dtype)  # the wrapper casts input2 to input1's dtype
    ref = _corr_ref64(ar, br, *params)
    go = torch.randn(ref.shape, generator=g).cuda().to(dtype)
    ga, gb = torch.autograd.grad(ref, (ar, br), go.double())
    aa, ba = _leaf64(a.abs()), _leaf64(b.abs(), dtype)
    s_out = _corr_ref64(aa, ba, *params)
    s_a, s_b = torch.autograd.grad(s_out, (aa, ba), go.double().abs())
    return dict(a=a, b=b, go=go, ref=ref.detach(), ga=ga, gb=gb, s_out=s_out.detach(), s_a=s_a,
                s_b=s_b)


def _k6_run(row_id, fwd, bwd, bwd_lds, dtype_b=None):
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.ops.flownet_ops import _CorrelationFn
    _, dtype, N, C, H, W, params, _, s2t, _, _ = _K6_BY_ID[row_id]
    pad, ks, md, s1, s2 = params
    case = _k6_case(row_id, dtype_b)
    a = case['a'].clone(memory_format=torch.preserve_format).requires_grad_(True)
    b = case['b'].clone().requires_grad_(True)
    p = dict(_ext.ext().correlation_plan(a, *params))
    D = 2 * (md // s2) + 1
    assert (p['fwd'], p['bwd']) == (fwd, bwd), p
    assert p['s2_template'] == (s2t if fwd.startswith('mfma') else 0), p
    assert p['D'] == D and (p['oH'], p['oW']) == tuple(case['ref'].shape[2:]), p
    if row_id in _K6_SIZES:
        assert (p['oH'], p['oW']) == _K6_SIZES[row_id]
    if bwd_lds is not None:
        assert p['bwd_lds'] == bwd_lds, p
    assert (p['bwd_lds'] == 0) == (bwd == 'elem') and (p['fwd_lds'] == 0) == (
        fwd in ('mfma', 'generic')), p
    out = _CorrelationFn.apply(a, b, *params)
    assert out.dtype == dtype and out.is_contiguous(memory_format=torch.channels_last)
    ga, gb = torch.autograd.grad(out, (a, b), case['go'])
    assert ga.dtype == a.dtype and gb.dtype == b.dtype
    kf = 'corr_fwd_%s' % fwd + ('<%d>' % p['s2_template'] if p['s2_template'] else '')
    kb = {'k1r': 'corr_bwd_k1r', 'k1': 'corr_bwd_k1', 'elem': 'corr_bwd'}[bwd]
    _check(out, case['ref'], ks * ks * C + 4, case['s_out'], kf, 'out')
    _check(ga, case['ga'], D * D * ks * ks + 4, case['s_a'], kb, 'd_input1')
    _check(gb, case['gb'], D * D * ks * ks + 4, case['s_b'], kb, 'd_input2')


def _k6_clean_env(monkeypatch, env=()):
    for name in _K6_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in dict(env).items():
        monkeypatch.setenv(name, value)  # the switches are read on every call


@gpu
@pytest.mark.parametrize('row_id', [r[0] for r in _K6_ROWS])
def test_correlation_routes(row_id, monkeypatch):
    _k6_clean_env(monkeypatch)
    row = _K6_BY_ID[row_id]
    _k6_run(row_id, row[7], row[9], row[10])


@gpu
@pytest.mark.parametrize('row_id,env,fwd,bwd,bwd_lds', [
    pytest.param(*e, id='%s-%s' % (e[0], '-'.join(
        '%s=%s' % (k.rsplit('_', 1)[-1], v) for k, v in e[1].items()))) for e in _K6_EXTRA])
def test_correlation_routes_env(row_id, env, fwd, bwd, bwd_lds, monkeypatch):
    _k6_clean_env(monkeypatch, env)
    _k6_run(row_id, fwd, bwd, bwd_lds)


@gpu
def test_correlation_second_input_fp32(monkeypatch):
    """input1 bf16, input2 fp32: the wrapper rounds input2 to bf16 and returns its gradient in
    fp32."""
    _k6_clean_env(monkeypatch)
    _k6_run('pad-lt-md', 'mfma_diag', 'k1', None, dtype_b=FP32)


# ---- k9 / k7: positions and taps ----------------------------------------------------------
def _pos32(flow, H, W):
    """Sample positions s = float32(x) + float32(flow), the ops' definition, as float64."""
    f = flow.detach().float()
    xs = torch.arange(W, device=f.device, dtype=FP32).view(1, 1, W)
    ys = torch.arange(H, device=f.device, dtype=FP32).view(1, H, 1)
    return (xs + f[:, 0]).double(), (ys + f[:, 1]).double()


def _gather(img, yy, xx):
    B, C, H, W = img.shape
    idx = (yy * W + xx).reshape(B, 1, H * W).expand(B, C, H * W)
    return img.reshape(B, C, H * W).gather(2, idx).reshape(B, C, H, W)


def _sample(img, taps):
    return sum(w[:, None] * _gather(img, yy, xx) for yy, xx, w in taps)


def _tap_count(taps, B, H, W):
    """How many taps (of any weight) land on each image pixel: [B, 1, H, W]."""
    cnt = torch.zeros(B, H * W, device=taps[0][0].device, dtype=torch.float64)
    for yy, xx, _ in taps:
        cnt.scatter_add_(1, (yy * W + xx).reshape(B, -1), torch.ones_like(cnt))
    return cnt.reshape(B, 1, H, W)


def _warp_taps(flow, H, W):
    """k9: clamp s to [0, size - 1], floor, x1 = min(x0 + 1, W - 1); four taps."""
    sx, sy = _pos32(flow, H, W)
    cx, cy = sx.clamp(0, W - 1), sy.clamp(0, H - 1)
    x0, y0 = cx.floor(), cy.floor()
    wx, wy = cx - x0, cy - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    taps = [(y0, x0, (1 - wx) * (1 - wy)), (y0, x1, wx * (1 - wy)),
            (y1, x0, (1 - wx) * wy), (y1, x1, wx * wy)]
    return taps, (sx, sy, wx, wy)


def _warp_ref64(img, flow):
    return _sample(img, _warp_taps(flow, img.shape[2], img.shape[3])[0])


def _warp_flow_grad64(img, flow, gout):
    """d(out)/d(flow) by the tap differences; zero where s <= 0 or s >= size - 1 (grid_sample's
    border rule)."""
    B, C, H, W = img.shape
    taps, (sx, sy, wx, wy) = _warp_taps(flow, H, W)
    v00, v01, v10, v11 = (_gather(img, yy, xx) for yy, xx, _ in taps)
    wx, wy = wx[:, None], wy[:, None]
    gx = (gout * ((v01 - v00) * (1 - wy) + (v11 - v10) * wy)).sum(1)
    gy = (gout * ((v10 - v00) * (1 - wx) + (v11 - v01) * wx)).sum(1)
    gx = torch.where((sx <= 0) | (sx >= W - 1), torch.zeros_like(gx), gx)
    gy = torch.where((sy <= 0) | (sy >= H - 1), torch.zeros_like(gy), gy)
    return torch.stack([gx, gy], 1)


def _resample_taps(flow, H, W, ks):
    """k7: alpha / beta from the unclamped position; corner indices clamped, window offsets
    added and clamped again. ``flow`` may be a float64 leaf: alpha and beta then carry its
    gradient (derivative 1) on top of the values of the fp32 position."""
    sx, sy = _pos32(flow, H, W)
    fl = flow.double()
    alpha = (sx - sx.floor()) + (fl[:, 0] - fl[:, 0].detach())
    beta = (sy - sy.floor()) + (fl[:, 1] - fl[:, 1].detach())
    x0, y0 = sx.floor().long(), sy.floor().long()
    xL, xR = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
    yT, yB = y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
    taps = []
    for fy in range(ks):
        for fx in range(ks):
            yt, yb = (yT + fy).clamp(0, H - 1), (yB + fy).clamp(0, H - 1)
            xl, xr = (xL + fx).clamp(0, W - 1), (xR + fx).clamp(0, W - 1)
            taps += [(yt, xl, (1 - alpha) * (1 - beta)), (yt, xr, alpha * (1 - beta)),
                     (yb, xl, (1 - alpha) * beta), (yb, xr, alpha * beta)]
    return taps


def _resample_ref64(img, flow, ks):
    return _sample(img, _resample_taps(flow, img.shape[2], img.shape[3], ks))


def _flows(kind, B, H, W, seed, device='cuda'):
    """fp32 flows on the CPU generator: 'frac' round(4 randn) + 0.1 + 0.8 rand (partly out of
    frame, never on an integer); 'int' integer-valued, with rows / columns 0..3 sampling exactly
    0, exactly size - 1 and beyond both; 'far' +-1e4; 'wide' x in +-50, y in +-3, fractional."""
    g = torch.Generator().manual_seed(seed)
    frac = 0.1 + 0.8 * torch.rand(B, 2, H, W, generator=g)
    if kind == 'frac':
        f = torch.round(4 * torch.randn(B, 2, H, W, generator=g)) + frac
    elif kind == 'int':
        f = torch.round(4 * torch.randn(B, 2, H, W, generator=g))
        xs, ys = torch.arange(W, dtype=FP32), torch.arange(H, dtype=FP32)
        for r, (tx, ty) in enumerate(((0, 0), (W - 1, H - 1), (-2, -2), (W + 1, H + 1))):
            if r < H:
                f[:, 0, r, :] = tx - xs
            if r < W:
                f[:, 1, :, r] = ty - ys
    elif kind == 'far':
        sign = 1 - 2 * (torch.rand(B, 2, H, W, generator=g) < 0.5).float()
        f = sign * (1e4 + frac)
    else:
        assert kind == 'wide'
        reach = torch.tensor([50., 3.]).view(1, 2, 1, 1)
        f = torch.round((torch.rand(B, 2, H, W, generator=g) * 2 - 1) * reach) + frac
    return f.to(device)


def _randn(shape, seed, dtype=FP32, device='cuda'):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(device).to(dtype)


# ---- k9: flow warp ------------------------------------------------------------------------
def _k9_refs(img, flow, gout):
    B, C, H, W = img.shape
    ir = _leaf64(img)
    ref = _warp_ref64(ir, flow)
    g64 = gout.detach().double()
    (dimg,) = torch.autograd.grad(ref, ir, g64)
    ia = _leaf64(img.abs())
    s_out = _warp_ref64(ia, flow)
    (s_img,) = torch.autograd.grad(s_out, ia, g64.abs())
    taps = _warp_taps(flow, H, W)[0]
    return dict(out=ref.detach(), dimg=dimg, s_out=s_out.detach(), s_img=s_img,
                n_img=_tap_count(taps, B, H, W) + 4,
                dflow=_warp_flow_grad64(ir.detach(), flow, g64),
                s_flow=4 * g64.abs().sum(1, keepdim=True) * float(img.abs().max()))


def _k9_run(img, flow, gout, refs, mode='atomic', check_out=True):
    """mode: 'atomic' (image scatter in the kernel), 'flow_only' (detached image) or
    'deterministic' (index_put_ scatter). Returns (d_image or None, d_flow)."""
    from imaginaire_amd.ops.flow_warp import _FlowWarpFn
    C = img.shape[1]
    x = img.detach().requires_grad_(mode != 'flow_only')
    f = flow.detach().requires_grad_(True)
    assert x.stride() == img.stride() and f.stride() == flow.stride()
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    if mode == 'deterministic':
        torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        out = _FlowWarpFn.apply(x, f)
        grads = torch.autograd.grad(out, (x, f) if x.requires_grad else (f,), gout)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert out.dtype == img.dtype and out.shape == img.shape
    if check_out:
        _check(out, refs['out'], 8, refs['s_out'], 'warp_fwd', 'out')
    dflow = grads[-1]
    assert dflow.dtype == flow.dtype
    _check(dflow, refs['dflow'], 4 * C + 4, refs['s_flow'], 'warp_bwd', 'd_flow/' + mode)
    if mode == 'flow_only':
        return None, dflow
    dimg = grads[0]
    assert dimg.dtype == img.dtype
    if img.is_contiguous(memory_format=torch.channels_last) and not img.is_contiguous():
        assert dimg.is_contiguous(memory_format=torch.channels_last)
    _check(dimg, refs['dimg'], refs['n_img'], refs['s_img'],
           'warp_bwd' if mode == 'atomic' else 'warp_bwd+index_put', 'd_image/' + mode)
    return dimg, dflow


def _k9_image(layout, B, C, H, W, dtype, seed):
    if layout == 'nchw':
        return _randn((B, C, H, W), seed, dtype)
    if layout == 'cl':
        return _randn((B, C, H, W), seed, dtype).contiguous(memory_format=torch.channels_last)
    if layout == 'frame':  # img_prev[:, -1] of a [B, T, C, H, W] clip
        return _randn((B, 3, C, H, W), seed, dtype)[:, -1]
    assert layout == 'chslice'  # x[:, :3] of a wider tensor
    return _randn((B, 2 * C, H, W), seed, dtype)[:, :C]


@gpu
@pytest.mark.parametrize('gout_cl', [False, True], ids=['g-nchw', 'g-cl'])
@pytest.mark.parametrize('flow_cl', [False, True], ids=['f-nchw', 'f-cl'])
@pytest.mark.parametrize('layout', ['nchw', 'cl', 'frame', 'chslice'])
def test_flow_warp_layouts(layout, flow_cl, gout_cl):
    B, C, H, W = 2, 3, 17, 23
    img = _k9_image(layout, B, C, H, W, FP32, 31)
    assert img.is_contiguous() == (layout == 'nchw')
    flow = _flows('frac', B, H, W, 32)
    gout = _randn((B, C, H, W), 33)
    if flow_cl:
        flow = flow.contiguous(memory_format=torch.channels_last)
    if gout_cl:
        gout = gout.contiguous(memory_format=torch.channels_last)
    _k9_run(img, flow, gout, _k9_refs(img, flow, gout))


@gpu
@pytest.mark.parametrize('img_dtype,flow_dtype', [(FP32, FP32), (BF16, BF16), (BF16, FP32),
                                                  (FP32, BF16)],
                         ids=['fp32-fp32', 'bf16-bf16', 'bf16-fp32', 'fp32-bf16'])
def test_flow_warp_dtypes(img_dtype, flow_dtype):
    """bf16 image with the fp32 flow FlowNet2 returns: the position keeps the flow's precision
    (a 50-pixel flow rounded to bf16 moves the sample by up to 0.125 px)."""
    B, C, H, W = 1, 3, 8, 160
    img = _randn((B, C, H, W), 41, img_dtype)
    flow = _flows('wide', B, H, W, 42).to(flow_dtype)
    gout = _randn((B, C, H, W), 43, img_dtype)
    _k9_run(img, flow, gout, _k9_refs(img, flow, gout))


@gpu
@pytest.mark.parametrize('img_dtype,flow_dtype', [(FP32, FP32), (BF16, BF16)],
                         ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind,shape', [('frac', (2, 3, 17, 23)), ('int', (2, 3, 17, 23)),
                                        ('far', (2, 3, 17, 23)), ('frac', (2, 3, 1, 23)),
                                        ('frac', (2, 3, 17, 1)), ('int', (2, 3, 1, 23)),
                                        ('int', (2, 3, 17, 1))],
                         ids=['frac', 'int', 'far', 'h1', 'w1', 'h1-int', 'w1-int'])
def test_flow_warp_positions(kind, shape, img_dtype, flow_dtype):
    B, C, H, W = shape
    img = _randn(shape, 51, img_dtype)
    flow = _flows(kind, B, H, W, 52).to(flow_dtype)
    gout = _randn(shape, 53, img_dtype)
    if kind == 'int' and min(H, W) > 4:  # samples on 0, on size - 1 and beyond both are there
        sx, sy = _pos32(flow, H, W)
        for s, size in ((sx, W), (sy, H)):
            assert bool((s == s.floor()).all())
            for v in (0, size - 1, -2, size + 1):
                assert bool((s == v).any())
    _, dflow = _k9_run(img, flow, gout, _k9_refs(img, flow, gout))
    if H == 1:
        assert not bool(dflow[:, 1].any())
    if W == 1:
        assert not bool(dflow[:, 0].any())


@gpu
def test_flow_warp_grid_stride():
    """2,111,500 pixels against the 8192 x 256 = 2,097,152 threads of the capped grid."""
    B, C, H, W = 1, 1, 1030, 2050
    assert B * H * W > 8192 * 256
    img = _randn((B, C, H, W), 61)
    flow = _flows('frac', B, H, W, 62)
    gout = _randn((B, C, H, W), 63)
    refs = _k9_refs(img, flow, gout)
    _k9_run(img, flow, gout, refs, 'atomic')
    _k9_run(img, flow, gout, refs, 'flow_only', check_out=False)


@gpu
@pytest.mark.parametrize('case', ['bf16-fp32', 'cl'])
def test_flow_warp_backward_modes_oracle(case):
    """Atomic, flow-only and deterministic backward, each against the oracle; the deterministic
    image gradient is bitwise equal on two runs."""
    B, C, H, W = 2, 3, 17, 23
    if case == 'cl':
        img = _k9_image('cl', B, C, H, W, FP32, 71)
    else:
        img = _randn((B, C, H, W), 71, BF16)
    flow = _flows('frac', B, H, W, 72)
    gout = _randn((B, C, H, W), 73, img.dtype)
    refs = _k9_refs(img, flow, gout)
    _k9_run(img, flow, gout, refs, 'atomic')
    _k9_run(img, flow, gout, refs, 'flow_only', check_out=False)
    d1, f1 = _k9_run(img, flow, gout, refs, 'deterministic', check_out=False)
    d2, f2 = _k9_run(img, flow, gout, refs, 'deterministic', check_out=False)
    assert torch.equal(d1, d2) and torch.equal(f1, f2)


# ---- k7: Resample2d -----------------------------------------------------------------------
def _k7_run(img, flow, gout, ks, backward=True):
    from imaginaire_amd.ops.flownet_ops import _Resample2dFn
    B, C, H, W = img.shape
    ir, fr = _leaf64(img), _leaf64(flow)
    ref = _resample_ref64(ir, fr, ks)
    ia = _leaf64(img.abs())
    s_out = _resample_ref64(ia, flow, ks)
    x = img.detach().requires_grad_(True)
    f = flow.detach().requires_grad_(True)
    out = _Resample2dFn.apply(x, f, ks)
    assert out.dtype == img.dtype and out.shape == img.shape
    _check(out, ref, 4 * ks * ks + 4, s_out.detach(), 'resample2d_fwd', 'out')
    if not backward:
        return
    g64 = gout.double()
    dimg_ref, dflow_ref = torch.autograd.grad(ref, (ir, fr), g64)
    (s_img,) = torch.autograd.grad(s_out, ia, g64.abs())
    dimg, dflow = torch.autograd.grad(out, (x, f), gout)
    assert dimg.dtype == img.dtype and dflow.dtype == flow.dtype
    n_img = _tap_count(_resample_taps(flow, H, W, ks), B, H, W) + 4
    _check(dimg, dimg_ref, n_img, s_img, 'resample2d_bwd', 'd_image')
    s_flow = 4 * ks * ks * g64.abs().sum(1, keepdim=True) * float(img.abs().max())
    _check(dflow, dflow_ref, 4 * ks * ks * C + 4, s_flow, 'resample2d_bwd', 'd_flow')


@gpu
@pytest.mark.parametrize('ks', [1, 2, 3])
@pytest.mark.parametrize('img_dtype,flow_dtype', [(FP32, FP32), (BF16, BF16), (BF16, FP32)],
                         ids=['fp32-fp32', 'bf16-bf16', 'bf16-fp32'])
@pytest.mark.parametrize('kind,shape', [('frac', (2, 3, 17, 23)), ('int', (2, 3, 17, 23)),
                                        ('far', (2, 3, 17, 23)), ('frac', (2, 3, 1, 23)),
                                        ('frac', (2, 3, 17, 1)), ('wide', (1, 3, 8, 160))],
                         ids=['frac', 'int', 'far', 'h1', 'w1', 'wide'])
def test_resample2d_positions(kind, shape, img_dtype, flow_dtype, ks):
    B, C, H, W = shape
    img = _randn(shape, 81, img_dtype)
    flow = _flows(kind, B, H, W, 82).to(flow_dtype)
    gout = _randn(shape, 83, img_dtype)
    _k7_run(img, flow, gout, ks)


@gpu
@pytest.mark.parametrize('ks', [1, 2])
def test_resample2d_channels_last(ks):
    shape = (2, 3, 17, 23)
    img = _k9_image('cl', *shape, FP32, 84)
    flow = _flows('frac', 2, 17, 23, 85).contiguous(memory_format=torch.channels_last)
    gout = _randn(shape, 86).contiguous(memory_format=torch.channels_last)
    _k7_run(img, flow, gout, ks)


@gpu
def test_resample2d_grid_stride_forward():
    """B C H W = 2,121,800 elements against the 2,097,152 threads of the capped grid."""
    shape = (1, 2, 1030, 1030)
    assert shape[1] * shape[2] * shape[3] > 8192 * 256
    _k7_run(_randn(shape, 87), _flows('frac', 1, 1030, 1030, 88), None, 1, backward=False)


@gpu
def test_resample2d_grid_stride_backward():
    """The backward runs one thread per pixel: 2,111,500 pixels."""
    shape = (1, 1, 1030, 2050)
    _k7_run(_randn(shape, 89), _flows('frac', 1, 1030, 2050, 90), _randn(shape, 91), 1)


# ---- k8: channel norm ---------------------------------------------------------------------
def _chnorm_ref64(x):
    """sqrt(sum_c x^2); the gradient g x / (norm + 1e-9) is returned by ``_chnorm_grad64``."""
    return (x * x).sum(1, keepdim=True).sqrt()


def _chnorm_grad64(x, g):
    return g * x / (_chnorm_ref64(x) + 1e-9)


def _k8_input(layout, N, C, H, W, dtype, seed):
    if layout == 'perm':  # dense, neither NCHW nor channels-last
        x = _randn((N, H, C, W), seed, dtype).permute(0, 2, 1, 3)
    else:
        x = _randn((N, C, H, W), seed, dtype)
        if layout == 'cl':
            x = x.contiguous(memory_format=torch.channels_last)
    x[0, :, 3, 4] = 0  # a pixel whose vector is all zero
    return x


@gpu
@pytest.mark.parametrize('layout', ['nchw', 'cl', 'perm'])
@pytest.mark.parametrize('C', [1, 5, 400])
@pytest.mark.parametrize('dtype', [FP32, BF16], ids=['fp32', 'bf16'])
def test_channelnorm_paths(dtype, C, layout):
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.ops.flownet_ops import _ChannelNormFn
    N, H, W = 2, 7, 19
    assert (N * H * W) % 256 != 0 and N * H * W > 256
    x = _k8_input(layout, N, C, H, W, dtype, 95).requires_grad_(True)
    assert _ext.is_dense(x) and x.is_contiguous() == (layout == 'nchw' or C == 1)
    y = _ChannelNormFn.apply(x)
    assert y.shape == (N, 1, H, W) and y.dtype == dtype
    x64 = x.detach().double()
    ref = _chnorm_ref64(x64)
    _check(y, ref, C + 4, ref, 'chnorm_fwd', 'out')
    g = _randn((N, 1, H, W), 96, dtype)
    (dx,) = torch.autograd.grad(y, x, g)
    assert dx.dtype == dtype
    dref = _chnorm_grad64(x64, g.double())
    _check(dx, dref, C + 4, dref.abs(), 'chnorm_bwd', 'd_x')
    assert float(y.detach()[0, 0, 3, 4]) == 0 and not bool(dx[0, :, 3, 4].any())


@gpu
@pytest.mark.parametrize('dtype', [FP32, BF16], ids=['fp32', 'bf16'])
def test_channelnorm_channel_slice_forward(dtype):
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.ops.flownet_ops import _ChannelNormFn
    x = _randn((2, 6, 7, 19), 97, dtype)[:, 1:4]
    assert not _ext.is_dense(x)
    ref = _chnorm_ref64(x.double())
    _check(_ChannelNormFn.apply(x), ref, 3 + 4, ref, 'chnorm_fwd', 'out/slice')
