"""The paired SPADE norms (``fused_norm_act_pair``: two modulations of one batch norm, read from
the map BEFORE its nearest upsampling) and the γ|β conv bias gradient summed by the norm's
backward (``BiasGradHolder``), on the GPU.

* the pair op against the formula written out in float64 (gradients by float64 autograd), in
  the style and at the tolerances of ``test_norm_paths_gpu``: N = 2, UP 1 and 2, low-res 3x5
  with C = 8, 5x7 with C = 24 (3 threads per pixel row, a ragged last chunk), 16x24 with C = 64
  (several pixel chunks), slopes (0.2, 1.0), bf16 and fp32, training and eval;
* the pair op against the unpaired HIP path on the same inputs (running statistics included);
* the holder's [2C] vector against the k2 bias pass over the very dγ|dβ map the kernel wrote,
  within ``n·2⁻²³·Σ|v|`` per channel (n summed elements): only the fp32 order may differ, which a
  sum over the unrounded values would miss in bf16;
* every fallback gives today's result through today's launches;
* one unit-test SPADE training step: graph replay against eager, pair on against off.
"""
import os
import types

import pytest
import torch

gpu = pytest.mark.gpu
BF16, FP32 = torch.bfloat16, torch.float32
EPS = 1e-5
CL = torch.channels_last
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOPES = (0.2, 1.0)
# (h, w, C) of the low-resolution map, N = 2
SHAPES = [(3, 5, 8), (5, 7, 24), (16, 24, 64)]


def _tol(dtype):
    return 2e-2 if dtype == BF16 else 1e-4


def _scale(t):
    return max(1.0, float(t.abs().max()))


def _close(got, ref, atol, rtol, name):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), '%s: %d of %d off, max err %.3e (atol %.3e)' % (
        name, int(bad.sum()), bad.numel(), float(err.max()), atol)


def _act(y, slope, mask=None):
    if slope == 1.0:
        return y
    return torch.where(y > 0 if mask is None else mask, y, y * slope)


def _up64(x, up):
    return x.repeat_interleave(up, 2).repeat_interleave(up, 3) if up != 1 else x


def _inputs(h, w, C, up, dtype, seed, layout=CL):
    torch.manual_seed(seed)
    N = 2
    x = (torch.randn(N, C, h, w, device='cuda') * 2 + 0.5).to(dtype)
    gbs = [(torch.randn(N, 2 * C, h * up, w * up, device='cuda') * 0.3).to(dtype)
           for _ in range(2)]
    gos = [torch.randn(N, C, h * up, w * up, device='cuda').to(dtype) for _ in range(2)]
    return [t.contiguous(memory_format=layout) for t in [x] + gbs + gos]


def _running(C, eval_mode):
    """Per norm (running_mean, running_var, num_batches); distinct values per norm."""
    out = []
    for k in range(2):
        rm = torch.randn(C, device='cuda') * 0.5 + 0.3 * (k + 1)
        rv = torch.rand(C, device='cuda') * 3 + 1
        nb = None if eval_mode else torch.tensor([5 + k], device='cuda', dtype=torch.int64)
        out.append((rm, rv, nb))
    return out


def _cfg(training):
    from imaginaire_amd.ops.norm import _NormCfg
    return _NormCfg('batch', training, 0.1 if training else 0.0, EPS, 1.0, None)


def _plan(x):
    from imaginaire_amd.ops import _ext
    return dict(_ext.ext().norm_plan(x, False))


@gpu
@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', [BF16, FP32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('up', [1, 2])
@pytest.mark.parametrize('h,w,C', SHAPES)
def test_pair_against_float64(h, w, C, up, dtype, mode, affine):
    from imaginaire_amd.ops.norm import _FusedNormActPairFn, fused_norm_act_pair
    x, gb0, gbs, go0, gos = _inputs(h, w, C, up, dtype, 11 * C + up)
    # the pair kernels take 8 channels per lane in either dtype: the plan of a bf16 tensor
    p = _plan(x.to(BF16).contiguous(memory_format=CL))
    assert p['cl'] and p['vec'] == 8
    if C == 24:  # 3 threads per pixel row: 85 rows, the last chunk is short
        assert p['tpr'] == 3 and p['rpb'] == 85 and (h * w) % p['chunk'] != 0
    if C == 64:
        assert p['P'] > 1
    training = mode == 'train'
    run = _running(C, not training)
    run0 = [(rm.clone(), rv.clone(), None if nb is None else nb.clone()) for rm, rv, nb in run]
    leaves = [t.clone(memory_format=torch.preserve_format).requires_grad_(True)
              for t in (x, gb0, gbs)]
    aff = [(None, None), (None, None)]
    if affine:  # each norm's own per-channel weight and bias
        aff = [((torch.randn(C, device='cuda') * 0.5 + 1).requires_grad_(True),
                (torch.randn(C, device='cuda') * 0.1).requires_grad_(True)) for _ in range(2)]
    n0 = _FusedNormActPairFn.launches
    y0, ys = fused_norm_act_pair(leaves[0], up, leaves[1], leaves[2], SLOPES, _cfg(training),
                                 running=run, affines=aff)
    assert _FusedNormActPairFn.launches == n0 + 1
    assert y0.shape == go0.shape and ys.shape == go0.shape and y0.dtype == dtype
    torch.autograd.backward([y0, ys], [go0, gos])

    # float64: upsample, statistics of the upsampled tensor, the two modulations
    xr = x.double().requires_grad_(True)
    gr = [g.double().requires_grad_(True) for g in (gb0, gbs)]
    xu = _up64(xr, up)
    n = xu.numel() // C
    mean = xu.mean((0, 2, 3), keepdim=True)
    var = ((xu - mean) ** 2).mean((0, 2, 3), keepdim=True)
    tol = _tol(dtype)
    refs = []
    affr = [[None if t is None else t.detach().double().requires_grad_(True) for t in ab]
            for ab in aff]
    for k, (g, y) in enumerate(zip(gr, (y0, ys))):
        if training:
            xh = (xu - mean) / torch.sqrt(var + EPS)
        else:
            xh = (xu - run0[k][0].double().reshape(1, C, 1, 1)) / torch.sqrt(
                run0[k][1].double().reshape(1, C, 1, 1) + EPS)
        if affine:
            xh = xh * affr[k][0].reshape(1, C, 1, 1) + affr[k][1].reshape(1, C, 1, 1)
        pre = xh * (1 + g[:, :C]) + g[:, C:]
        mask = None
        if dtype == BF16 and SLOPES[k] != 1.0:
            # bf16 sign ties of a pre-activation within a rounding of 0: the mask of the
            # kernel's own output; the two may differ on isolated elements only
            mask = y.detach() > 0
            assert float((mask != (pre.detach() > 0)).double().mean()) <= 0.01
        refs.append(_act(pre, SLOPES[k], mask))
        _close(y, refs[-1].detach(), tol * 5, tol, 'y%d' % k)
    torch.autograd.backward(refs, [go0.double(), gos.double()])
    _close(leaves[0].grad, xr.grad, tol * 5 * _scale(xr.grad), tol * 5, 'dx')
    for k in range(2):
        _close(leaves[1 + k].grad, gr[k].grad, tol * 5 * _scale(gr[k].grad), tol * 5,
               'dgb%d' % k)
        if affine:
            for j, name in enumerate(('dw', 'db')):
                got, ref = aff[k][j].grad, affr[k][j].grad
                assert got.dtype == aff[k][j].dtype
                _close(got, ref, tol * 20 * _scale(ref), tol * 5, '%s%d' % (name, k))
    for k in range(2):
        rm, rv, nb = run[k]
        if training:  # both norms: the statistics of the UPSAMPLED tensor
            _close(rm, 0.9 * run0[k][0].double() + 0.1 * mean.reshape(-1), 1e-3, 1e-3, 'rm')
            _close(rv, 0.9 * run0[k][1].double() + 0.1 * var.reshape(-1) * n / (n - 1), 1e-3,
                   1e-3, 'rv')
            assert int(nb) == int(run0[k][2]) + 1
        else:
            assert torch.equal(rm, run0[k][0]) and torch.equal(rv, run0[k][1])


def _unpaired(x, up, gb0, gbs, run, holders=(None, None), aff=((None, None), (None, None))):
    from imaginaire_amd.ops.norm import fused_norm_act
    from imaginaire_amd.ops.resize import interpolate
    xu = interpolate(x, scale_factor=float(up), mode='nearest') if up != 1 else x
    outs = []
    for gb, slope, (rm, rv, nb), hd, (w, b) in zip((gb0, gbs), SLOPES, run, holders, aff):
        outs.append(fused_norm_act(xu, 'batch', w, b, gb=gb, running_mean=rm, running_var=rv,
                                   training=True, momentum=0.1, eps=EPS, slope=slope,
                                   num_batches=nb, bias_grad=hd))
    return outs


@gpu
@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
@pytest.mark.parametrize('dtype', [BF16, FP32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('up', [1, 2])
@pytest.mark.parametrize('h,w,C', SHAPES)
def test_pair_against_unpaired_hip_path(h, w, C, up, dtype, affine):
    """The statistics of the pair are those of the materialised upsampled tensor bit for bit
    (the same kernels visit the same values in the same order), so the forward of the pair
    equals the unpaired HIP path exactly: both outputs, both dγ|dβ maps (which depend on
    forward quantities alone), num_batches, and the running statistics wherever the unpaired
    path updates them in the statistics kernel too (norm 0; norm s when it has an affine and
    so computes its own statistics; otherwise fp32 tolerance against its PyTorch update).
    dx_low against nearest_bwd(dx0 + dxs) (autograd's) and the affine gradients differ by the
    fp32 order of S1 / S2 alone: the float64 test's tolerances."""
    from imaginaire_amd.ops.norm import fused_norm_act_pair
    x, gb0, gbs, go0, gos = _inputs(h, w, C, up, dtype, 5 * C)
    res = []
    for pair in (True, False):
        torch.manual_seed(1)
        run = _running(C, False)
        aff = [(None, None), (None, None)]
        if affine:
            aff = [((torch.randn(C, device='cuda') * 0.5 + 1).requires_grad_(True),
                    (torch.randn(C, device='cuda') * 0.1).requires_grad_(True))
                   for _ in range(2)]
        leaves = [t.clone(memory_format=torch.preserve_format).requires_grad_(True)
                  for t in (x, gb0, gbs)]
        if pair:
            y0, ys = fused_norm_act_pair(leaves[0], up, leaves[1], leaves[2], SLOPES,
                                         _cfg(True), running=run, affines=aff)
        else:
            y0, ys = _unpaired(leaves[0], up, leaves[1], leaves[2], run, aff=aff)
        torch.autograd.backward([y0, ys], [go0, gos])
        res.append((y0, ys, [t.grad for t in leaves], run, aff))
    (p0, ps, pg, prun, paff), (u0, us, ug, urun, uaff) = res
    tol = _tol(dtype)
    assert torch.equal(p0, u0) and torch.equal(ps, us), 'forward outputs'
    assert torch.equal(pg[1], ug[1]) and torch.equal(pg[2], ug[2]), 'dgb maps'
    _close(pg[0], ug[0], tol * 5 * _scale(ug[0]), tol * 5, 'dx_low')
    for k, ((prm, prv, pnb), (urm, urv, unb)) in enumerate(zip(prun, urun)):
        if k == 0 or affine:
            assert torch.equal(prm, urm) and torch.equal(prv, urv), 'running statistics %d' % k
        else:
            _close(prm, urm, 1e-5, 1e-5, 'running_mean')
            _close(prv, urv, 1e-5, 1e-5, 'running_var')
        assert int(pnb) == int(unb)
    if affine:
        for k in range(2):
            for j, name in enumerate(('dw', 'db')):
                ref = uaff[k][j].grad
                _close(paff[k][j].grad, ref, tol * 20 * _scale(ref), tol * 5, '%s%d' % (name, k))


def _bias_bound(dgb):
    """n·2⁻²³·Σ|v| per channel of the [N, 2C, H, W] map, in float64 (n = N·H·W summed
    elements: at most 2048 here, but 3072 for the 16x24 low-res map at UP = 2)."""
    n = dgb.shape[0] * dgb.shape[2] * dgb.shape[3]
    assert n <= 3072
    return n * 2.0 ** -23 * dgb.double().abs().sum((0, 2, 3))


def _check_bias(holder, dgb, name):
    from imaginaire_amd.ops.conv import _bias_grad
    assert holder.db is not None and holder.db.dtype == FP32
    assert tuple(holder.db.shape) == (dgb.shape[1],)
    ref = _bias_grad(dgb.contiguous(memory_format=CL))[:dgb.shape[1]].double()
    err = (holder.db.double() - ref).abs()
    bound = _bias_bound(dgb)
    worst = float((err - bound).max())
    print('%s: max |Δ| %.3e, smallest bound %.3e' % (name, float(err.max()), float(bound.min())))
    assert worst <= 0.0, '%s: |Δ| exceeds n·2^-23·Σ|v| by %.3e' % (name, worst)


@gpu
@pytest.mark.parametrize('dtype', [BF16, FP32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('layout', ['cl', 'nchw'])
@pytest.mark.parametrize('h,w,C', [(6, 10, 8), (10, 14, 24), (32, 32, 64)])
def test_bias_sums_single_reduce(h, w, C, layout, dtype):
    from imaginaire_amd.ops.norm import BiasGradHolder, fused_norm_act
    fmt = CL if layout == 'cl' else torch.contiguous_format
    x, gb, _, go, _ = _inputs(h, w, C, 1, dtype, 3 * C + h, fmt)
    assert _plan(x)['cl'] == (layout == 'cl')
    gb.requires_grad_(True)
    x.requires_grad_(True)
    holder = BiasGradHolder()
    y = fused_norm_act(x, 'batch', gb=gb, training=True, momentum=0.0, eps=EPS, slope=0.2,
                       bias_grad=holder)
    y.backward(go)
    _check_bias(holder, gb.grad, 'single %s' % layout)


@gpu
@pytest.mark.parametrize('dtype', [BF16, FP32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('up', [1, 2])
@pytest.mark.parametrize('h,w,C', SHAPES)
def test_bias_sums_pair_reduce(h, w, C, up, dtype):
    from imaginaire_amd.ops.norm import BiasGradHolder, fused_norm_act_pair
    x, gb0, gbs, go0, gos = _inputs(h, w, C, up, dtype, 7 * C + up)
    for t in (x, gb0, gbs):
        t.requires_grad_(True)
    holders = (BiasGradHolder(), BiasGradHolder())
    y0, ys = fused_norm_act_pair(x, up, gb0, gbs, SLOPES, _cfg(True), holders=holders)
    torch.autograd.backward([y0, ys], [go0, gos])
    _check_bias(holders[0], gb0.grad, 'pair norm 0')
    _check_bias(holders[1], gbs.grad, 'pair norm s')


# ---- the block: pair path and its fallbacks ---------------------------------------------------
def _block(cin, cout, norm='sync_batch', conds=5, affine=False):
    from imaginaire_amd.layers import Res2dBlock
    params = types.SimpleNamespace(
        num_filters=64, kernel_size=3, cond_dims=conds, separate_projection=True,
        activation_norm_type=norm, weight_norm_type='',
        activation_norm_params=types.SimpleNamespace(affine=affine))
    torch.manual_seed(3)
    blk = Res2dBlock(cin, cout, kernel_size=3, padding=1, bias=[True, True, False],
                     weight_norm_type='', activation_norm_type='spatially_adaptive',
                     activation_norm_params=params, skip_activation_norm=True,
                     nonlinearity='leakyrelu', order='NACNAC')
    return blk.cuda()


def _run_block(blk, x, segs, pre, go):
    """One bf16-autocast forward / backward; returns (output, dx, parameter gradients, pair
    launches, holders used)."""
    from imaginaire_amd.ops.norm import BiasGradHolder, _FusedNormActPairFn
    from imaginaire_amd.ops.resize import interpolate
    blk.zero_grad(set_to_none=True)
    x = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    n0, u0 = _FusedNormActPairFn.launches, BiasGradHolder.used
    with torch.autocast('cuda', dtype=BF16):
        if pre:
            y = blk(x, *segs, pre_upsample=2)
        else:
            y = blk(interpolate(x, scale_factor=2.0, mode='nearest'), *segs)
    y.backward(go.to(y.dtype))
    grads = {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None}
    return y.detach(), x.grad, grads, _FusedNormActPairFn.launches - n0, \
        BiasGradHolder.used - u0


def _same(a, b, exact, name):
    if exact:
        assert torch.equal(a, b), name
    else:  # fp32 summation order (statistics, S1 / S2, bias sums) under bf16 tensors
        _close(a, b, 2e-2 * 5 * _scale(b), 2e-2 * 5, name)


def _compare_runs(new, old, exact):
    _same(new[0], old[0], exact, 'y')
    _same(new[1], old[1], exact, 'dx')
    assert set(new[2]) == set(old[2])
    for k in old[2]:
        _same(new[2][k], old[2][k], exact, k)


@gpu
@pytest.mark.parametrize('case', ['pair', 'C12', 'nchw', 'affine', 'two_conds', 'switch_off',
                                  'identity_shortcut'])
def test_block_pair_path_and_fallbacks(case, monkeypatch):
    """``block(x_low, seg, pre_upsample=2)`` against ``block(upsample(x_low), seg)`` (today's
    call). The pair kernel runs in the 'pair' case alone; every fallback takes today's
    launches and gives today's result bit for bit (deterministic mode: no atomics). 'pair' has
    the frozen per-channel affine of a SPADE 'sync_batch' layer built with affine=False, 'affine'
    the trainable one of the SPADE generator's default: both are pair cases, their weight and
    bias gradients included (the pair kernels carry each norm's affine)."""
    cin, cout, conds, affine = 64, 32, 5, False
    if case == 'C12':
        cin = 12
    if case == 'affine':
        affine = True  # trainable norm weights and biases
    if case == 'identity_shortcut':
        cout = cin
    blk = _block(cin, cout, conds=[5, 5] if case == 'two_conds' else conds, affine=affine)
    if case == 'switch_off':
        monkeypatch.setenv('IMAGINAIRE_AMD_SPADE_PAIR', '0')
    torch.manual_seed(9)
    x = torch.randn(2, cin, 6, 10, device='cuda').to(BF16)
    if case != 'nchw':
        x = x.contiguous(memory_format=CL)
    nseg = 2 if case == 'two_conds' else 1
    segs = [torch.randn(2, 5, 12, 20, device='cuda').contiguous(memory_format=CL)
            for _ in range(nseg)]
    go = torch.randn(2, cout, 12, 20, device='cuda').contiguous(memory_format=CL)
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        state = {k: v.clone() for k, v in blk.state_dict().items()}
        new = _run_block(blk, x, segs, True, go)
        state_new = {k: v.clone() for k, v in blk.state_dict().items()}
        blk.load_state_dict(state)
        old = _run_block(blk, x, segs, False, go)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    paired = case in ('pair', 'affine')
    assert new[3] == (1 if paired else 0) and old[3] == 0
    _compare_runs(new, old, exact=not paired)
    for k, v in blk.state_dict().items():  # running statistics and batch counters
        if paired and v.is_floating_point():
            _close(state_new[k], v, 1e-5, 1e-5, k)
        else:
            assert torch.equal(state_new[k], v), k
    # the γ|β convs took their bias gradient from the norms' backward on both routes
    if paired:
        assert new[4] >= 2 and old[4] >= 2


@gpu
def test_empty_holder_falls_back(monkeypatch):
    """A norm backward that leaves the holders empty: the convs sum their bias gradient
    themselves, and the result is the one with the hand-over."""
    from imaginaire_amd.ops.norm import BiasGradHolder
    blk = _block(64, 32)
    torch.manual_seed(4)
    x = torch.randn(2, 64, 6, 10, device='cuda').to(BF16).contiguous(memory_format=CL)
    seg = torch.randn(2, 5, 12, 20, device='cuda').contiguous(memory_format=CL)
    go = torch.randn(2, 32, 12, 20, device='cuda').contiguous(memory_format=CL)
    # (deterministic mode, as in the block test above: these small γ|β convs then take the k10
    # route, whose backward is the one that looks into the holder)
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        with_holder = _run_block(blk, x, [seg], True, go)
        assert with_holder[4] >= 2
        monkeypatch.setattr(BiasGradHolder, 'fill', lambda self, db, dgb: None)
        without = _run_block(blk, x, [seg], True, go)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert without[4] == 0 and without[3] == 1
    for k, g in with_holder[2].items():
        if k.endswith('.bias') and ('gammas' in k or 'betas' in k):
            # both are fp32 sums of the same 480 bf16 numbers per channel, in another order
            _close(g, without[2][k], 1e-3 * _scale(without[2][k]), 1e-3, k)


# ---- captured: no memset node, no host read ----------------------------------------------------
@gpu
def test_pair_capture_has_no_memset_node(tmp_path):
    from imaginaire_amd.ops.norm import BiasGradHolder, fused_norm_act_pair
    h, w, C, up = 16, 24, 64, 2
    x, gb0, gbs, go0, gos = _inputs(h, w, C, up, BF16, 2)
    for t in (x, gb0, gbs):
        t.requires_grad_(True)
    run = _running(C, False)

    def step():
        holders = (BiasGradHolder(), BiasGradHolder())
        y0, ys = fused_norm_act_pair(x, up, gb0, gbs, SLOPES, _cfg(True), holders=holders,
                                     running=run)
        return torch.autograd.grad([y0, ys], [x, gb0, gbs], [go0, gos])

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        eager = step()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    dot = str(tmp_path / 'pair.dot')
    g = torch.cuda.CUDAGraph(keep_graph=True)
    g.enable_debug_mode()
    with torch.cuda.graph(g, stream=st):  # a host read would fail the capture here
        grads = step()
    g.debug_dump(dot)
    g.instantiate()
    g.replay()
    torch.cuda.synchronize()
    with open(dot) as f:
        text = f.read()
    assert 'KERNEL' in text.upper()
    assert 'MEMSET' not in text.upper(), 'memset node in the captured pair op'
    for a, b in zip(grads, eager):
        _close(a, b, 2e-2 * 5 * _scale(b), 2e-2 * 5, 'replayed gradient')


# ---- one training step --------------------------------------------------------------------------
def _trainer(tmp):
    from imaginaire_amd.config import Config
    from imaginaire_amd.utils.trainer import get_model_optimizer_and_scheduler, get_trainer
    torch.manual_seed(0)
    cfg = Config(os.path.join(ROOT, 'configs', 'unit_test', 'spade.yaml'))
    cfg.speed_benchmark = False
    cfg.logdir = str(tmp)
    nets = get_model_optimizer_and_scheduler(cfg, seed=0)
    tr = get_trainer(cfg, *nets, train_data_loader=[], val_data_loader=None)
    tr.net_G_module.style_encoder.freeze_random = True
    return cfg, tr


def _state_tensors(tr):
    ts = list(tr.net_G.parameters()) + list(tr.net_G.buffers())
    ts += list(tr.net_D.parameters()) + list(tr.net_D.buffers())
    for o in (tr.opt_G, tr.opt_D):
        for st in o.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
        ts += [g['_hyper'] for g in o.param_groups if '_hyper' in g]
    return ts


@gpu
def test_training_step_graph_and_switch(tmp_path, monkeypatch):
    """configs/unit_test/spade.yaml: the captured step replays what the eager step computes
    (the bounds of test_graph_gpu.test_graph_replay_matches_eager), with the pair kernels in
    it; the same step with IMAGINAIRE_AMD_SPADE_PAIR=0 agrees within the same bounds."""
    from imaginaire_amd.datasets.synthetic import DeviceBatchSource
    from imaginaire_amd.ops.norm import BiasGradHolder, _FusedNormActPairFn
    from imaginaire_amd.utils.cuda_graph import make_trainer_step
    torch.cuda.set_device(0)
    cfg, tr = _trainer(tmp_path)
    src = DeviceBatchSource(cfg, 2, torch.device('cuda', 0), pool=4, seed=0)
    batches = [src.next() for _ in range(4)]
    step, graphed = make_trainer_step(tr, warmup=2, enabled=True)
    assert graphed is not None
    for i, b in enumerate(batches[:3]):
        torch.manual_seed(1)
        # (the third call captures: the pair kernels and the bias hand-over are in the graph)
        n0, u0, f0 = _FusedNormActPairFn.launches, BiasGradHolder.used, BiasGradHolder.filled
        step(tr.start_of_iteration({k: v.clone() if torch.is_tensor(v) else v
                                    for k, v in b.items()}, i))
    torch.cuda.synchronize()
    assert graphed.graph is not None and not graphed.failed, 'step was not captured'
    print('pair launches in the captured step: %d, holders used: %d' % (
        _FusedNormActPairFn.launches - n0, BiasGradHolder.used - u0))
    # up_0a and up_1a pair in every generator forward of the step; its one generator backward
    # has 19 SPADE norms, each fills a holder, and every γ|β conv takes its own (no silent
    # fall-back)
    assert _FusedNormActPairFn.launches - n0 == 2 * 2  # two generator forwards per step
    assert BiasGradHolder.filled - f0 == 19 and BiasGradHolder.used - u0 == 19
    # (the capture succeeded, so the step made no host read. Its graph does hold memset nodes,
    # from zero-filled buffers elsewhere in the step as in the parent; that the pair op adds
    # none is what test_pair_capture_has_no_memset_node checks on a capture of the op alone)

    state = _state_tensors(tr)
    saved = [t.detach().clone() for t in state]
    gparams = list(tr.net_G.parameters())

    def one(fn, d):
        with torch.no_grad():
            for t, c in zip(state, saved):
                t.copy_(c)
        torch.cuda.synchronize()
        fn(d)
        torch.cuda.synchronize()
        loss = (float(tr.dis_losses['total']), float(tr.gen_losses['total']))
        return loss, [None if p.grad is None else p.grad.detach().float().clone()
                      for p in gparams]

    d = tr.start_of_iteration({k: v.clone() if torch.is_tensor(v) else v
                               for k, v in batches[3].items()}, 3)
    lg, gg = one(graphed, d)
    le, ge = one(graphed.step_fn, d)
    monkeypatch.setenv('IMAGINAIRE_AMD_SPADE_PAIR', '0')
    n1 = _FusedNormActPairFn.launches
    lo, go = one(graphed.step_fn, d)
    assert _FusedNormActPairFn.launches == n1
    print('graph', lg, 'eager', le, 'pair off', lo)
    for name, (la, ga) in (('graph', (lg, gg)), ('pair off', (lo, go))):
        assert all(v == v and abs(v) != float('inf') for v in la), (name, la)
        assert abs(la[0] - le[0]) <= 1e-3 * max(1.0, abs(le[0])), (name, la, le)
        assert abs(la[1] - le[1]) <= 1e-3 * max(1.0, abs(le[1])), (name, la, le)
        num = sum(float((a - b).pow(2).sum()) for a, b in zip(ga, ge) if a is not None)
        den = sum(float(b.pow(2).sum()) for a, b in zip(ga, ge) if a is not None)
        assert den > 0 and num <= 1e-4 * den, (name, num, den)
