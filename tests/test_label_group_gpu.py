"""The grouped launch of the SPADE label convs (ops/conv.py ``conv2d_act_group`` /
``_MfmaConvGroup``, csrc ``conv2d_mfma_grouped`` / ``bias_act_bwd_grouped`` /
``conv2d_wgrad_mfma_grouped``) against the same layers run one by one and against fp32 PyTorch,
at kernel level and through ``SpatiallyAdaptiveNorm`` under a ``LabelMapCache``.

Tolerances are those of tests/test_kernels_gpu.py::test_conv2d_mfma_fwd_bwd for the ungrouped
path: outputs 1e-2 and gradients 2e-2 of max(1, |reference|max)."""
import contextlib
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
G, CIN, CINP, COUT, K, PAD = 3, 185, 192, 128, 5, 2
SHAPES = [(1, 16, 16),   # one 256-pixel tile per group: a grid of 3 tiles, split-K engages
          (2, 16, 32),   # the bench's smallest row width
          (1, 8, 64)]    # 64-pixel rows


@pytest.fixture
def small_grids(monkeypatch):
    """k10 / k11 for grids below the eager thresholds, the variant choice left untouched."""
    from imaginaire_amd.ops import conv as C
    monkeypatch.setattr(C, '_MFMA_MIN_BLOCKS', 0)
    # (the gamma|beta convs' data gradients too: MIOpen's small-problem solvers sum with atomics)
    monkeypatch.setattr(C, '_MFMA_MIN_DGRAD_BLOCKS', 0)
    monkeypatch.setattr(C, '_MFMA_WGRAD', '1')
    monkeypatch.setattr(C, '_WGRAD_PENDING', {})
    monkeypatch.delenv('IMAGINAIRE_AMD_SPADE_GROUP', raising=False)
    monkeypatch.delenv('IMAGINAIRE_AMD_CONV_SPLITK', raising=False)
    return C


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Label map (192 channels, 185 valid), per group a bf16-exact fp32 W, u, v, bias, output
    gradient; the fp32 reference outputs and gradients of relu(conv(x, W / (u^T W v)) + b)."""
    B, H, W = shape
    torch.manual_seed(7)
    x = torch.zeros(B, CINP, H, W, device='cuda', dtype=BF).contiguous(memory_format=CL)
    x[:, :CIN] = torch.randn(B, CIN, H, W, device='cuda').to(BF)
    groups = []
    for g in range(G):
        w = (torch.randn(COUT, CIN, K, K, device='cuda') * (1.0 + 0.5 * g) / (CIN * K * K) ** 0.5 +
             torch.arange(COUT, device='cuda').view(-1, 1, 1, 1) * 1e-3).to(BF).float()
        w = w.contiguous(memory_format=CL)
        u = F.normalize(torch.randn(COUT, device='cuda'), dim=0)
        v = F.normalize(torch.randn(CIN * K * K, device='cuda'), dim=0)
        b = torch.randn(COUT, device='cuda') * 0.1
        go = torch.randn(B, COUT, H, W, device='cuda').to(BF).contiguous(memory_format=CL)
        groups.append((w, u, v, b, go))
    return x, groups


def _members(C, shape):
    """Fresh parameters and SNWeights over the shared data."""
    x, groups = _data(shape)
    C.mark_zero_tail(x, CIN)
    ws, bs, sws = [], [], []
    for w, u, v, b, _ in groups:
        W = torch.nn.Parameter(w.clone(memory_format=torch.preserve_format))
        sigma = (u @ w.reshape(COUT, -1) @ v).detach()
        sws.append(C.SNWeight(W, w.to(BF).contiguous(memory_format=CL), u, v, sigma, None, None))
        ws.append(W)
        bs.append(torch.nn.Parameter(b.clone()))
    return x, ws, bs, sws


def _reference(shape, ys):
    """fp32 autograd: outputs (activation mask from the kernel's own output), dW, db."""
    x, groups = _data(shape)
    outs = []
    for (w, u, v, b, go), y in zip(groups, ys):
        wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yr = F.conv2d(x[:, :CIN].float(), wr / (u @ wr.reshape(COUT, -1) @ v), br, 1, PAD)
        yr = torch.where(y.detach().float() > 0, yr, yr * 0.0)
        yr.backward(go.float())
        outs.append((yr.detach(), wr.grad, br.grad))
    return outs


@contextlib.contextmanager
def _conv_log(C):
    C.enable_conv_log(True)
    try:
        yield
    finally:
        C.enable_conv_log(False)


def _label_rows(rows, kind):
    """{kernel label: calls} of the label-conv rows of a conv-log summary."""
    out = {}
    for k, path, desc, calls, _, _ in rows:
        if k == kind and '[%d, %d, %d, %d]' % (COUT, CINP, K, K) in desc:
            out[path.split('/')[0]] = out.get(path.split('/')[0], 0) + calls
    return out


@pytest.mark.parametrize('split', ['1', '2'])
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_bitwise_with_split_pinned(small_grids, monkeypatch, shape, split):
    """Same tile, k order and split: each group's output equals the layer alone, bit for bit."""
    C = small_grids
    monkeypatch.setenv('IMAGINAIRE_AMD_CONV_SPLITK', split)
    x, ws, bs, sws = _members(C, shape)
    with torch.no_grad(), _conv_log(C):
        ys = C.conv2d_act_group(x, sws, bs, 1, PAD, 1, 0.0)
        rows = C.conv_log_summary()
        alone = [C.conv2d_act(x, sw, b, 1, PAD, 1, 0.0) for sw, b in zip(sws, bs)]
        rows1 = C.conv_log_summary()
    assert _label_rows(rows, 'fwd') == {'k10g': 1}, rows
    assert _label_rows(rows1, 'fwd') == {'k10': G}, rows1
    for g in range(G):
        assert ys[g].shape == alone[g].shape and ys[g].is_contiguous(memory_format=CL)
        assert torch.equal(ys[g], alone[g]), g


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_and_gradients(small_grids, shape):
    """Split free: outputs, dW (with the spectral-norm backward) and db against fp32 autograd
    of W / (u^T W v); gradients against the one-by-one path, bitwise where conv2d_wgrad_plan
    names the same k11 kernel and S for the concatenated and the single GEMM."""
    C = small_grids
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    x, ws, bs, sws = _members(C, shape)
    _, groups = _data(shape)
    with _conv_log(C):
        ys = C.conv2d_act_group(x, sws, bs, 1, PAD, 1, 0.0)
        torch.autograd.backward(ys, [g[4] for g in groups])
        rows = C.conv_log_summary()
    assert _label_rows(rows, 'fwd') == {'k10g': 1} and _label_rows(rows, 'wgrad') == {'k11g': 1}, \
        rows
    ref = _reference(shape, ys)
    x1, ws1, bs1, sws1 = _members(C, shape)
    ys1 = [C.conv2d_act(x1, sw, b, 1, PAD, 1, 0.0) for sw, b in zip(sws1, bs1)]
    torch.autograd.backward(ys1, [g[4] for g in groups])
    B, H, W = shape
    dyg = torch.empty(B, G * COUT, H, W, device='cuda', dtype=BF).contiguous(memory_format=CL)
    dy1 = torch.empty(B, COUT, H, W, device='cuda', dtype=BF).contiguous(memory_format=CL)
    pg = X.conv2d_wgrad_plan(dyg, x, K, K, 1, 1, PAD, PAD, 1, 1)
    p1 = X.conv2d_wgrad_plan(dy1, x, K, K, 1, 1, PAD, PAD, 1, 1)
    same = pg['kernel'] == p1['kernel'] and pg['S'] == p1['S']
    print('plan grouped', dict(pg), 'single', dict(p1))
    for g in range(G):
        yr, dwr, dbr = ref[g]
        e = (ys[g].float() - yr).abs().max().item()
        print('group', g, 'y err', e, 'ref max', yr.abs().max().item())
        assert e <= 1e-2 * max(1.0, yr.abs().max().item()), (g, e)
        for got, one, r, name in ((ws[g].grad, ws1[g].grad, dwr, 'dw'),
                                  (bs[g].grad, bs1[g].grad, dbr, 'db')):
            e = (got.float() - r).abs().max().item()
            e1 = (got.float() - one.float()).abs().max().item()
            print('group', g, name, 'err vs fp32', e, 'vs one-by-one', e1, 'ref max',
                  r.abs().max().item())
            assert got.shape == r.shape
            assert e <= 2e-2 * max(1.0, r.abs().max().item()), (g, name, e)
            if same or name == 'db':
                assert torch.equal(got, one), (g, name, e1)
            else:
                assert e1 <= 2e-2 * max(1.0, r.abs().max().item()), (g, name, e1)


def test_plain_members(small_grids):
    """Members without spectral norm (fp32 parameters under bf16 autocast, no sigma): outputs
    and bias gradients equal the layers alone bit for bit (the same split at this shape), weight
    gradients too where the k11 plan is the same, else at the fp32 tolerance."""
    C = small_grids
    from imaginaire_amd.ops import _ext
    X = _ext.ext()
    shape = SHAPES[1]
    x, groups = _data(shape)
    C.mark_zero_tail(x, CIN)

    def run(grouped):
        ws = [torch.nn.Parameter(g[0].clone()) for g in groups]
        bs = [torch.nn.Parameter(g[3].clone()) for g in groups]
        with torch.autocast('cuda', dtype=BF), _conv_log(C):
            if grouped:
                ys = C.conv2d_act_group(x, ws, bs, 1, PAD, 1, 0.0)
            else:
                ys = [C.conv2d_act(x, w, b, 1, PAD, 1, 0.0) for w, b in zip(ws, bs)]
            torch.autograd.backward(ys, [g[4] for g in groups])
            rows = C.conv_log_summary()
        return ys, ws, bs, rows

    ys, ws, bs, rows = run(True)
    ys1, ws1, bs1, rows1 = run(False)
    assert _label_rows(rows, 'fwd') == {'k10g': 1} and _label_rows(rows, 'wgrad') == {'k11g': 1}
    assert _label_rows(rows1, 'fwd') == {'k10': G} and _label_rows(rows1, 'wgrad') == {'k11': G}
    B, H, W = shape
    dyg = torch.empty(B, G * COUT, H, W, device='cuda', dtype=BF).contiguous(memory_format=CL)
    dy1 = torch.empty(B, COUT, H, W, device='cuda', dtype=BF).contiguous(memory_format=CL)
    pg = X.conv2d_wgrad_plan(dyg, x, K, K, 1, 1, PAD, PAD, 1, 1)
    p1 = X.conv2d_wgrad_plan(dy1, x, K, K, 1, 1, PAD, PAD, 1, 1)
    same = pg['kernel'] == p1['kernel'] and pg['S'] == p1['S']
    for g in range(G):
        assert torch.equal(ys[g], ys1[g]) and torch.equal(bs[g].grad, bs1[g].grad), g
        assert ws[g].grad.shape == (COUT, CIN, K, K)
        e = (ws[g].grad - ws1[g].grad).abs().max().item()
        print('group', g, 'dw vs one-by-one', e, 'same plan', same)
        if same:
            assert torch.equal(ws[g].grad, ws1[g].grad), (g, e)
        else:
            assert e <= 2e-2 * max(1.0, ws1[g].grad.abs().max().item()), (g, e)


def test_missing_gradient(small_grids):
    """A group whose output receives no gradient gets None; the others get what the layers
    alone get."""
    C = small_grids
    shape = SHAPES[1]
    _, groups = _data(shape)
    x, ws, bs, sws = _members(C, shape)
    ys = C.conv2d_act_group(x, sws, bs, 1, PAD, 1, 0.0)
    torch.autograd.backward([ys[0], ys[2]], [groups[0][4], groups[2][4]])
    x1, ws1, bs1, sws1 = _members(C, shape)
    ys1 = [C.conv2d_act(x1, sw, b, 1, PAD, 1, 0.0) for sw, b in zip(sws1, bs1)]
    torch.autograd.backward([ys1[0], ys1[2]], [groups[0][4], groups[2][4]])
    assert ws[1].grad is None and bs[1].grad is None
    for g in (0, 2):
        assert torch.equal(ws[g].grad, ws1[g].grad) and torch.equal(bs[g].grad, bs1[g].grad), g


def test_fallback_shape(small_grids):
    """1 x 8 x 24 is a shape the v4 tile refuses: the native entry declines and the Python path
    gives the one-by-one results bitwise."""
    C = small_grids
    from imaginaire_amd.ops import _ext
    shape = (1, 8, 24)
    _, groups = _data(shape)
    x, ws, bs, sws = _members(C, shape)
    assert _ext.ext().conv2d_mfma_grouped(
        x, [sw.shadow.new_zeros(COUT, CINP, K, K).contiguous(memory_format=CL) for sw in sws],
        [], [], PAD, PAD, 0.0) == []
    with _conv_log(C):
        ys = C.conv2d_act_group(x, sws, bs, 1, PAD, 1, 0.0)
        torch.autograd.backward(ys, [g[4] for g in groups])
        rows = C.conv_log_summary()
    assert 'k10g' not in _label_rows(rows, 'fwd') and 'k11g' not in _label_rows(rows, 'wgrad')
    x1, ws1, bs1, sws1 = _members(C, shape)
    ys1 = [C.conv2d_act(x1, sw, b, 1, PAD, 1, 0.0) for sw, b in zip(sws1, bs1)]
    torch.autograd.backward(ys1, [g[4] for g in groups])
    for g in range(G):
        assert torch.equal(ys[g], ys1[g]), g
        assert torch.equal(ws[g].grad, ws1[g].grad) and torch.equal(bs[g].grad, bs1[g].grad), g


# ---- module level ---------------------------------------------------------------------------

class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from imaginaire_amd.layers.activation_norm import SpatiallyAdaptiveNorm
        self.norms = torch.nn.ModuleList(
            SpatiallyAdaptiveNorm(64, CIN, num_filters=COUT, kernel_size=K,
                                  weight_norm_type='spectral', separate_projection=True)
            for _ in range(G))

    def forward(self, x, label, cache=True):
        from imaginaire_amd.layers.activation_norm import LabelMapCache
        with LabelMapCache() if cache else contextlib.nullcontext():
            for n in self.norms:
                x = n(x, label)
        return x


def _net():
    from imaginaire_amd.layers import spectral_norm as snm
    torch.manual_seed(11)
    net = _Net().cuda().to(memory_format=CL)
    assert snm.install_batched_spectral_norm(net) == 3 * G
    return net


def _inputs():
    torch.manual_seed(12)
    x = torch.randn(2, 64, 16, 32, device='cuda').contiguous(memory_format=CL)
    label = torch.randn(2, CIN, 16, 32, device='cuda').contiguous(memory_format=CL)
    go = torch.randn(2, 64, 16, 32, device='cuda').contiguous(memory_format=CL)
    return x, label, go


def _step(net, x, label, go, cache=True):
    xi = x.clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    with torch.autocast('cuda', dtype=BF):
        y = net(xi, label, cache)
    y.backward(go.to(y.dtype))
    out = {'y': y.detach().clone(), 'dx': xi.grad.clone()}
    out.update({'grad.' + n: p.grad.clone() for n, p in net.named_parameters()
                if p.grad is not None})
    out.update({'buf.' + n: b.clone() for n, b in net.named_buffers()
                if n.endswith(('weight_u', 'weight_v'))})
    return out


@pytest.fixture
def sn_fused(monkeypatch):
    from imaginaire_amd.layers import spectral_norm as snm
    monkeypatch.setattr(snm, '_SN_SHADOW', True)
    monkeypatch.setattr(snm, '_SN_FUSED', True)


def _two_steps(C, monkeypatch, switch, cache=True):
    """A fresh net, one step that learns the members, then the measured step with its conv log."""
    monkeypatch.setenv('IMAGINAIRE_AMD_SPADE_GROUP', switch)
    net = _net()
    x, label, go = _inputs()
    _step(net, x, label, go, cache)
    with _conv_log(C):
        out = _step(net, x, label, go, cache)
        rows = C.conv_log_summary()
    return out, rows


@pytest.mark.parametrize('split', ['2', None])
def test_module_switch_on_equals_off(small_grids, sn_fused, monkeypatch, split):
    """Three SPADE norms on one label map: outputs, dx, every parameter gradient and every
    u / v with the switch on against off — u / v bitwise always, the rest bitwise with the split
    pinned and at the fp32-reference tolerance otherwise; 1 grouped forward and 1 grouped weight
    gradient where the switch-off run shows 3 of each."""
    C = small_grids
    if split is not None:
        monkeypatch.setenv('IMAGINAIRE_AMD_CONV_SPLITK', split)
    on, rows_on = _two_steps(C, monkeypatch, '1')
    off, rows_off = _two_steps(C, monkeypatch, '0')
    assert _label_rows(rows_on, 'fwd') == {'k10g': 1}, rows_on
    assert _label_rows(rows_on, 'wgrad') == {'k11g': 1}, rows_on
    assert _label_rows(rows_off, 'fwd') == {'k10': G}, rows_off
    assert _label_rows(rows_off, 'wgrad') == {'k11': G}, rows_off
    assert on.keys() == off.keys()
    for name in on:
        a, b = on[name], off[name]
        e = (a.float() - b.float()).abs().max().item()
        print(name, 'max diff', e, 'max', b.float().abs().max().item())
        if name.startswith('buf.') or split is not None:
            assert torch.equal(a, b), (name, e)
        else:
            assert e <= 2e-2 * max(1.0, b.float().abs().max().item()), (name, e)


def test_module_without_cache_is_per_layer(small_grids, sn_fused, monkeypatch):
    """No active cache: the switch changes nothing, bit for bit, and nothing is grouped."""
    C = small_grids
    on, rows_on = _two_steps(C, monkeypatch, '1', cache=False)
    off, _ = _two_steps(C, monkeypatch, '0', cache=False)
    assert _label_rows(rows_on, 'fwd') == {'k10': G} and \
        _label_rows(rows_on, 'wgrad') == {'k11': G}, rows_on
    diff = {name: (on[name].float() - off[name].float()).abs().max().item()
            for name in on if not torch.equal(on[name], off[name])}
    assert not diff, diff


def test_module_graph_replay(small_grids, sn_fused, monkeypatch):
    """Forward + backward with the grouped launches captured after warm-up: two replays equal
    the eager result (u / v put back before each run)."""
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.utils.cuda_graph import graph_routing
    C = small_grids
    monkeypatch.setenv('IMAGINAIRE_AMD_SPADE_GROUP', '1')
    net = _net()
    x, label, go = _inputs()
    xi = x.clone().requires_grad_(True)
    params = [p for p in net.parameters() if p.requires_grad]
    seen = []
    orig = C._run_group
    monkeypatch.setattr(C, '_run_group', lambda *a: (seen.append(len(a[1])), orig(*a))[1])

    def step():
        with torch.autocast('cuda', dtype=BF):
            y = net(xi, label)
        gr = torch.autograd.grad(y, [xi] + params, go.to(y.dtype), allow_unused=True)
        return (y,) + tuple(t for t in gr if t is not None)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with graph_routing(), torch.cuda.stream(s):
        for _ in range(2):
            step()
        snap = {n: b.clone() for n, b in net.named_buffers()}

        def restore():
            with torch.no_grad():
                for n, b in net.named_buffers():
                    b.copy_(snap[n])
        restore()
        eager = [t.clone() for t in step()]
        restore()
        del seen[:]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            outs = step()
        assert seen == [G]
        _ext.ext().flush_deferred_uploads()
        for _ in range(2):
            restore()
            graph.replay()
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(outs, eager)):
                assert torch.equal(a, b), i
    torch.cuda.current_stream().wait_stream(s)
