"""The grouping logic of the SPADE label convs without a GPU: which convs
``ops.conv.conv2d_act_group`` hands to the grouped executor, and how ``LabelMapCache`` learns the
members of a resolution on one forward, verifies them on the next and hands out the hidden maps.
The native entry is replaced by a stub that records its calls and runs the one-by-one
reference."""
import pytest
import torch
import torch.nn.functional as F


# ---- conv2d_act_group: what is grouped ------------------------------------------------------

@pytest.fixture
def stubbed(monkeypatch):
    """ops.conv with the planner answering 'k10' for every conv, ``_run`` replaced by an fp32
    reference and ``_run_group`` by a recorder that runs the same reference per member."""
    from imaginaire_amd.ops import conv as C
    calls = {'group': [], 'single': 0}

    def plain(w):
        return w.W / w.sigma if isinstance(w, C.SNWeight) else w

    def ref(x, w, b, pd, slope):
        y = F.conv2d(x, w, b, 1, pd)
        return torch.where(y > 0, y, y * slope)

    def route(x, weight, stride, padding, dilation, groups=1, padding_mode='zeros',
              residual=None, slope=1.0):
        return C.Route('k10', 0, False, False, isinstance(weight, C.SNWeight), False, 0)

    def run(r, x, weight, bias, stride, padding, dilation, groups, padding_mode, residual, slope):
        calls['single'] += 1
        return ref(x, plain(weight), bias, padding, slope)

    def run_group(x, ws, sws, bs, padding, slope):
        calls['group'].append(len(ws))
        return [ref(x, w if sw is None else plain(sw), bs[g] if bs else None, padding, slope)
                for g, (w, sw) in enumerate(zip(ws, sws))]

    monkeypatch.setattr(C, '_route', route)
    monkeypatch.setattr(C, '_run', run)
    monkeypatch.setattr(C, '_run_group', run_group)
    monkeypatch.delenv('IMAGINAIRE_AMD_SPADE_GROUP', raising=False)
    return C, calls


def _sn(C, cout=128, cin=8, k=3):
    w = torch.randn(cout, cin, k, k)
    return C.SNWeight(torch.nn.Parameter(w), w.to(torch.bfloat16), torch.randn(cout),
                      torch.randn(cin * k * k), torch.tensor(1.5), None, None)


def test_group_of_sn_members(stubbed):
    C, calls = stubbed
    torch.manual_seed(0)
    x = torch.randn(1, 8, 6, 6)
    ws = [_sn(C) for _ in range(3)]
    bs = [torch.randn(128) for _ in range(3)]
    ys = C.conv2d_act_group(x, ws, bs, 1, 1, 1, 0.0)
    assert calls == {'group': [3], 'single': 0}
    for y, w, b in zip(ys, ws, bs):
        assert torch.equal(y, F.relu(F.conv2d(x, w.W / w.sigma, b, 1, 1)))


def test_plain_members_are_grouped_too(stubbed):
    C, calls = stubbed
    x = torch.randn(1, 8, 6, 6)
    C.conv2d_act_group(x, [torch.randn(128, 8, 3, 3) for _ in range(2)], [None, None], 1, 1, 1, 0.2)
    assert calls == {'group': [2], 'single': 0}


@pytest.mark.parametrize('case', ['mixed', 'switch', 'shape', 'cout', 'bias', 'stride', 'one',
                                  'x_grad'])
def test_not_grouped(stubbed, monkeypatch, case):
    """Mixed SN / plain members, the switch, unequal shapes, Cout off the 128 tile, a missing
    bias, a stride, a single member or an input that needs a gradient: one by one."""
    C, calls = stubbed
    x = torch.randn(1, 8, 6, 6)
    ws = [_sn(C), _sn(C), _sn(C)]
    bs = [torch.randn(128) for _ in range(3)]
    stride = 1
    if case == 'mixed':
        ws[1] = torch.randn(128, 8, 3, 3)
    elif case == 'switch':
        monkeypatch.setenv('IMAGINAIRE_AMD_SPADE_GROUP', '0')
    elif case == 'shape':
        ws[2] = _sn(C, k=5)
    elif case == 'cout':
        ws, bs = [_sn(C, cout=64) for _ in range(3)], [torch.randn(64) for _ in range(3)]
    elif case == 'bias':
        bs[0] = None
    elif case == 'stride':
        stride = 2
    elif case == 'one':
        ws, bs = ws[:1], bs[:1]
    elif case == 'x_grad':
        x.requires_grad_(True)
    if case == 'shape':  # (the reference conv pads by 1: give the 5 x 5 member room)
        x = torch.randn(1, 8, 8, 8)
    if case == 'stride':
        monkeypatch.setattr(C, '_run', lambda r, x, w, b, st, *a: (
            calls.__setitem__('single', calls['single'] + 1), st)[1])
    C.conv2d_act_group(x, ws, bs, stride, 1, 1, 0.0)
    assert calls['group'] == [] and calls['single'] == len(ws)


# ---- LabelMapCache: membership --------------------------------------------------------------

class _Net(torch.nn.Module):
    def __init__(self, n=3, twice=False, weight_norm_type='spectral'):
        super().__init__()
        from imaginaire_amd.layers.activation_norm import SpatiallyAdaptiveNorm
        self.twice = twice
        self.norms = torch.nn.ModuleList(
            SpatiallyAdaptiveNorm(8, 5, num_filters=16, kernel_size=3,
                                  weight_norm_type=weight_norm_type, separate_projection=True,
                                  activation_norm_type='instance') for _ in range(n))

    def forward(self, x, label, cache=True):
        import contextlib
        from imaginaire_amd.layers.activation_norm import LabelMapCache
        with LabelMapCache() if cache else contextlib.nullcontext():
            for i, n in enumerate(self.norms):
                x = n(x, label)
                if self.twice and i == 0:
                    x = n(x, label)
        return x


@pytest.fixture
def recorded(monkeypatch):
    """``conv2d_act_group`` replaced by a recorder that runs ``conv2d_act`` per member."""
    from imaginaire_amd.ops import conv as C
    groups = []

    def group(x, weights, biases, stride=1, padding=0, dilation=1, slope=1.0):
        groups.append(len(weights))
        return [C.conv2d_act(x, w, b, stride, padding, dilation, slope)
                for w, b in zip(weights, biases)]

    monkeypatch.setattr(C, 'conv2d_act_group', group)
    monkeypatch.delenv('IMAGINAIRE_AMD_SPADE_GROUP', raising=False)
    return groups


def _inputs():
    torch.manual_seed(3)
    return torch.randn(2, 8, 6, 10), torch.randn(2, 5, 6, 10), torch.randn(2, 8, 6, 10)


def _step(net, cache=True):
    x, label, go = _inputs()
    x.requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    y = net(x, label, cache)
    y.backward(go)
    out = {'y': y.detach().clone(), 'dx': x.grad.clone()}
    out.update({'grad.' + n: p.grad.clone() for n, p in net.named_parameters()
                if p.grad is not None})
    out.update({'buf.' + n: b.clone() for n, b in net.named_buffers()})
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize('twice', [False, True])
def test_members_learned_then_grouped(recorded, monkeypatch, twice):
    """The first forward learns who reads the label map, the second computes their hidden maps
    in one grouped call (a module called twice takes part once, its second call runs alone);
    outputs, gradients and the spectral-norm buffers equal the ungrouped module's."""
    torch.manual_seed(1)
    net = _Net(twice=twice)
    torch.manual_seed(1)
    ref = _Net(twice=twice)
    first = _step(net)
    assert recorded == []
    members = net.norms[0]._label_groups[(0, (6, 10))]
    assert [m for m, _ in members] == list(net.norms) and all(i == 0 for _, i in members)
    second = _step(net)
    assert recorded == [3]
    monkeypatch.setenv('IMAGINAIRE_AMD_SPADE_GROUP', '0')
    _same(first, _step(ref))
    _same(second, _step(ref))
    assert recorded == [3]


def test_members_verified_at_use(recorded):
    """A member that no longer agrees with the first layer: nothing is grouped on that forward
    (every layer runs alone, with the right result), and the next one groups those that agree."""
    torch.manual_seed(1)
    net = _Net()
    torch.manual_seed(1)
    ref = _Net()
    _step(net)
    _step(ref, cache=False)
    for n in (net, ref):  # the third layer's MLP now ends in another activation
        n.norms[2].mlps[0][0].layers['nonlinearity'] = torch.nn.LeakyReLU(0.2)
    _same(_step(net), _step(ref, cache=False))
    assert recorded == []
    assert [m for m, _ in net.norms[0]._label_groups[(0, (6, 10))]] == list(net.norms[:2])
    _step(net)
    assert recorded == [2]


def test_no_cache_no_group(recorded):
    torch.manual_seed(1)
    net = _Net()
    _step(net, cache=False)
    _step(net, cache=False)
    assert recorded == [] and net.norms[0]._label_groups == {}


def test_plain_and_sn_layers_never_share_a_group(stubbed):
    """Two norms with spectral norm and one without on one label map: their first convs agree
    in shape, so the cache asks for one group, and conv2d_act_group runs them one by one."""
    C, calls = stubbed
    from imaginaire_amd.layers.activation_norm import SpatiallyAdaptiveNorm
    torch.manual_seed(1)
    net = _Net()
    net.norms[1] = SpatiallyAdaptiveNorm(8, 5, num_filters=16, kernel_size=3,
                                         weight_norm_type='', separate_projection=True,
                                         activation_norm_type='instance')
    seen = []
    orig = C.conv2d_act_group

    def spy(x, weights, *a, **k):
        seen.append([isinstance(w, C.SNWeight) for w in weights])
        return orig(x, weights, *a, **k)
    C.conv2d_act_group = spy
    try:
        x, label, _ = _inputs()
        sn = _sn(C, 16, 5, 3)
        from imaginaire_amd.layers import conv as LC
        real = LC._plain_conv_weight
        # (off the GPU no layer hands out an SNWeight: stand one in for the spectral-norm layers)
        LC._plain_conv_weight = lambda c: sn if hasattr(c, 'weight_orig') else real(c)
        try:
            with torch.no_grad():
                net(x, label)
                net(x, label)
        finally:
            LC._plain_conv_weight = real
    finally:
        C.conv2d_act_group = orig
    assert seen == [[True, False, True]] and calls['group'] == []
