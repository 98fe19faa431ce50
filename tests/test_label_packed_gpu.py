"""Packed label maps on the GPU: the k19 kernel (``csrc/label.hip``) against the PyTorch
reference of ``ops.label``, the packed branch of ``LabelMapCache.resize`` against its
pad-then-resize path, and a SPADE iteration (eager and captured) with ``data.packed_labels``.

Comparisons are bitwise (values, dtype, shape, strides): the tensors hold zeros, ones and
copied values. Shapes are the smallest that reach every path of the kernel: an odd 5 x 7 source
(pieces run across row and pixel ends, the tensor ends in a scalar tail), channel counts that
are no multiple of the 4- / 8-element piece, a one-hot segment across a 64-channel boundary."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, H, W = 2, 5, 7
SIZES = [None, (5, 7), (10, 14), (3, 4), (2, 3)]  # none, same, exact 2x, non-integer, down


def _layouts():
    g = torch.Generator().manual_seed(0)
    # A: 6 + 1 + 70 + 2 = 79 channels; the 70-label segment spans channels 7 .. 76
    a_idx = torch.stack([torch.randint(0, 6, (B, H, W), generator=g),
                         torch.randint(0, 71, (B, H, W), generator=g)], 1)
    a_idx[0, 0, 0, 0], a_idx[1, 0, 4, 6] = 5, 5      # n with a don't-care channel
    a_idx[0, 1, 0, 1], a_idx[1, 1, 4, 6] = 70, 70    # n without one: no channel set
    a_idx[0, 1, 2, 3], a_idx[1, 1, 0, 0] = 0, 69
    b_idx = torch.randint(0, 301, (B, 1, H, W), generator=g)
    b_idx[0, 0, 0, 0], b_idx[1, 0, 4, 6], b_idx[0, 0, 1, 1] = 300, 299, 256
    return {
        'A': (a_idx.to(torch.uint8), torch.rand(B, 3, H, W, generator=g),
              [('seg', 'index', 6, 5, True), ('edge', 'dense', 1, 0, False),
               ('parts', 'index', 70, 70, False), ('flow', 'dense', 2, 0, False)]),
        'B': (b_idx.to(torch.int16), None, [('seg', 'index', 301, 300, True)]),
        'C': (None, torch.rand(B, 3, H, W, generator=g), [('maps', 'dense', 3, 0, False)]),
    }


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride() and \
        torch.equal(a, b)


def _dev(t):
    return None if t is None else t.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_expand_labels_matches_reference(name, dtype, channels_last):
    from imaginaire_amd.ops.label import expand_labels, layout_channels
    idx, dense, layout = _layouts()[name]
    c = layout_channels(layout)
    assert c == {'A': 79, 'B': 301, 'C': 3}[name]
    for size in SIZES:
        for pad_to in (None, (c + 63) // 64 * 64):
            kw = dict(size=size, pad_to=pad_to, dtype=dtype, channels_last=channels_last)
            want = expand_labels(idx, dense, layout, **kw)  # CPU tensors: the reference
            got = expand_labels(_dev(idx), _dev(dense), layout, **kw)
            assert got.is_cuda and _same(got.cpu(), want), (name, kw)
            assert want.shape == (B, pad_to or c) + (size or (H, W))


@pytest.mark.gpu
def test_expand_labels_video_and_errors():
    from imaginaire_amd.ops.label import expand_labels
    idx, dense, layout = _layouts()['A']
    idx5 = torch.stack([idx, idx.flip(0), idx.flip(3)], 1)        # [B, T = 3, K, H, W]
    dense5 = torch.stack([dense, dense.flip(2), dense * 0.5], 1)
    want = expand_labels(idx5, dense5, layout, size=(3, 4), pad_to=128)
    got = expand_labels(idx5.cuda(), dense5.cuda(), layout, size=(3, 4), pad_to=128)
    assert want.shape == (B, 3, 128, 3, 4) and _same(got.cpu(), want)
    with pytest.raises(RuntimeError, match='not differentiable'):
        expand_labels(idx.cuda(), dense.cuda().requires_grad_(), layout)
    with pytest.raises(ValueError):
        expand_labels(idx5.cuda(), dense5.cuda(), layout, channels_last=True)


def _packed_label(dtype):
    """A channels-last label as the trainer delivers it: 184 classes + don't care + edge map,
    186 channels (above 64 and no multiple of 64: the conv consumers ask for the padded map)."""
    from imaginaire_amd.ops.label import cast_label, expand_packed_labels
    g = torch.Generator().manual_seed(1)
    layout = [('seg_maps', 'index', 185, 184, True), ('edge_maps', 'dense', 1, 0, False)]
    idx = torch.randint(0, 185, (2, 1, 8, 12), generator=g).to(torch.uint8)
    data = {'label_idx': idx.cuda(), 'label_dense': torch.rand(2, 1, 8, 12, generator=g).cuda()}
    label = expand_packed_labels(data, layout, channels_last=True)['label']
    assert label.shape == (2, 186, 8, 12) and label.dtype == torch.float32
    assert label.is_contiguous(memory_format=torch.channels_last)
    return cast_label(label, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_label_map_cache_resize(monkeypatch, dtype):
    from imaginaire_amd.layers.activation_norm import LabelMapCache
    from imaginaire_amd.ops import label as label_ops
    label = _packed_label(dtype)
    assert getattr(label, '_iamd_packed_label', None) is not None
    calls = []
    real = label_ops.expand_labels

    def spy(*args, **kwargs):
        calls.append(kwargs.get('size'))
        return real(*args, **kwargs)
    monkeypatch.setattr(label_ops, 'expand_labels', spy)
    for size in [(8, 12), (16, 24), (3, 5)]:
        for conv_pad in (True, False):
            if size == (8, 12) and not conv_pad:
                continue  # the label itself is returned
            monkeypatch.setenv('IMAGINAIRE_AMD_LABEL_PACKED_RESIZE', '0')
            n = len(calls)
            off = LabelMapCache.resize(label, size, conv_pad=conv_pad)
            assert len(calls) == n
            monkeypatch.setenv('IMAGINAIRE_AMD_LABEL_PACKED_RESIZE', '1')
            on = LabelMapCache.resize(label, size, conv_pad=conv_pad)
            assert calls[n:] == [size]
            assert _same(on, off), (size, conv_pad)
            assert getattr(on, '_iamd_valid_channels', None) == \
                getattr(off, '_iamd_valid_channels', None) == (186 if conv_pad else None)
            assert on.shape[1] == (192 if conv_pad else 186)
            # a modified label is a new tensor without the packed source: today's path
            n = len(calls)
            mod = LabelMapCache.resize(label * 1, size, conv_pad=conv_pad)
            assert len(calls) == n and _same(mod, off)
    # the per-forward cache serves the packed result under the usual key
    with LabelMapCache():
        n = len(calls)
        first = LabelMapCache.resize(label, (4, 6), conv_pad=True)
        assert LabelMapCache.resize(label, (4, 6), conv_pad=True) is first
        assert len(calls) == n + 1


def _trainer(tmp, packed, seed=0):
    from imaginaire_amd.config import Config
    from imaginaire_amd.utils.dataset import get_train_and_val_dataloader
    from imaginaire_amd.utils.trainer import get_model_optimizer_and_scheduler, get_trainer
    torch.manual_seed(0)
    cfg = Config(os.path.join(ROOT, 'configs', 'unit_test', 'spade.yaml'))
    cfg.speed_benchmark = False
    cfg.logdir = str(tmp)
    if packed:
        cfg.data.packed_labels = True
    loaders = get_train_and_val_dataloader(cfg)
    nets = get_model_optimizer_and_scheduler(cfg, seed=seed)
    tr = get_trainer(cfg, *nets, *loaders)
    tr.net_G_module.style_encoder.freeze_random = True
    return tr


def _batch(tr, i):
    from torch.utils.data import default_collate
    ds = tr.train_data_loader.dataset
    return default_collate([ds[(2 * i) % len(ds)], ds[(2 * i + 1) % len(ds)]])


@pytest.mark.gpu
def test_spade_iteration_packed_equals_unpacked(tmp_path, monkeypatch):
    """Same seed, flag off and on, deterministic kernels (as tests/test_determinism_gpu.py):
    equal ``label`` out of ``start_of_iteration`` and bitwise equal losses after one D and
    one G update; the packed run takes the packed branch of ``LabelMapCache.resize``."""
    from imaginaire_amd.ops import label as label_ops
    sized = []
    real = label_ops.expand_labels

    def spy(*args, **kwargs):
        sized.append(kwargs.get('size'))
        return real(*args, **kwargs)
    monkeypatch.setattr(label_ops, 'expand_labels', spy)
    prev = torch.are_deterministic_algorithms_enabled()
    prev_cudnn = torch.backends.cudnn.deterministic
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic = True
    out = {}
    try:
        for packed in (False, True):
            tr = _trainer(tmp_path / str(packed), packed, seed=7)
            batch = _batch(tr, 0)
            assert ('label_idx' in batch) == packed and ('label' in batch) != packed
            torch.manual_seed(11)
            d = tr.start_of_iteration(batch, 0)
            assert 'label_idx' not in d and 'label_dense' not in d
            before = len([s for s in sized if s is not None])
            tr.dis_update(d)
            tr.gen_update(d)
            torch.cuda.synchronize()
            resized = len([s for s in sized if s is not None]) - before
            assert (resized > 0) == packed
            losses = {'G/' + k: v.detach().float().cpu() for k, v in tr.gen_losses.items()}
            losses.update({'D/' + k: v.detach().float().cpu()
                           for k, v in tr.dis_losses.items()})
            out[packed] = (d, losses)
    finally:
        torch.use_deterministic_algorithms(prev)
        torch.backends.cudnn.deterministic = prev_cudnn
    (d0, l0), (d1, l1) = out[False], out[True]
    assert sorted(d0) == sorted(d1)
    assert _same(d0['label'].cpu(), d1['label'].cpu())
    assert d0['label'].stride() == d1['label'].stride()
    assert _same(d0['images'].cpu(), d1['images'].cpu())
    assert l0.keys() == l1.keys()
    for k in l0:
        print(k, float(l0[k]), float(l1[k]))
        assert torch.equal(l0[k], l1[k]), (k, l0[k], l1[k])


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [False, True])
def test_graph_replay_matches_eager(tmp_path, packed):
    """The captured iteration fed by the (packed) loader replays and follows an eager step from
    the same state, to the tolerances of tests/test_graph_gpu.py (the step is not reproducible
    run to run outside deterministic mode: atomics, Adam with beta1 = 0)."""
    from imaginaire_amd.utils.cuda_graph import make_trainer_step
    n = 4
    torch.cuda.set_device(0)
    tr = _trainer(tmp_path, packed)
    step, graphed = make_trainer_step(tr, warmup=2, enabled=True)
    assert graphed is not None
    for i in range(n):
        torch.manual_seed(1)
        step(tr.start_of_iteration(_batch(tr, i), i))
    torch.cuda.synchronize()
    assert graphed.graph is not None and not graphed.failed, 'step was not captured'
    state = [t for net in (tr.net_G, tr.net_D) for t in
             list(net.parameters()) + list(net.buffers())]
    for o in (tr.opt_G, tr.opt_D):
        for st in o.state.values():
            state += [v for v in st.values() if torch.is_tensor(v)]
        state += [g['_hyper'] for g in o.param_groups if '_hyper' in g]
    saved = [t.detach().clone() for t in state]
    gparams = list(tr.net_G.parameters())
    d = tr.start_of_iteration(_batch(tr, n), n)
    assert 'label_idx' not in d and d['label'].dim() == 4
    graphed(d)  # replay
    torch.cuda.synchronize()
    lg = (float(tr.dis_losses['total']), float(tr.gen_losses['total']))
    gg = [None if p.grad is None else p.grad.detach().float().clone() for p in gparams]
    with torch.no_grad():
        for t, c in zip(state, saved):
            t.copy_(c)
    torch.cuda.synchronize()
    graphed.step_fn(d)  # the same iteration, eagerly, from the same state
    torch.cuda.synchronize()
    le = (float(tr.dis_losses['total']), float(tr.gen_losses['total']))
    ge = [None if p.grad is None else p.grad.detach().float() for p in gparams]
    print('packed', packed, 'graph', lg, 'eager', le)
    assert all(x == x for x in lg + le)
    assert abs(lg[0] - le[0]) <= 1e-3 * max(1.0, abs(le[0])), (lg, le)
    assert abs(lg[1] - le[1]) <= 1e-3 * max(1.0, abs(le[1])), (lg, le)
    gnum = sum(float((x - y).pow(2).sum()) for x, y in zip(gg, ge) if x is not None)
    gden = sum(float(y.pow(2).sum()) for x, y in zip(gg, ge) if x is not None)
    assert gden > 0 and gnum <= 1e-4 * gden, (gnum, gden)
