"""bench.py ``--dump-outputs``: the files hold the last step's losses and a fixed sample of the
updated network state, as float64 / float32 ``.npy``, identical from call to call and bounded
in size whatever the networks' size; the seeded state that the dumped step starts from is put
back completely. ``--full`` is accepted."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _trainer():
    torch.manual_seed(0)
    net_G = torch.nn.Sequential(torch.nn.Conv2d(3, 64, 5), torch.nn.BatchNorm2d(64),
                                torch.nn.Linear(300, 700))
    net_G[0].weight.data = net_G[0].weight.data.contiguous(memory_format=torch.channels_last)
    net_D = torch.nn.Linear(5, 7)
    return types.SimpleNamespace(
        net_G=net_G, net_D=net_D,
        gen_losses={'total': torch.tensor(2.5), 'GAN': torch.tensor(0.5), 'note': 'x'},
        dis_losses={'total': torch.tensor(1.25)})


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_files(tmp_path):
    t = _trainer()
    bench._dump_outputs(t, str(tmp_path / 'a'))
    bench._dump_outputs(t, str(tmp_path / 'b'))
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sorted(a) == ['dis_losses', 'gen_losses', 'net_D_state', 'net_G_state']
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].ndim == 1
        assert np.array_equal(a[k], b[k]), k
    assert a['gen_losses'].tolist() == [0.5, 2.5]  # sorted keys: GAN, total
    assert a['dis_losses'].tolist() == [1.25]
    # small tensors whole, in key order
    assert np.array_equal(a['net_D_state'], np.concatenate(
        [t.net_D.bias.detach().numpy(), t.net_D.weight.detach().numpy().ravel()]))
    # tensors above the cap (the 300x700 weight, the 64x3x5x5 conv weight) are sampled; integer
    # buffers (num_batches_tracked) are left out
    state = t.net_G.state_dict()
    want = sum(min(v.numel(), 4096) for v in state.values() if v.is_floating_point())
    assert a['net_G_state'].size == want
    # a changed weight shows, whatever its memory format
    with torch.no_grad():
        t.net_G[0].weight.add_(1.0)
        t.net_G[2].weight.add_(1.0)
    bench._dump_outputs(t, str(tmp_path / 'c'))
    c = _load(str(tmp_path / 'c'))
    assert int((c['net_G_state'] != a['net_G_state']).sum()) == 4096 + 4096


def test_dump_is_bounded():
    class Many(object):
        def state_dict(self):
            return {'p%05d' % i: torch.zeros(1000) for i in range(20000)}
    s = bench._state_sample(Many(), torch.Generator().manual_seed(0))
    assert s.dtype == np.float32 and s.nbytes <= bench.DUMP_BYTES_PER_NET
    assert 2 * bench.DUMP_BYTES_PER_NET < 64 * 10 ** 6


def test_seeded_restore_repeats_the_first_step():
    """After ``_Seeded.restore()`` a step repeats the first one bit for bit: weights, BatchNorm
    statistics, Adam moments and step counters, the random generator and the batch source's
    position are all back, and the optimizer's state tensors are still the same storage."""
    from imaginaire_amd.optimizers.fused_adam import FusedAdam
    torch.manual_seed(3)
    net_G = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5))
    net_D = torch.nn.Linear(5, 1)
    t = types.SimpleNamespace(net_G=net_G, net_D=net_D,
                              opt_G=FusedAdam(net_G.parameters(), lr=1e-2),
                              opt_D=FusedAdam(net_D.parameters(), lr=1e-2))
    src = types.SimpleNamespace(step=0)
    seeded = bench._Seeded(t, src, torch.device('cpu'))

    def one():
        x = torch.randn(8, 6)
        src.step += 8
        loss = net_D(net_G(x)).pow(2).mean()
        for o in (t.opt_G, t.opt_D):
            o.zero_grad()
        loss.backward()
        for o in (t.opt_G, t.opt_D):
            o.step()
        state = {n + k: v.clone() for n, net in (('G.', net_G), ('D.', net_D))
                 for k, v in net.state_dict().items()}
        return loss.detach().clone(), state

    first = one()
    one()
    one()
    moment = t.opt_G.state[net_G[0].weight]['exp_avg']
    seeded.restore()
    assert src.step == 0 and t.opt_G.param_groups[0]['step'] == 0
    assert t.opt_G.state[net_G[0].weight]['exp_avg'] is moment and float(moment.abs().sum()) == 0
    again = one()
    assert torch.equal(first[0], again[0])
    assert first[1].keys() == again[1].keys()
    for k in first[1]:
        assert torch.equal(first[1][k], again[1][k]), k


def test_full_and_dump_options_parse(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '2'])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == 'out'
