"""World-consistent vid2vid runs its training iteration as a replayed hipGraph (GPU).

Its guidance renderer kept the point cloud, the frame's point list and the rendered image on
the host, so the trainer was not capturable. With ops/splat.py the cloud is device state of
fixed capacity and the point lists are inputs of the step: the iteration is captured, and a
replay follows ITS batch's points, not the recorded ones. Modelled on
tests/test_graph_pose_gpu.py: child processes with their own timeouts, the helpers of
tests/test_graph_families_gpu.py."""
import json
import os
import subprocess
import sys

import pytest

import test_graph_families_gpu as fam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('wc_vid2vid_guidance', 3), ('wc_vid2vid', 3)]


@pytest.mark.gpu
def test_guidance_config_is_captured():
    cmd = [sys.executable, '-u', 'scripts/bench_families.py', '--config',
           'configs/unit_test/wc_vid2vid_guidance.yaml', '--seq-len', '3', '--graph', '--steps',
           '3', '--warmup', '3']
    env = dict(os.environ)
    env.pop('DEBUG_CLR_GRAPH_PACKET_CAPTURE', None)  # the package default is under test
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert out['hipgraph'] is True, 'the wc-vid2vid iteration was not captured:\n' + '\n'.join(
        ln for ln in r.stderr.splitlines() if ln.startswith('[graph]'))
    assert out['losses_finite'] is True
    assert out['losses']['Guidance'] > 0, out['losses']


def _cloud(tr):
    """Colour words and counters of the generator's point cloud (clones), or None."""
    state = tr.net_G_module.renderer.state
    return None if state is None else (state.color.clone(), state.counters.clone())


def _run_case(name, seq_len):
    """``test_graph_families_gpu._run_case`` plus the renderer's state: after the capture-time
    batch, after the replay of the OTHER batch and after the eager run of that batch."""
    import torch
    from imaginaire_amd.utils.cuda_graph import graph_routing, make_trainer_step
    torch.cuda.set_device(0)
    torch.use_deterministic_algorithms(True, warn_only=True)
    cfg, tr, batches = fam._build(name, seq_len)
    capturable = bool(getattr(tr, 'graph_capturable', False))
    step, graphed = make_trainer_step(tr, warmup=2, enabled=True)
    if graphed is None:
        return {'capturable': capturable, 'graphed': False}
    for i in range(3):  # 2 eager warm-up iterations, then capture (+ first replay): batch 0
        torch.manual_seed(3)
        step(tr.start_of_iteration(fam._fresh(batches[i % 2]), i))
    torch.cuda.synchronize()
    captured = graphed.graph is not None and not graphed.failed
    cloud_capture = _cloud(tr)
    state = fam._state(tr)
    saved = [t.detach().clone() for t in state]
    gparams = list(tr.net_G.parameters())
    p0 = [p.detach().clone() for p in gparams]
    d = tr.start_of_iteration(fam._fresh(batches[1]), 3)
    torch.manual_seed(11)
    graphed(d)
    torch.cuda.synchronize()
    lg = fam._losses(tr)
    cloud_replay = _cloud(tr)
    dg = [p.detach() - q for p, q in zip(gparams, p0)]
    gg = [None if p.grad is None else p.grad.detach().float().clone() for p in gparams]
    with torch.no_grad():
        for t, c in zip(state, saved):
            t.copy_(c)
    torch.cuda.synchronize()
    d = tr.start_of_iteration(fam._fresh(batches[1]), 3)
    torch.manual_seed(11)
    with graph_routing():  # the kernels the capture recorded
        graphed.step_fn(d)
    torch.cuda.synchronize()
    le = fam._losses(tr)
    cloud_eager = _cloud(tr)
    de = [p.detach() - q for p, q in zip(gparams, p0)]
    ge = [None if p.grad is None else p.grad.detach().float() for p in gparams]
    gnum = sum(float((x - y).pow(2).sum()) for x, y in zip(gg, ge) if x is not None)
    gden = sum(float(y.pow(2).sum()) for x, y in zip(gg, ge) if x is not None)
    names = [n for n, _ in tr.net_G.named_parameters()]
    bad = [n for n, x in zip(names, dg) if not torch.isfinite(x).all()]
    bad_eager = [n for n, x in zip(names, de) if not torch.isfinite(x).all()]
    num = sum(float((x - y).float().pow(2).sum()) for x, y in zip(dg, de))
    den = sum(float(y.float().pow(2).sum()) for y in de)
    res = {'capturable': capturable, 'graphed': True, 'captured': captured, 'lg': lg, 'le': le,
           'bad': bad[:8], 'bad_eager': bad_eager[:8], 'num': num, 'den': den, 'gnum': gnum,
           'gden': gden, 'cloud': cloud_replay is not None}
    if cloud_replay is not None:
        res['cloud_equal'] = all(torch.equal(a, b) for a, b in zip(cloud_replay, cloud_eager))
        res['cloud_moved'] = not torch.equal(cloud_replay[0], cloud_capture[0])
        res['counters'] = [cloud_capture[1].tolist(), cloud_replay[1].tolist(),
                           cloud_eager[1].tolist()]
        res['points'] = tr.net_G_module.renderer.num_points()
    return res


def _worker(cases, q):
    import faulthandler
    faulthandler.dump_traceback_later(170 * len(cases), exit=True, file=sys.__stderr__)
    for case in cases:
        try:
            q.put((case[0], 'ok', _run_case(*case)))
        except BaseException as e:  # noqa: BLE001 - reported to the parent
            import traceback
            q.put((case[0], 'error', '%s: %s\n%s' % (type(e).__name__, e,
                                                     traceback.format_exc())))


_RESULTS = {}


def _results():
    if not _RESULTS:
        import multiprocessing as mp
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        proc = ctx.Process(target=_worker, args=(CASES, q))
        proc.start()
        try:
            for _ in CASES:
                name, status, res = q.get(timeout=190)
                _RESULTS[name] = (status, res)
        finally:
            proc.join(30)
            if proc.is_alive():
                proc.kill()
    return _RESULTS


@pytest.mark.gpu
@pytest.mark.parametrize('name,seq_len', CASES)
def test_wc_graph_replay_matches_eager(name, seq_len):
    """The comparison of test_graph_families_gpu.py (same thresholds: losses 1e-3, G gradients
    1e-4 in relative L2^2, G update 1e-2) on a batch different from the capture batch, for the
    config with point lists and the plain one. With point lists the replay must also leave
    the renderer's colour state and counters (call_idx, drops) exactly as the eager run
    does, and the colour state not as the capture-time batch left it (call_idx is the number
    of frames after every iteration, since each iteration starts from a reset cloud: it is
    checked against the sequence length)."""
    status, res = _results()[name]
    assert status == 'ok', res
    assert res['capturable'], name + ' is not marked capturable'
    assert res['graphed'] and res['captured'], 'step was not captured'
    lg, le = res['lg'], res['le']
    print(name, 'graph', lg, '\n', name, 'eager', le)
    assert not res['bad'], 'non-finite replayed G updates: %s (eager: %s; losses %s / %s)' % (
        res['bad'], res['bad_eager'], lg, le)
    assert lg.keys() == le.keys() and lg
    for k in le:
        assert lg[k] == lg[k], k  # finite
        assert abs(lg[k] - le[k]) <= 1e-3 * max(1.0, abs(le[k])), (k, lg[k], le[k])
    assert res['gden'] > 0 and res['gnum'] <= 1e-4 * res['gden'], (res['gnum'], res['gden'])
    assert res['den'] > 0 and res['num'] <= 1e-2 * res['den'], (res['num'], res['den'])
    if name == 'wc_vid2vid_guidance':
        assert res['cloud'] and lg['G/Guidance'] > 0
        print('counters capture / replay / eager', res['counters'], 'points', res['points'])
        assert res['cloud_equal'], 'replayed renderer state differs from the eager run\'s'
        assert res['cloud_moved'], 'the replay kept the capture-time point cloud'
        assert res['counters'][1] == res['counters'][2]
        assert res['counters'][1][0][0] == seq_len and res['points'][0] > 0
    else:
        assert not res['cloud']
