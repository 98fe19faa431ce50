"""Flagship benchmark: SPADE/GauGAN training throughput, 256x512, bf16.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line; it measures
nothing else. ``--full`` is where measurements beyond the headline figure belong (there are
none at present: the profiling options below are each asked for by name). ``--dump-outputs
DIR`` writes what the last timed step left its caller (see ``_dump_outputs``), so that two
builds can be compared output for output: weights, data and noise are seeded, and that last
step starts from the seeded state again (see ``_Seeded``), so the same arguments give it the
same inputs in every run.

Metric (BASELINE.json): whole-node images/s for SPADE 256x512 — one "step" is
one full training iteration of the reference SPADE trainer: D update (G
forward under no_grad, D forward on real+fake, hinge loss, backward, Adam)
followed by G update (G forward with style encoder, D forward, GAN + feature
matching + VGG-19 perceptual + KL, backward through D and G, Adam) and the EMA
update of the averaged generator. COCO-Stuff-shaped synthetic data
(183 classes + don't-care + edge), random-init weights, batch 4 per GPU
(the reference recipe), weak scaling. rank 0 prints ONE JSON line.
"""
import argparse
import contextlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# Reference throughput: the model zoo trained SPADE COCO-Stuff 256x256 on a
# DGX-1 (8x V100) in 2-3 weeks => 26-39 img/s/node; pixel-scaled to 256x512
# => 13-20 img/s per 8-GPU node. We compare against the upper
# end (20 img/s), the conservative choice.
BASELINE_IMG_S = 20.0


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1,
                   help='number of ranks (one per GPU). Without a launcher (no WORLD_SIZE) '
                        'bench.py starts them itself through torch.distributed.run')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=6)
    p.add_argument('--config', default=os.path.join(HERE, 'configs', 'bench',
                                                     'spade_256x512_synthetic.yaml'))
    p.add_argument('--batch', type=int, default=None, help='per-GPU batch (default: config)')
    p.add_argument('--dump-outputs', metavar='DIR', default=None,
                   help='after the timed steps, write what the last step computed (losses, and a '
                        'fixed seeded sample of the updated G / D state) as DIR/<name>.npy; '
                        'that step starts from the seeded initial state, put back with the '
                        'clock stopped')
    p.add_argument('--full', action='store_true',
                   help='also run every measurement and check beyond the headline figure (none '
                        'at present: a plain run already does only what its result line needs)')
    p.add_argument('--eager', action='store_true',
                   help='self-baseline: PyTorch reference ops instead of the HIP kernels '
                        '(implies --no-graph)')
    p.add_argument('--no-graph', action='store_true',
                   help='issue every kernel from Python each step instead of replaying the '
                        'hipGraph-captured step (A/B)')
    p.add_argument('--profile-phases', action='store_true')
    p.add_argument('--verbose', action='store_true')
    p.add_argument('--backend', default='nccl',
                   help='process-group backend for N>1 (nccl = RCCL over xGMI; gloo for '
                        'single-GPU multi-rank rehearsals with --share-gpu)')
    p.add_argument('--device', default='cuda', choices=('cuda', 'cpu'),
                   help='cpu: plumbing rehearsal of the launcher / DDP path (gloo), no GPU')
    p.add_argument('--force-dist', action='store_true',
                   help='measurement only: run the distributed wrappers (bucketed DDP over a '
                        'native RCCL communicator, sync-BN exchanges) on a ONE-rank process '
                        'group, to price their overhead against the plain world-1 step')
    p.add_argument('--share-gpu', action='store_true',
                   help='testing only: every rank uses cuda:0 (rehearse the DDP path on one GPU)')
    p.add_argument('--torch-profile', action='store_true',
                   help='after warm-up, profile one step on the host (torch.profiler, CPU '
                        'activities) and print the top operators to stderr')
    p.add_argument('--conv-profile', action='store_true',
                   help='after warm-up, profile one step with device activity and shapes and '
                        'print GPU time per (op, input shapes) to stderr')
    p.add_argument('--op-profile', action='store_true',
                   help='like --conv-profile but for every aten op (self device time)')
    p.add_argument('--conv-log', action='store_true',
                   help='after warm-up, time every conv kernel call of one eager step (device '
                        'events) and print time / TF/s per (kind, shape, kernel) to stderr')
    p.add_argument('--op-stack', action='store_true',
                   help='with --op-profile: group the small elementwise ops by Python call site')
    return p.parse_args()


def _heartbeat(period=20.0):
    """Print a line to stderr every ``period`` s: the first warm-up step on a fresh
    box spends minutes inside MIOpen kernel compilation and prints nothing else."""
    import threading

    t0 = time.time()

    def run():
        while True:
            time.sleep(period)
            print('[bench] alive %.0f s' % (time.time() - t0), file=sys.__stderr__, flush=True)

    threading.Thread(target=run, daemon=True).start()


def _free_port():
    import socket
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args, argv):
    """``--gpus N`` without a launcher: start N ranks (one process per GPU) as a CHILD
    ``torch.distributed.run`` and exit with its status. Runs before anything touches the
    GPU (no exec from a process holding a HIP context). Reference launch form:
    ``python -m torch.distributed.launch --nproc_per_node=N train.py`` (projects/*/README.md)."""
    import subprocess
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node=%d' % args.gpus, '--master-addr=127.0.0.1',
           '--master-port=%d' % _free_port(), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '4')
    print('[bench] launching %d ranks: %s' % (args.gpus, ' '.join(cmd)), file=sys.stderr,
          flush=True)
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    world_env = os.environ.get('WORLD_SIZE')
    if world_env is None and args.gpus > 1:
        sys.exit(launch_ranks(args, sys.argv[1:]))
    if world_env is not None and int(world_env) != args.gpus:
        sys.exit('bench.py: --gpus %d but WORLD_SIZE=%s: refusing to report a %s-rank number '
                 'as %d GPUs' % (args.gpus, world_env, world_env, args.gpus))
    if args.share_gpu and args.gpus > 1 and args.backend == 'nccl':
        sys.exit('bench.py: --share-gpu needs --backend gloo (RCCL cannot place two ranks '
                 'on one GPU)')
    _heartbeat()
    if args.eager:
        os.environ['IMAGINAIRE_AMD_EAGER'] = '1'
    import torch
    import torch.distributed as dist

    real_stdout = sys.stdout
    sys.stdout = sys.stderr  # keep stdout for the single JSON line
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.share_gpu:
        local_rank = 0
    from imaginaire_amd.config import Config
    from imaginaire_amd.utils.distributed import init_dist
    from imaginaire_amd.utils.trainer import get_model_optimizer_and_scheduler, get_trainer
    from imaginaire_amd.datasets.synthetic import DeviceBatchSource

    on_gpu = args.device == 'cuda'
    if on_gpu:
        # set the device before the process group so RCCL binds rank r to GPU r
        torch.cuda.set_device(local_rank)
    if args.force_dist and world == 1:
        os.environ.setdefault('RANK', '0')
        os.environ.setdefault('WORLD_SIZE', '1')
        os.environ.setdefault('MASTER_PORT', str(29500 + os.getpid() % 1000))
        os.environ['IMAGINAIRE_AMD_FORCE_DIST'] = '1'
    if world > 1 or args.force_dist:
        init_dist(local_rank, backend=args.backend if on_gpu else 'gloo')
    from imaginaire_amd.utils.cudnn import init_cudnn
    init_cudnn(False, True)
    device = torch.device('cuda', local_rank) if on_gpu else torch.device('cpu')
    cfg = Config(args.config)
    cfg.logdir = os.path.join('/tmp', 'imaginaire_amd_bench')
    if args.batch:
        cfg.data.train.batch_size = args.batch
    if args.profile_phases:
        cfg.speed_benchmark = True  # synchronised per-phase timers in the trainer
    bs = cfg.data.train.batch_size
    net_G, net_D, opt_G, opt_D, sch_G, sch_D = get_model_optimizer_and_scheduler(cfg, seed=0)
    trainer = get_trainer(cfg, net_G, net_D, opt_G, opt_D, sch_G, sch_D,
                          train_data_loader=[], val_data_loader=None)
    src = DeviceBatchSource(cfg, bs, device, pool=8, seed=rank)
    # steady-state iteration: hipGraph-captured (world size 1) after max(1, W-2) eager
    # warm-up steps, so with W >= 2 the timed steps are all replays
    from imaginaire_amd.utils.cuda_graph import make_trainer_step
    use_graph = on_gpu and not (args.no_graph or args.eager or args.profile_phases or
                                args.conv_log) and args.warmup >= 2
    run_step, graphed = make_trainer_step(trainer, warmup=min(3, max(1, args.warmup - 2)),
                                          enabled=use_graph)

    def step(it):
        data = src.next()
        data = trainer.start_of_iteration(data, it)
        run_step(data)

    # --dump-outputs: the last timed step starts from the seeded state held here (see _Seeded)
    seeded = _Seeded(trainer, src, device) if args.dump_outputs else None

    for it in range(args.warmup):
        step(it)
        if rank == 0:
            print('[bench] warmup {} done'.format(it), flush=True)

    if args.torch_profile and rank == 0:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU], with_stack=False) as prof:
            step(args.warmup)
            torch.cuda.synchronize()
        print(prof.key_averages().table(sort_by='self_cpu_time_total', row_limit=45),
              flush=True)

    if args.conv_log and rank == 0:
        from imaginaire_amd.ops import conv as conv_ops
        torch.cuda.synchronize()
        conv_ops.enable_conv_log(True)
        t0 = time.perf_counter()
        step(args.warmup)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        rows = conv_ops.conv_log_summary()
        conv_ops.enable_conv_log(False)
        tot = sum(r[4] for r in rows)
        fl = sum(r[5] * r[4] * 1e9 for r in rows)
        print('conv kernels in one eager step: %.2f ms of %.1f ms wall, %.1f TFLOP, %.0f TF/s' % (
            tot, wall, fl / 1e12, fl / max(tot, 1e-9) / 1e9))
        by_kind = {}
        for r in rows:
            k = by_kind.setdefault((r[0], r[1]), [0, 0.0, 0.0])
            k[0] += r[3]
            k[1] += r[4]
            k[2] += r[5] * r[4] * 1e9
        for (kind, path), (n, ms, f) in sorted(by_kind.items(), key=lambda kv: -kv[1][1]):
            print('  %-6s %-7s %4d calls %8.2f ms %6.0f TF/s' % (kind, path, n, ms,
                                                              f / max(ms, 1e-9) / 1e9))
        for kind, path, desc, n, ms, tfs in rows:
            print('%8.3f ms %3d  %-6s %-7s %5.0f TF/s  %s' % (ms, n, kind, path, tfs, desc))
        sys.stdout.flush()

    if (args.conv_profile or args.op_profile) and rank == 0:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA],
                     record_shapes=True, with_stack=args.op_stack) as prof:
            step(args.warmup)
            torch.cuda.synchronize()
        if args.op_profile and args.op_stack:
            rows = [e for e in prof.key_averages(group_by_stack_n=4)
                    if e.self_device_time_total > 0 and e.key.startswith('aten::') and
                    e.key not in ('aten::convolution_backward', 'aten::miopen_convolution')]
            rows.sort(key=lambda e: -e.self_device_time_total)
            print('op self GPU time by call site (aten ops only): %.2f ms' % (
                sum(e.self_device_time_total for e in rows) / 1e3))
            for e in rows[:60]:
                print('%9.3f ms %5d  %-24s %s' % (e.self_device_time_total / 1e3, e.count,
                                                  e.key[:24], ' <- '.join(e.stack[:4])[:220]))
        elif args.op_profile:
            rows = [e for e in prof.key_averages(group_by_input_shape=True)
                    if e.self_device_time_total > 0 and e.input_shapes is not None and
                    not e.key.startswith(('void', 'igemm', 'iamd', '__amd', 'Sub'))]
            rows.sort(key=lambda e: -e.self_device_time_total)
            tot = sum(e.self_device_time_total for e in rows)
            print('op self GPU time in one step: %.2f ms' % (tot / 1e3))
            for e in rows[:250]:
                print('%9.3f ms %4d  %-34s %s' % (e.self_device_time_total / 1e3, e.count,
                                                  e.key[:34], str(e.input_shapes)[:140]))
        else:
            rows = [e for e in prof.key_averages(group_by_input_shape=True)
                    if e.key in ('aten::convolution', 'aten::convolution_backward')]
            rows.sort(key=lambda e: -e.device_time_total)
            tot = sum(e.device_time_total for e in rows)
            print('conv GPU time in one step: %.2f ms' % (tot / 1e3))
            for e in rows[:60]:
                print('%9.3f ms %4d  %-22s %s' % (e.device_time_total / 1e3, e.count, e.key[6:],
                                                  str(e.input_shapes)[:150]))
        sys.stdout.flush()

    def barrier():
        if world > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    barrier()
    if args.profile_phases:
        trainer._reset_speed_accumulators()
    if args.verbose:
        try:  # phase marker for scripts/gpu/summarize_kernels.py (steady-state split)
            from imaginaire_amd.ops import _ext
            _ext.ext().profile_marker(1)
        except Exception:  # noqa: BLE001
            pass
    t0 = time.perf_counter()
    paused = 0.0
    for it in range(args.steps):
        if seeded is not None and it == args.steps - 1:
            barrier()  # the clock stops while the seeded state is put back
            t1 = time.perf_counter()
            seeded.restore()
            barrier()
            paused = time.perf_counter() - t1
        step(args.warmup + it)
        if rank == 0 and args.verbose:
            print('[bench] step {} queued'.format(it), flush=True)
    barrier()
    elapsed = time.perf_counter() - t0 - paused
    t = torch.tensor([elapsed], device=device if args.backend == 'nccl' and on_gpu else 'cpu',
                     dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    if args.profile_phases and rank == 0:
        n = args.steps
        for k in ('gen_forw', 'gen_loss', 'gen_back', 'gen_step', 'gen_avg', 'dis_forw',
                  'dis_loss', 'dis_back', 'dis_step'):
            print('[bench] phase %-9s %8.1f ms/step' % (
                k, getattr(trainer, 'accu_%s_iter_time' % k) / n * 1e3), flush=True)
    # correctness of what was timed: the last step's losses (every rank) and, at world > 1,
    # whether the replicas still hold bitwise identical parameters (a rank-divergent replay or
    # unused-parameter mask would desynchronise them silently)
    losses = _last_losses(trainer)
    finite = all(v == v and abs(v) != float('inf') for v in losses.values())
    if world > 1:
        fl = torch.tensor([0.0 if finite else 1.0], dtype=torch.float64,
                          device=device if args.backend == 'nccl' and on_gpu else 'cpu')
        dist.all_reduce(fl, op=dist.ReduceOp.MAX)
        finite = float(fl.item()) == 0.0
    in_sync = _replicas_in_sync(trainer, world, device if args.backend == 'nccl' and on_gpu
                                else torch.device('cpu'))
    ms_per_step = elapsed / args.steps * 1e3
    value = world * bs * args.steps / elapsed
    mem_gb = torch.cuda.max_memory_allocated(device) / 2 ** 30 if on_gpu else 0.0
    if args.dump_outputs and rank == 0:
        _dump_outputs(trainer, args.dump_outputs)
    sys.stdout = real_stdout
    if rank == 0:
        out = {
            'metric': 'imgs/sec (whole node) SPADE 256x512 training',
            'value': round(value, 3),
            'unit': 'images/s',
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(ms_per_step, 3),
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': round(value / BASELINE_IMG_S, 3),
            'dtype': 'bf16' if on_gpu else 'fp32',
            'data': 'synthetic (COCO-Stuff-shaped: 183 classes + dont-care + edge), random-init weights',
            'config': {'model': 'SPADE/GauGAN (cocostuff base128_bs4 recipe: F=128, style VAE, '
                                'sync-BN SPADE 5x5 separate-projection, 2xPatchGAN+FPSE D, '
                                'VGG19 perceptual, EMA)',
                       'global_batch': bs * world, 'seq_len': None, 'resolution': '256x512',
                       'parallelism': 'dp%d' % world + ('-forced-dist' if args.force_dist else ''),
                       'kernels': 'eager-reference' if args.eager else 'hip',
                       'hipgraph': bool(graphed is not None and graphed.graph is not None),
                       'backend': args.backend if (world > 1 and on_gpu) else
                       ('gloo' if world > 1 else None),
                       'device': args.device},
            'peak_mem_gb_rank0': round(mem_gb, 2),
            'losses_rank0': losses,
            'losses_finite': finite,
            'replicas_in_sync': in_sync,
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if not finite:
        print('[bench] NON-FINITE losses after the timed steps: %s' % json.dumps(losses),
              file=sys.stderr, flush=True)
        sys.exit(3)
    if in_sync is False:
        print('[bench] replicas hold different parameters after the timed steps',
              file=sys.stderr, flush=True)
        sys.exit(4)


def _last_losses(trainer):
    """The last step's D and G losses (graph outputs after a replay) as floats."""
    import torch
    out = {}
    for tag, src in (('G', getattr(trainer, 'gen_losses', {})),
                     ('D', getattr(trainer, 'dis_losses', {}))):
        for k, v in src.items():
            if torch.is_tensor(v) and v.numel() == 1:
                out['%s/%s' % (tag, k)] = round(float(v), 5)
    return out


class _Seeded(object):
    """The state a step starts from, taken right after the seeded set-up: G (with its averaged
    copy) and D parameters and buffers, the random generators, the batch source's position.
    ``restore()`` puts it back in place (a captured step keeps its pointers), zeroes the Adam
    moments and rewinds the optimizers' step counters.

    ``--dump-outputs`` restores it before the last timed step, with the clock stopped. Without
    that the dumped step would start from wherever the earlier steps led, and that is no fixed
    point: the default kernels accumulate with atomics, Adam's first steps turn a last-bit
    difference of a small gradient into a +-lr difference of its weight, and GAN training
    grows it from there. Measured on one MI355X, same build and arguments, relative L2
    distance of the sampled G state between two runs: 9e-6 after 1 step, 4e-3 after 3, 8e-2
    after 7, 5e-1 after 25 (the G loss 11.05 against 9.14). From the restored state two runs
    of --steps 20 --warmup 5 (graph replays) agree as after 1 step, with each other and with
    an eager first step: every loss bitwise, the sampled state to 9e-6 (at most 2 lr per
    weight). So two builds can be compared at any --steps. The stop costs the timed window one
    extra synchronisation: 72.1-72.3 ms per step against 71.9-72.0 without the option."""

    def __init__(self, trainer, src, device):
        import copy
        import torch
        self.trainer, self.src, self.device = trainer, src, device
        self.nets = [(net, copy.deepcopy(net.state_dict()))
                     for net in (trainer.net_G, trainer.net_D) if net is not None]
        self.src_step = src.step
        self.cpu_rng = torch.get_rng_state()
        self.gpu_rng = torch.cuda.get_rng_state(device) if device.type == 'cuda' else None

    def restore(self):
        import torch
        with torch.no_grad():
            for net, state in self.nets:
                net.load_state_dict(state)
            for opt in (self.trainer.opt_G, self.trainer.opt_D):
                if opt is None:
                    continue
                sd = opt.state_dict()
                moments = [t for s in sd['state'].values() for t in s.values()
                           if torch.is_tensor(t)]
                where = [t.data_ptr() for t in moments]
                for t in moments:
                    t.zero_()
                for g in sd['param_groups']:
                    if 'step' in g:
                        g['step'] = 0
                opt.load_state_dict(sd)  # (FusedAdam: also rewinds its device step counter)
                now = [t.data_ptr() for s in opt.state_dict()['state'].values()
                       for t in s.values() if torch.is_tensor(t)]
                assert now == where, 'optimizer state moved: a captured step would not see it'
        self.src.step = self.src_step
        torch.set_rng_state(self.cpu_rng)
        if self.gpu_rng is not None:
            torch.cuda.set_rng_state(self.gpu_rng, self.device)


DUMP_BYTES_PER_NET = 24 << 20  # two networks: 48 MB of float32 at the most


def _state_sample(net, gen):
    """A fixed sample of every floating-point tensor of ``net.state_dict()`` (parameters, the
    averaged generator, BatchNorm statistics, spectral-norm u / v), in key order, as one
    float32 vector: tensors up to the per-tensor cap whole, larger ones at indices drawn from
    ``gen`` (logical element order, so the memory format of a tensor does not matter)."""
    import torch
    state = [(k, v) for k, v in sorted(net.state_dict().items())
             if torch.is_tensor(v) and v.is_floating_point() and v.numel() > 0]
    cap = max(16, min(4096, DUMP_BYTES_PER_NET // 4 // max(1, len(state))))
    parts = []
    for _, v in state:
        flat = v.detach().reshape(-1)
        if flat.numel() > cap:
            idx = torch.randint(0, flat.numel(), (cap,), generator=gen)
            flat = flat.index_select(0, idx.to(flat.device))
        parts.append(flat.float().cpu())
    return torch.cat(parts).numpy()[:DUMP_BYTES_PER_NET // 4]


def _dump_outputs(trainer, out_dir):
    """What the last timed step handed its caller, as ``out_dir/<name>.npy``: the D and G
    losses it left in ``trainer.dis_losses`` / ``trainer.gen_losses`` (float64, in sorted key
    order) and the state it updated, G with its averaged copy and D (float32, a fixed seeded
    sample per tensor: see ``_state_sample``)."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    arrays = {}
    for name, src in (('gen_losses', trainer.gen_losses), ('dis_losses', trainer.dis_losses)):
        keys = sorted(k for k, v in src.items() if torch.is_tensor(v) and v.numel() == 1)
        arrays[name] = np.array([float(src[k]) for k in keys], dtype=np.float64)
    gen = torch.Generator().manual_seed(20240229)
    for name, net in (('net_G_state', trainer.net_G), ('net_D_state', trainer.net_D)):
        if net is not None:
            arrays[name] = _state_sample(net, gen)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)
    print('[bench] wrote %s to %s (%.1f MB)' % (
        ', '.join(sorted(arrays)), out_dir, sum(a.nbytes for a in arrays.values()) / 1e6),
        flush=True)


def _replicas_in_sync(trainer, world, device):
    """World > 1: True when every rank holds bitwise identical G and D parameters (one fp64
    checksum per tensor of the fp32 bits, compared by a MIN / MAX all-reduce); None at world 1."""
    if world <= 1:
        return None
    import torch
    import torch.distributed as dist
    sums = []
    for net in (trainer.net_G, trainer.net_D):
        if net is None:
            continue
        for p in net.parameters():
            # the int32 view makes the checksum sensitive to every bit of every element
            bits = p.detach().float().contiguous().view(torch.int32)
            sums.append(bits.to(torch.float64).sum() + 1e-3 * bits[::7].to(torch.float64).sum())
    v = torch.stack(sums).to(device)
    hi, lo = v.clone(), v.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return bool(torch.equal(hi, lo))


if __name__ == '__main__':
    main()
