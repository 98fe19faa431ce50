"""What ``data.packed_labels`` buys on the label path of the SPADE recipe (k19).

    python scripts/probe/label_transport_probe.py [--out profiles/label_transport_mi355x.txt]

Recipe label shape: 183 classes + don't care + edge map = 185 channels, 256 x 512, batch 4.
Packed (one uint8 index plane + the fp32 edge map per sample) against unpacked (185 fp32
channels per sample), four figures:

1. the label stage of ONE loader worker, one CPU thread: ``_encode_onehot`` + ``cat`` against
   ``_encode_index``, samples/s (host clock; no file decoding, which both paths share);
2. bytes per batch the worker hands to the main process, computed from the tensors;
3. pinned host batch -> device label (fp32, channels-last, as ``BaseTrainer.to_device``
   delivers it): copy + layout pass against copy + one k19 launch;
4. the label resizes of one generator forward at the recipe's resolutions
   (``LabelMapCache.resize`` of the bf16 label: 16 x 32 plain, then 16 x 32 .. 256 x 512
   padded to 192 channels for the SPADE convs), ``IMAGINAIRE_AMD_LABEL_PACKED_RESIZE`` 0 / 1.

3 and 4 are host-clock times around work that ends in a device synchronise, after a warm-up, the
two paths alternating round by round; median and range over the rounds. The outputs of the two
paths are compared bit for bit before anything is timed. 1 is a CPU figure of the host the
probe runs on.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

B, H, W, CLASSES = 4, 256, 512, 183
LAYOUT = [('seg_maps', 'index', CLASSES + 1, CLASSES, True), ('edge_maps', 'dense', 1, 0, False)]
RESIZES = [((16, 32), False), ((16, 32), True), ((32, 64), True), ((64, 128), True),
           ((128, 256), True), ((256, 512), True)]


def _stats(ts):
    return '%8.3f ms (min %.3f, max %.3f, %d rounds)' % (
        statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, len(ts))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    p.add_argument('--rounds', type=int, default=20)
    args = p.parse_args()

    import torch
    from imaginaire_amd.datasets.base import BaseDataset, _image_to_tensor
    from imaginaire_amd.datasets.synthetic import edge_map, voronoi_labels
    from imaginaire_amd.layers.activation_norm import LabelMapCache
    from imaginaire_amd.ops.label import cast_label, expand_packed_labels
    from imaginaire_amd.utils.misc import to_device

    if not torch.cuda.is_available():
        sys.exit('label_transport_probe.py needs a GPU')
    dev = torch.device('cuda', 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('label_transport_probe: %s, torch %s; label %d ch x %d x %d, batch %d' % (
        torch.cuda.get_device_name(0), torch.__version__, CLASSES + 2, H, W, B))
    gen = torch.Generator().manual_seed(0)
    segs = [voronoi_labels(H, W, CLASSES + 8, gen, num_sites=64) for _ in range(B)]
    # what to_tensor hands make_one_hot: the 8-bit PNG as a [1, H, W] float in [0, 1]
    raw = [_image_to_tensor(s.numpy().astype('uint8'), False) for s in segs]
    edges = [edge_map(s)[None] for s in segs]

    # -- 1. the worker's label stage
    def worker_unpacked(i):
        hot = BaseDataset._encode_onehot(raw[i] * 255.0, CLASSES, True)
        return torch.cat([hot, edges[i]], 0)

    def worker_packed(i):
        return BaseDataset._encode_index(raw[i] * 255.0, CLASSES, torch.uint8), edges[i]

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    rates = {}
    for name, fn in (('unpacked', worker_unpacked), ('packed', worker_packed)):
        fn(0)
        ts = []
        for r in range(args.rounds):
            t0 = time.perf_counter()
            fn(r % B)
            ts.append(time.perf_counter() - t0)
        rates[name] = 1.0 / statistics.median(ts)
        say('1. worker label stage, 1 CPU thread, %-8s: %s per sample = %.1f samples/s' % (
            name, _stats(ts), rates[name]))
    torch.set_num_threads(threads)

    # -- 2. bytes per batch
    unpacked = torch.stack([worker_unpacked(i) for i in range(B)])
    idx = torch.stack([worker_packed(i)[0] for i in range(B)])
    dense = torch.stack(edges)
    nb_u = unpacked.numel() * unpacked.element_size()
    nb_p = idx.numel() * idx.element_size() + dense.numel() * dense.element_size()
    say('2. label bytes per batch handed to the main process: unpacked %d (%.1f MB), packed %d '
        '(%.2f MB), %.0fx fewer' % (nb_u, nb_u / 1e6, nb_p, nb_p / 1e6, nb_u / nb_p))

    # -- 3. pinned batch -> device label
    unpacked, idx, dense = unpacked.pin_memory(), idx.pin_memory(), dense.pin_memory()

    def h2d_unpacked():
        return to_device({'label': unpacked}, dev, non_blocking=True,
                         memory_format=torch.channels_last)['label']

    def h2d_packed():
        data = to_device({'label_idx': idx, 'label_dense': dense}, dev, non_blocking=True)
        return expand_packed_labels(data, LAYOUT, channels_last=True)['label']

    a, b = h2d_unpacked(), h2d_packed()
    torch.cuda.synchronize()
    assert a.dtype == b.dtype and a.stride() == b.stride() and torch.equal(a, b)
    say('   (device labels of the two paths are bitwise equal: %s, strides %s)' % (
        tuple(a.shape), a.stride()))
    del a

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        del out
        return time.perf_counter() - t0

    ts = {'unpacked': [], 'packed': []}
    for r in range(args.rounds + 3):
        for name, fn in (('unpacked', h2d_unpacked), ('packed', h2d_packed)):
            t = timed(fn)
            if r >= 3:
                ts[name].append(t)
    for name in ('unpacked', 'packed'):
        say('3. H2D + expansion per batch, %-8s: %s' % (name, _stats(ts[name])))

    # -- 4. the label resizes of one generator forward
    label = cast_label(b, torch.bfloat16)

    def resizes():
        return [LabelMapCache.resize(label, size, conv_pad=pad) for size, pad in RESIZES]

    outs = {}
    for flag in ('0', '1'):
        os.environ['IMAGINAIRE_AMD_LABEL_PACKED_RESIZE'] = flag
        outs[flag] = resizes()
    torch.cuda.synchronize()
    for x, y in zip(outs['0'], outs['1']):
        assert x.dtype == y.dtype and x.stride() == y.stride() and torch.equal(x, y)
    out_bytes = sum(x.numel() * x.element_size() for x in outs['1'])
    del outs
    ts = {'0': [], '1': []}
    for r in range(args.rounds + 3):
        for flag in ('0', '1'):
            os.environ['IMAGINAIRE_AMD_LABEL_PACKED_RESIZE'] = flag
            t = timed(resizes)
            if r >= 3:
                ts[flag].append(t)
    say('   (resized maps of the two paths are bitwise equal; %.1f MB of bf16 maps per forward)'
        % (out_bytes / 1e6))
    for flag, name in (('0', 'pad + resize'), ('1', 'packed (k19)')):
        say('4. label resizes per generator forward, %-12s: %s' % (name, _stats(ts[flag])))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
