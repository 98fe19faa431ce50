"""wc-vid2vid guidance of one frame: the former host path vs the device path (k18).

    python scripts/probe/splat_probe.py [--out profiles/splat_probe_mi355x.txt]

Recipe shape: batch 1, 512x1024, with h * w / 4 and with h * w rows per frame (synthetic point
lists of datasets/synthetic.py: a scrolling world of ids, 1/8 duplicate pixels / ids). One
"frame" is what the generator does per frame: render the guidance of the frame's points, then
colour the cloud from the generated frame.

* host path (what the generator did before k18): the point list is copied to the host and cut
  at its length sentinel, ``SplatRenderer`` renders numpy arrays that are turned into a tensor
  and uploaded, and the generated frame comes down through ``tensor2im`` for the update;
* device path: ``splat_render`` + ``splat_update`` on device tensors (four kernel launches).

Both are timed with a host clock around a sequence of 3 frames that ends in a device
synchronise, after a warm-up, alternating round by round; the medians are per frame. Then each
op alone with device events around back-to-back launches, with the bytes the algorithm has to
move computed from the shapes (rows twice, winner words, colour words, the image pixels it
reads, the output it writes) and the share of HBM bandwidth that gives.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    p.add_argument('--rounds', type=int, default=15)
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--hw', default='512,1024')
    args = p.parse_args()

    import torch
    from imaginaire_amd.datasets.synthetic import Dataset
    from imaginaire_amd.model_utils.wc_vid2vid.render import (DeviceSplatRenderer, SplatRenderer,
                                                              unprojections_to_rows)
    from imaginaire_amd.utils.visualization import tensor2im

    if not torch.cuda.is_available():
        sys.exit('splat_probe.py needs a GPU')
    dev = torch.device('cuda', 0)
    h, w = [int(v) for v in args.hw.split(',')]
    frames = 3
    lines = ['splat_probe: %s, %dx%d, batch 1, %d frames per sequence, %d rounds' % (
        torch.cuda.get_device_name(dev), h, w, frames, args.rounds)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def lists(n):
        ds = Dataset.__new__(Dataset)
        ds.h, ds.w, ds.unprojection_points, ds._world = h, w, n, None
        ds.sequence_length_max = frames
        return ds._unprojections(0, frames)['w%dxh%d' % (w, h)]

    images = [(torch.rand(1, 3, h, w, device=dev) * 2 - 1).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last) for _ in range(frames)]

    for n in (h * w // 4, h * w):
        value = lists(n).to(dev)  # [T, N + 1, 3]
        rows, counts = unprojections_to_rows(value.unsqueeze(0), h * w, w)
        device_ren = DeviceSplatRenderer()
        host_ren = SplatRenderer()

        def device_sequence():
            device_ren.reset()
            out = None
            for t in range(frames):
                out = device_ren.render(rows[:, t], counts[:, t], h, w)
                device_ren.update(images[t], rows[:, t], counts[:, t])
            torch.cuda.synchronize()
            return out

        def host_sequence():
            host_ren.reset()
            out = None
            for t in range(frames):
                info = value[t].cpu().numpy()
                info = info[:info[-1][0]]
                image, mask = host_ren.render_image(info, w, h, return_mask=True)
                image = torch.from_numpy(image).permute(2, 0, 1).float().div(255).sub(0.5).mul(2)
                mask = torch.from_numpy(mask).permute(2, 0, 1).float().div(255)
                out = torch.cat((image, mask), dim=0).unsqueeze(0).to(dev)
                host_ren.update_point_cloud(tensor2im(images[t])[0], info)
            torch.cuda.synchronize()
            return out

        same = torch.equal(device_sequence(), host_sequence())
        host_sequence()
        device_sequence()
        td, th = [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            device_sequence()
            td.append((time.perf_counter() - t0) / frames)
            t0 = time.perf_counter()
            host_sequence()
            th.append((time.perf_counter() - t0) / frames)
        md, mh = statistics.median(td), statistics.median(th)
        say('rows/frame %7d  last guidance equal %s  per frame: host path %9.3f ms '
            '(min %.3f)  device path %7.3f ms (min %.3f)  x%.1f' % (
                n, same, mh * 1e3, min(th) * 1e3, md * 1e3, min(td) * 1e3, mh / md))

        # each op alone: events around back-to-back launches on the last frame's list
        r, c = rows[:, frames - 1], counts[:, frames - 1]
        nn = int(c[0])
        listed = int(torch.unique(r[0, :nn, 0] * w + r[0, :nn, 1]).numel())
        ops = {
            'splat_update': (lambda: device_ren.update(images[-1], r, c),
                             nn * (2 * 12 + 2 * 4 + 4) + nn * 3 * 2),
            'splat_render': (lambda: device_ren.render(r, c, h, w),
                             nn * (12 + 4) + h * w * (4 + 16) + listed * (4 + 4 + 4)),
        }
        for name, (fn, nbytes) in ops.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            meds = []
            for _ in range(5):
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                meds.append(e0.elapsed_time(e1) / args.iters * 1e-3)
            t = statistics.median(meds)
            say('    %-13s %8.1f us per call (2 kernels), %6.2f MB to move, %7.1f GB/s = '
                '%.1f %% of HBM peak' % (name, t * 1e6, nbytes / 1e6, nbytes / t / 1e9,
                                          100.0 * nbytes / t / HBM_PEAK))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
