"""World-consistent vid2vid trainer (reference trainers/wc_vid2vid.py:20-513).

vid2vid schedule with the fork's external flow (``data['flow']`` = flow xy
+ occlusion mask per frame), guidance images from the point-cloud renderer
(masked, valid-normalised L1 ``Guidance`` loss) and a frozen single-image
model for the first frame. The reference's hard-coded output path
(wc_vid2vid.py:138) is replaced by the standard per-sequence directory.
"""
import os
import time

import numpy as np
import torch

from imaginaire_amd.generators.wc_vid2vid import guidance_key
from imaginaire_amd.losses import MaskedL1Loss
from imaginaire_amd.model_utils.fs_vid2vid import concat_frames
from imaginaire_amd.model_utils.wc_vid2vid.render import unprojections_to_rows
from imaginaire_amd.trainers.base import follows_test_loader
from imaginaire_amd.trainers.vid2vid import Trainer as Vid2VidTrainer
from imaginaire_amd.trainers.vid2vid import _imwrite, _save_video
from imaginaire_amd.utils.distributed import is_master
from imaginaire_amd.utils.distributed import master_only_print as print
from imaginaire_amd.utils.misc import split_labels
from imaginaire_amd.utils.visualization import tensor2flow, tensor2im


class Trainer(Vid2VidTrainer):
    # the point cloud of the guidance renderer is device state of fixed capacity, updated and
    # rendered in place from point lists that are inputs of the step (``_device_unprojections``):
    # the iteration is captured like vid2vid's, and every replay follows its own batch's points
    graph_capturable = True

    @classmethod
    def rank_uniform(cls, cfg):
        # which frames carry point lists (and so which guidance layers get gradients) is decided
        # by each rank's data: DDP keeps the global unused mask, multi-rank steps stay eager
        return False

    def __init__(self, cfg, net_G, net_D, opt_G, opt_D, sch_G, sch_D, train_data_loader,
                 val_data_loader):
        super().__init__(cfg, net_G, net_D, opt_G, opt_D, sch_G, sch_D, train_data_loader,
                         val_data_loader)
        self.guidance_start_after = getattr(cfg.gen.guidance, 'start_from', 0)

    def _define_custom_losses(self):
        self.criteria['Guidance'] = MaskedL1Loss(normalize_over_valid=True)
        self.weights['Guidance'] = self.cfg.trainer.loss_weight.guidance

    def _device_unprojections(self, data):
        """Replace ``data['unprojections']`` (``{resolution: [B, T, N + 1, 3]}``, padded, with
        the length sentinel) by what the device renderer takes: ``unprojection_rows`` int32
        ``[B, T, Rcap, 3]``, ``unprojection_counts`` int32 ``[B, T]`` and the guidance size
        ``unprojection_hw``, with the horizontal flip of ``data['is_flipped']`` applied to the
        rows. Runs outside the captured step; reads nothing back. Idempotent."""
        unprojections = data.get('unprojections')
        if not isinstance(unprojections, dict) or not unprojections or \
                'unprojection_rows' in data:
            return data
        data = dict(data)
        del data['unprojections']
        key, h, w = guidance_key(unprojections, *data['label'].shape[-2:])
        if key not in unprojections:
            return data
        value = unprojections[key].to(self.device)
        max_rows = int(getattr(self.cfg.gen.guidance, 'max_rows', 0) or h * w)
        data['unprojection_rows'], data['unprojection_counts'] = unprojections_to_rows(
            value, max_rows, w, data.get('is_flipped'))
        data['unprojection_hw'] = (h, w)
        return data

    def start_of_iteration(self, data, current_iteration):
        self.net_G_module.reset_renderer()
        data = self._device_unprojections(self.to_device(data))
        self.current_iteration = current_iteration
        if not self.is_inference:
            self.net_D.train()
        self.net_G.train()
        self.start_iteration_time = time.time()
        return data

    def reset(self):
        self.net_G_module.reset_renderer()
        self.net_G_output = self.data_prev = None
        self.t = 0
        net = self.net_G.module.averaged_model if getattr(
            self, 'test_in_model_average_mode', False) else self.net_G.module
        if hasattr(net, 'reset'):
            net.reset()

    def create_sequence_output_dir(self, output_dir, key):
        output_dir, seq_name = super().create_sequence_output_dir(output_dir, key)
        os.makedirs(output_dir + '/all', exist_ok=True)
        os.makedirs(output_dir + '/fake', exist_ok=True)
        return output_dir, seq_name

    @follows_test_loader
    def test(self, test_data_loader, root_output_dir, inference_args):
        loader = test_data_loader
        for sequence_idx in range(loader.dataset.num_inference_sequences()):
            loader.dataset.set_inference_sequence_idx(sequence_idx)
            print('Seq id: %d, Seq length: %d' % (sequence_idx + 1, len(loader)))
            self.reset()
            self.sequence_length = len(loader)
            video = []
            for idx, data in enumerate(loader):
                filename = 'frame_%04d' % idx
                if idx == 0:
                    key = data['key']['images'][0][0] if isinstance(data['key'], dict) \
                        else 'seq/frame'
                    output_dir, seq_name = self.create_sequence_output_dir(root_output_dir, key)
                    video_path = os.path.join(output_dir, '..', seq_name)
                data['img_name'] = filename
                data = self.to_device(data)
                output = self.test_single(data, output_dir=output_dir + '/all')
                fake = tensor2im(output['fake_images'])[0]
                video.append(fake)
                _imwrite(os.path.join(output_dir, 'fake', filename + '.jpg'), fake)
            _save_video(video_path + '.mp4', video, fps=15)

    def test_single(self, data, output_dir=None, save_fake_only=False):
        avg_mode = (self.is_inference and self.cfg.trainer.model_average) or \
            getattr(self, 'test_in_model_average_mode', False)
        # the device path of training, without a graph
        data = self._device_unprojections(data)
        data_t = self.get_data_t(data, self.net_G_output, self.data_prev, 0)
        if self.sequence_length > 1:
            self.data_prev = data_t
        net_G = self.net_G.module.averaged_model if avg_mode else self.net_G
        if self.t == 0:
            (net_G if avg_mode else self.net_G_module).reset_renderer()
        with torch.no_grad(), self.autocast():
            self.net_G_output = net_G(data_t)
        if output_dir is not None:
            if save_fake_only:
                image_grid = tensor2im(self.net_G_output['fake_images'])[0]
            else:
                vis = self.get_test_output_images(data)
                image_grid = np.hstack([np.vstack(im) for im in vis if im is not None])
            name = data['img_name'].split('.')[0] + '.jpg' if 'img_name' in data \
                else '%04d.jpg' % self.t
            _imwrite(os.path.join(output_dir, name), image_grid)
            self.t += 1
        return self.net_G_output

    def get_test_output_images(self, data):
        labels = split_labels(data['label'], self.val_data_loader.dataset.get_label_lengths())
        vis = [self.visualize_label(v[:, -1]) if k == 'seg_maps' else tensor2im(v[:, -1])
               for k, v in labels.items()]
        return vis + [tensor2im(self.net_G_output['fake_images'])]

    def gen_frames(self, data, use_model_average=False):
        net_G = self.net_G.module.averaged_model if use_model_average else self.net_G_module
        net_G.reset_renderer()
        return super().gen_frames(self._device_unprojections(data), use_model_average)

    def _get_custom_gen_losses(self, data_t, net_G_output, net_D_output):
        g = net_G_output.get('guidance_images_and_masks')
        if g is not None:
            self.gen_losses['Guidance'] = self.criteria['Guidance'](
                net_G_output['fake_images'], g[:, :3], g[:, 3:])
        else:
            self.gen_losses['Guidance'] = torch.zeros((), device=self.device)

    def get_data_t(self, data, net_G_output, data_prev, t):
        label = data['label'][:, t]
        flow = data['flow'][:, t][:, :2]
        mask = data['flow'][:, t][:, 2:]
        unprojection = None
        if t >= self.guidance_start_after and 'unprojection_rows' in data:
            # views of frame t's point list (device tensors; see _device_unprojections)
            unprojection = dict(rows=data['unprojection_rows'][:, t],
                                counts=data['unprojection_counts'][:, t],
                                hw=data['unprojection_hw'])
        if data_prev is not None:
            n = self.cfg.data.num_frames_G
            prev_labels = concat_frames(data_prev['prev_labels'], data_prev['label'], n - 1)
            prev_images = concat_frames(data_prev['prev_images'],
                                        net_G_output['fake_images'].detach(), n - 1)
        else:
            prev_labels = prev_images = None
        return dict(label=label, image=data['images'][:, t], flow=flow, mask=mask,
                    prev_labels=prev_labels, prev_images=prev_images,
                    real_prev_image=data['images'][:, t - 1] if t > 0 else None,
                    unprojection=unprojection)

    def save_image(self, path, data):
        self.net_G.eval()
        self.net_G_output = None
        first, last, all_info = self.gen_frames(data)
        labels = split_labels(data['label'], self.train_data_loader.dataset.get_label_lengths())
        vis_start = [self.visualize_label(v[:, -1]) if 'seg_maps' in k else tensor2im(v[:, -1])
                     for k, v in labels.items()]
        if is_master():
            vis = [*vis_start, tensor2im(data['images'][:, -1]), tensor2im(last['fake_images'])]
            if last['fake_flow_maps'] is not None:
                vis += [tensor2flow(last['fake_flow_maps']),
                        tensor2im(last['fake_occlusion_masks'], normalize=False),
                        tensor2im(last['warped_images'])]
            image_grid = np.hstack([np.vstack(im) for im in vis if im is not None])
            print('Save output images to {}'.format(path))
            _imwrite(path, image_grid)
            if self.sequence_length > 1:
                frames = [tensor2im(o['fake_images'])[0] for o in all_info['outputs']]
                _save_video(os.path.splitext(path)[0] + '.mp4', frames, fps=2)
        self.net_G.train()

    def _compute_fid(self):
        return None

    def load_checkpoint(self, cfg, checkpoint_path, resume=None):
        load_single = self.train_data_loader is not None
        self.net_G_module._init_single_image_model(load_weights=load_single,
                                                   locrank=getattr(cfg, 'local_rank', 0))
        return super().load_checkpoint(cfg, checkpoint_path, resume)
