"""Drop-in compatibility: every project / unit-test YAML of the reference
(imaginaire.* module paths, apex AMP levels, cudnn flags, ...) loads through
this framework's Config and instantiates its generator and discriminator.

The repository's own configs are written in that schema (every ``type:`` names an
``imaginaire.*`` module): they are cases on every machine (ids ``configs/...``). The
reference's own files are further cases where its checkout is mounted (ids relative to
its ``configs`` folder); where it is not, those cases do not exist and a warning says so."""
import glob
import os
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = os.path.join(ROOT, 'configs')
OWN_CONFIGS = sorted(glob.glob(os.path.join(OWN, '**', '*.yaml'), recursive=True))
REF = '/root/reference/configs'
CONFIGS = sorted(glob.glob(os.path.join(REF, '**', '*.yaml'), recursive=True))
IDS = [os.path.join('configs', os.path.relpath(p, OWN)) for p in OWN_CONFIGS] + \
    [os.path.relpath(p, REF) for p in CONFIGS]


if not CONFIGS:
    # not a skip (nothing here can run without those files), but not silence either: the line
    # shows in pytest's warnings summary
    warnings.warn('reference checkout not found at %s: only the repository\'s own configs are '
                  'cases of test_reference_config_builds_models' % REF)


@pytest.mark.parametrize('path', OWN_CONFIGS + CONFIGS, ids=IDS)
def test_reference_config_builds_models(path):
    from imaginaire_amd.config import Config
    from imaginaire_amd.registry import import_module
    cfg = Config(path)
    for t in (cfg.gen.type, cfg.dis.type):
        rel = t.replace('imaginaire.', '', 1).replace('.', '/') + '.py'
        if path in CONFIGS and t.startswith('imaginaire.') and \
                not os.path.exists(os.path.join(os.path.dirname(REF), 'imaginaire', rel)):
            pytest.skip('%s names %s, which the reference itself does not ship' % (path, t))
    torch.manual_seed(0)
    net_G = import_module(cfg.gen.type).Generator(cfg.gen, cfg.data)
    net_D = import_module(cfg.dis.type).Discriminator(cfg.dis, cfg.data)
    assert sum(p.numel() for p in net_G.parameters()) > 0
    assert sum(p.numel() for p in net_D.parameters()) >= 0
    import_module(cfg.trainer.type)  # the trainer module resolves too
