"""MLP-Mixer lane config (configs/Proj_polyline_fpn_mixseg_vertex.py) at the boundary, without a GPU: the net builds through the
registries with the reference's state-dict layout (golden G24, tests/golden/make_golden_mixseg.py), reference checkpoints load
strictly, and the head accepts spatial_att=False while the unsupported column branches stay refused."""
import json
import os

import pytest
import torch

from lanemapping_amd.boundary import build_net_from_config, load_config, load_reference_checkpoint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAME = 'Proj_polyline_fpn_mixseg_vertex'


def _g24():
    with open(os.path.join(GOLDEN, 'g24_mixseg_layout.json')) as f:
        return json.load(f)[NAME]


def _check_layout(net, cfg, ref):
    a = [(k, tuple(s)) for k, s in ref['state_dict']]
    b = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert a == b and len(a) > 300
    assert ref['dataset_test'] == dict(cfg.dataset.test) and ref['train_type'] == cfg.dataset.train.type
    e = ref['entry']
    assert (e['log_dir'], e['batch_size'], e['seed'], e['validate_buffer']) == (cfg.log_dir, cfg.batch_size, cfg.seed, cfg.validate_buffer)


def test_repo_config_builds_the_reference_layout():
    """G24 holds what the reference's UNMODIFIED config builds through the boundary (checked there against the reference net's own
    state dict); the repo's trimmed config must give the same."""
    ref = _g24()
    net = build_net_from_config(NAME, device='cpu')
    _check_layout(net, load_config(NAME), ref)
    sd = net.state_dict()
    # the Mixer's parameter names and shapes (mixsegnet.py:55-66 at image_size 144, patch 8, dim 512, depth 3, 8 outputs)
    assert tuple(sd['backbone.mixsegnet.1.weight'].shape) == (512, 4096)
    for blk in (2, 3, 4):
        assert tuple(sd[f'backbone.mixsegnet.{blk}.0.fn.0.weight'].shape) == (1296, 324, 1)
        assert tuple(sd[f'backbone.mixsegnet.{blk}.0.fn.3.weight'].shape) == (324, 1296, 1)
        assert tuple(sd[f'backbone.mixsegnet.{blk}.0.fn.0.bias'].shape) == (1296,)
        assert tuple(sd[f'backbone.mixsegnet.{blk}.1.fn.0.weight'].shape) == (2048, 512)
        assert tuple(sd[f'backbone.mixsegnet.{blk}.1.norm.weight'].shape) == (512,)
    assert tuple(sd['backbone.mixsegnet.5.weight'].shape) == (512,)
    assert tuple(sd['backbone.mixsegnet.7.weight'].shape) == (8, 8, 1, 1)
    assert 'heads.bi_seg_proposal.weight' in sd
    assert not any(k.startswith('backbone.mixsegnet.6.') or k.startswith('backbone.mixsegnet.0.') for k in sd)


def test_reference_checkpoint_loads_strictly(tmp_path):
    from lanemapping_amd import synth
    src = build_net_from_config(NAME, device='cpu')
    synth.fill_module_(src, 2021)
    path = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v for k, v in src.state_dict().items()}, 'epoch': 1}, path)
    dst = build_net_from_config(NAME, device='cpu')
    res = load_reference_checkpoint(dst, str(path), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    # a missing key is still an error
    sd = {'module.' + k: v for k, v in src.state_dict().items() if k != 'backbone.mixsegnet.3.0.fn.3.bias'}
    torch.save({'net': sd}, path)
    with pytest.raises(RuntimeError):
        load_reference_checkpoint(dst, str(path), strict=True)


def test_spatial_att_false_accepted_column_att_refused():
    """spatial_att=False gets past the head's configuration checks (then needs a device: the CPU tensors are refused by the library),
    column_att=True is still refused before anything runs."""
    net = build_net_from_config(NAME, device='cpu')
    head = net.heads
    x, x_up = torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288)
    assert head.cfg.spatial_att is False
    with pytest.raises(Exception) as e:          # (no device here, or CPU tensors refused by the library: never a fallback)
        head._forward_impl(x, x_up)
    assert not isinstance(e.value, NotImplementedError), e.value
    head.cfg.column_att = True
    try:
        with pytest.raises(NotImplementedError, match='column_att'):
            head._forward_impl(x, x_up)
    finally:
        head.cfg.column_att = False
