"""VitSegNet (GFC-T) at the patch sizes of the reference's config schema (square patches 4 / 6 / 8 / 12 / 16, dim a multiple of
32 and of patch^2 up to 4096 but 768, dim_head 64), without a GPU: the net builds the reference's state-dict layout for each geometry (golden
tests/golden/g26_vitgeom_layout.json, make_golden_vitgeom.py), reference checkpoints load strictly, and the backbone refuses every
other geometry with NotImplementedError before it touches a device."""
import json
import os

import pytest
import torch

from lanemapping_amd import backbone as backbone_mod
from lanemapping_amd.boundary import build_net_from_config, load_config, load_reference_checkpoint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CONFIG2 = 'Proj_polyline_fpn_vit_vertex_2'
TAGS = ('p4', 'p6', 'p12', 'p16', 'p4_mlp')


def _layouts():
    with open(os.path.join(GOLDEN, 'g26_vitgeom_layout.json')) as f:
        return json.load(f)


def build_geometry(over, config=CONFIG2, device='cpu'):
    """The repo's config with cfg.backbone overridden, as make_golden_vitgeom.py builds the reference net."""
    b = dict(load_config(config).backbone)
    b.update(over)
    return build_net_from_config(config, device=device, backbone=b)


def test_golden_covers_every_geometry():
    assert sorted(_layouts()) == sorted(TAGS)


@pytest.mark.parametrize('tag', TAGS)
def test_state_dict_layout_matches_reference(tag):
    ref = _layouts()[tag]
    net = build_geometry(ref['backbone'], ref['config'])
    want = [(k, tuple(s)) for k, s in ref['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(got) == len(want) and dict(got) == dict(want)
    assert [e for e in got if e[0].startswith('backbone.')] == [e for e in want if e[0].startswith('backbone.')], 'backbone order'
    p, dim = ref['backbone']['patch_h_size'], ref['backbone']['dim']
    sd = net.state_dict()
    assert tuple(sd['backbone.to_patch_embedding.1.weight'].shape) == (dim, 64 * p * p)
    assert tuple(sd['backbone.pos_embedding'].shape) == (1, (144 // p) ** 2, dim)
    assert ('backbone.shared_mlp.weight' in sd) == bool(ref['backbone'].get('is_with_shared_mlp', False))


@pytest.mark.parametrize('tag', TAGS)
def test_reference_checkpoint_loads_strictly(tag, tmp_path):
    from lanemapping_amd import synth
    ref = _layouts()[tag]
    src = build_geometry(ref['backbone'], ref['config'])
    synth.fill_module_(src, 2021)
    path = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v for k, v in src.state_dict().items()}, 'epoch': 1}, path)
    dst = build_geometry(ref['backbone'], ref['config'])
    res = load_reference_checkpoint(dst, str(path), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    other = build_geometry({})                      # the shipped patch-8 geometry does not take it
    with pytest.raises(RuntimeError):
        load_reference_checkpoint(other, str(path), strict=True)


@pytest.mark.parametrize('over', [
    dict(patch_h_size=4, patch_w_size=4, dim=128), dict(patch_h_size=6, patch_w_size=6, dim=288),
    dict(patch_h_size=12, patch_w_size=12, dim=1152), dict(patch_h_size=16, patch_w_size=16, dim=2048),
    dict(patch_h_size=4, patch_w_size=4, dim=512, is_with_shared_mlp=True), dict(), dict(dim=1024),
    dict(patch_h_size=4, patch_w_size=4, dim=4096, heads=1, expansion_factor=0.5), dict(heads=3, depth=1, expansion_factor=1.5)])
def test_supported_geometries_pass_the_check(over):
    b = build_geometry(over).backbone
    backbone_mod.check_vit_geometry(b.patch, b.dim, b.is_with_shared_mlp,
                                    [(a.fn.heads, a.fn.dim_head, f.fn.net[0].out_features) for a, f in b.transformer.layers])


@pytest.mark.parametrize('over', [
    dict(patch_h_size=2, patch_w_size=2, dim=512),             # patch 2: not in the set
    dict(patch_h_size=3, patch_w_size=3, dim=576),             # patch 3
    dict(patch_h_size=9, patch_w_size=9, dim=648),             # patch 9
    dict(patch_h_size=4, patch_w_size=4, dim=136),             # not a multiple of 32
    dict(patch_h_size=6, patch_w_size=6, dim=144),             # 144 % 32 != 0
    dict(patch_h_size=12, patch_w_size=12, dim=160),           # not a multiple of patch^2
    dict(patch_h_size=4, patch_w_size=4, dim=4128),            # above 4096
    dict(patch_h_size=4, patch_w_size=4, dim=768),             # LayerNorm keeps refusing D = 768
    dict(dim_head=32),
    dict(expansion_factor=1.01),                               # mlp_dim 517
    dict(is_with_shared_mlp=True),                             # 512 / 64 = 8 channels into the 1x1 MLP
    dict(patch_h_size=4, patch_w_size=4, dim=64, heads=1),     # heads = 1 with dim_head = dim: no to_out
])
def test_unsupported_geometry_refused_before_the_device(over, monkeypatch):
    """The refusal names the supported set and comes before any kernel: the library is made unreachable, and CPU tensors would be
    refused by it anyway."""
    from lanemapping_amd import ops

    def no_device(*a, **k):
        raise AssertionError('a device call was made before the geometry check')
    monkeypatch.setattr(ops, 'lib', no_device)
    monkeypatch.setattr(ops, 'new_act', no_device)
    net = build_geometry(over)
    with pytest.raises(NotImplementedError, match=r'square patches in \[4, 6, 8, 12, 16\]'):
        net.backbone._forward_impl(torch.zeros(1, 64, 144, 144))


@pytest.mark.parametrize('p_h,p_w', [(8, 4), (4, 8), (6, 12)])
def test_non_square_patches_still_refused(p_h, p_w):
    with pytest.raises(NotImplementedError, match='square patches only'):
        build_geometry(dict(patch_h_size=p_h, patch_w_size=p_w, dim=512))


@pytest.mark.parametrize('tag', TAGS)
def test_supported_geometry_gets_past_the_check(tag):
    """A supported geometry is not refused: on CPU tensors it fails later, in the library (never a fallback)."""
    ref = _layouts()[tag]
    net = build_geometry(ref['backbone'], ref['config'])
    with pytest.raises(Exception) as e:
        net.backbone._forward_impl(torch.zeros(1, 64, 144, 144))
    assert not isinstance(e.value, NotImplementedError), e.value


@pytest.mark.parametrize('tag', TAGS)
def test_vit_backbone_fake_shape(tag):
    """The stage op's fake kernel: [B, 8, 144, 144] channels-last at every G26 geometry (the head's input)."""
    from lanemapping_amd import torch_ops
    ref = _layouts()[tag]
    bb = build_geometry(ref['backbone'], ref['config']).backbone
    y = torch_ops._vit_backbone_fake(torch.zeros(3, 64, 144, 144), [], torch_ops.stage_name(bb))
    assert tuple(y.shape) == (3, 8, 144, 144) and y.stride(1) == 1
