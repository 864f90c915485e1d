"""ColumnProposal2 at the proposal geometries of the reference's config schema (num_prop 72 / 36 / 18, prop_width 2 / 4 / 8,
dim_shared up to 512), without a GPU: the net builds the reference's state-dict layout for each (golden
tests/golden/g25_propgeom_layout.json, make_golden_propgeom.py), reference checkpoints load strictly, and the head refuses every
other geometry with NotImplementedError before it touches a device."""
import json
import os

import pytest
import torch

from lanemapping_amd import heads as heads_mod
from lanemapping_amd.boundary import build_net_from_config, load_config, load_reference_checkpoint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TAGS = ('c2_p36', 'c2_p18', 'c2_d512', 'mixseg_p36')


def _layouts():
    with open(os.path.join(GOLDEN, 'g25_propgeom_layout.json')) as f:
        return json.load(f)


def build_geometry(config, over, device='cpu'):
    """The repo's config with cfg.heads overridden, as make_golden_propgeom.py builds the reference net."""
    h = dict(load_config(config).heads)
    h.update(over)
    return build_net_from_config(config, device=device, heads=h)


def test_golden_covers_every_geometry():
    assert sorted(_layouts()) == sorted(TAGS)


@pytest.mark.parametrize('tag', TAGS)
def test_state_dict_layout_matches_reference(tag):
    ref = _layouts()[tag]
    net = build_geometry(ref['config'], ref['heads'])
    want = [(k, tuple(s)) for k, s in ref['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(got) == len(want) and dict(got) == dict(want)     # key by key, shape by shape (loading is by key)
    # the geometry-dependent shapes
    h = net.heads
    fw, D = h.prop_width + 2 * h.prop_half_buff, h.dim_shared
    sd = net.state_dict()
    assert tuple(sd['heads.cls2.0.weight'].shape) == (D, 16 * fw, 1)
    assert tuple(sd['heads.cls2.2.weight'].shape) == (fw, D, 1)
    assert tuple(sd['heads.offset2.2.weight'].shape) == (fw, D, 1)
    assert tuple(sd['heads.ext2.2.weight'].shape) == (3, D, 1)
    assert tuple(sd['heads.proposal_confidence.1.weight'].shape) == (2, 16 * fw * 144)
    assert f'heads.emb_{h.num_prop - 1}' in sd and f'heads.emb_{h.num_prop}' not in sd


@pytest.mark.parametrize('tag', TAGS)
def test_reference_checkpoint_loads_strictly(tag, tmp_path):
    from lanemapping_amd import synth
    ref = _layouts()[tag]
    src = build_geometry(ref['config'], ref['heads'])
    synth.fill_module_(src, 2021)
    path = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v for k, v in src.state_dict().items()}, 'epoch': 1}, path)
    dst = build_geometry(ref['config'], ref['heads'])
    res = load_reference_checkpoint(dst, str(path), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    # a checkpoint of another geometry does not load
    other = build_geometry(ref['config'], {'num_prop': 72, 'prop_width': 2, 'dim_shared': 100})
    with pytest.raises(RuntimeError):
        load_reference_checkpoint(other, str(path), strict=True)


@pytest.mark.parametrize('num_prop,prop_width,half_buff,dim_shared', [
    (72, 2, 4, 100), (36, 4, 4, 100), (18, 8, 4, 100), (72, 2, 4, 512), (36, 4, 4, 4), (18, 8, 4, 508)])
def test_supported_geometries_pass_the_check(num_prop, prop_width, half_buff, dim_shared):
    heads_mod.check_geometry(num_prop, prop_width, half_buff, dim_shared)


@pytest.mark.parametrize('num_prop,prop_width,half_buff,dim_shared', [
    (48, 3, 4, 100),     # num_prop * prop_width = 144, not a supported pair
    (72, 4, 4, 100),     # 288 columns
    (36, 2, 4, 100),     # 72 columns
    (72, 2, 3, 100),     # half_buff 3: FW 8
    (36, 4, 2, 100),     # FW 8
    (18, 8, 5, 100),     # FW 18
    (72, 2, 4, 516),     # dim_shared above 512
    (72, 2, 4, 102),     # not a multiple of 4
    (36, 4, 4, 0),
])
@pytest.mark.parametrize('config', ['Proj_polyline_fpn_vit_vertex_2', 'Proj_polyline_fpn_mixseg_vertex'])
def test_unsupported_geometry_refused_before_the_device(config, num_prop, prop_width, half_buff, dim_shared, monkeypatch):
    """The refusal names the supported set and comes before any kernel: the library is made unreachable, and CPU tensors would be
    refused by it anyway."""
    from lanemapping_amd import ops

    def no_device(*a, **k):
        raise AssertionError('a device call was made before the geometry check')
    monkeypatch.setattr(ops, 'lib', no_device)
    monkeypatch.setattr(ops, 'new_act', no_device)
    net = build_geometry(config, dict(num_prop=num_prop, prop_width=prop_width, prop_half_buff=half_buff, dim_shared=dim_shared))
    x, x_up = torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288)
    with pytest.raises(NotImplementedError, match=r'\(72, 2\), \(36, 4\), \(18, 8\)'):
        net.heads._forward_impl(x, x_up)


@pytest.mark.parametrize('tag', TAGS)
def test_supported_geometry_gets_past_the_check(tag):
    """A supported geometry is not refused: on CPU tensors it fails later, in the library (never a fallback)."""
    ref = _layouts()[tag]
    net = build_geometry(ref['config'], ref['heads'])
    x, x_up = torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288)
    with pytest.raises(Exception) as e:
        net.heads._forward_impl(x, x_up)
    assert not isinstance(e.value, NotImplementedError), e.value
