"""CPU: the RowSharNotReducRef head (config 4) at every accepted geometry - `off_grid` 1..4, `is_reuse_same_network` False / True.

The state-dict layouts are held to tests/golden/rowref_geometry_keys.json (make_golden_rowref_geometry.py: what the reference's module
builds for the same keyword arguments, names and shapes), so a reference checkpoint of any of these settings loads strictly."""
import json
import os

import pytest
import torch

from lanemapping_amd import rowref
from lanemapping_amd.boundary import build_net_from_config, load_config
from lanemapping_amd.registry import build_heads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CONFIG4 = 'Proj28_GFC-T3_RowRef_82_73_laser'


@pytest.fixture(scope='module')
def layouts():
    with open(os.path.join(GOLDEN, 'rowref_geometry_keys.json')) as f:
        return json.load(f)


def _head(**over):
    cfg = load_config(CONFIG4)
    cfg.heads = dict(cfg.heads, **over)
    return build_heads(cfg).eval()


def test_fixture_covers_every_setting(layouts):
    assert sorted(layouts) == sorted(f'og{og}_reuse{r}' for og in (1, 2, 3, 4) for r in (0, 1))
    for tag, ent in layouts.items():
        assert tag == f'og{ent["off_grid"]}_reuse{int(ent["is_reuse_same_network"])}'


@pytest.mark.parametrize('reuse', [False, True])
@pytest.mark.parametrize('off_grid', [1, 2, 3, 4])
def test_head_builds_with_the_reference_layout(layouts, off_grid, reuse):
    head = _head(off_grid=off_grid, is_reuse_same_network=reuse)
    ref = {k: tuple(s) for k, s in layouts[f'og{off_grid}_reuse{int(reuse)}']['state_dict']}
    own = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert own == ref
    in_tok = (2 * off_grid + 1) * 144 * 8
    assert in_tok == {1: 3456, 2: 5760, 3: 8064, 4: 10368}[off_grid] and in_tok % 32 == 0
    assert own['to_token.1.weight'] == (1024, in_tok) and own['tr_lane_correlator.2.weight'] == (in_tok, 1024)
    assert any(k.startswith(('ext2_', 'cls2_')) for k in own) != reuse
    if reuse:
        assert not any(n.startswith(('ext2_', 'cls2_')) for n, _ in head.named_parameters())
    assert head.off_grid == off_grid and head.is_reuse_same_network is reuse
    # strict loading of a checkpoint with exactly the reference's keys
    sd = {k: torch.zeros(s) for k, s in ref.items()}
    res = head.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_reuse_checkpoint_is_refused_by_the_separate_head_and_vice_versa(layouts):
    """The two settings really have different layouts: strict loading across them fails."""
    sd_reuse = {k: torch.zeros(s) for k, s in layouts['og2_reuse1']['state_dict']}
    with pytest.raises(RuntimeError, match='Missing key'):
        _head(is_reuse_same_network=False).load_state_dict(sd_reuse, strict=True)
    sd_sep = {k: torch.zeros(s) for k, s in layouts['og2_reuse0']['state_dict']}
    with pytest.raises(RuntimeError, match='Unexpected key'):
        _head(is_reuse_same_network=True).load_state_dict(sd_sep, strict=True)


@pytest.mark.parametrize('over,name', [(dict(off_grid=0), 'off_grid=0'), (dict(off_grid=5), 'off_grid=5'), (dict(dim_feat=16), 'dim_feat=16')])
def test_refused_geometries_name_the_parameter(over, name):
    with pytest.raises(NotImplementedError, match=name):
        _head(**over)
    with pytest.raises(NotImplementedError, match=name):
        rowref.check_geometry(over.get('dim_feat', 8), over.get('off_grid', 2))


def test_check_geometry_accepts_every_listed_setting():
    for og in (1, 2, 3, 4):
        rowref.check_geometry(8, og)


def test_trimmed_config4_builds_the_same_keys_as_before(layouts):
    """The repo's config 4 (off_grid=2, separate second-stage networks) keeps its 449 head entries, in the reference's order."""
    net = build_net_from_config(CONFIG4, device='cpu')
    own = [(k[len('heads.'):], tuple(v.shape)) for k, v in net.state_dict().items() if k.startswith('heads.')]
    assert own == [(k, tuple(s)) for k, s in layouts['og2_reuse0']['state_dict']] and len(own) == 449
    assert net.heads.off_grid == 2 and net.heads.is_reuse_same_network is False
