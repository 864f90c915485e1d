"""GPU tests (-m gpu): the RowSharNotReducRef head (config 4) at `off_grid` 1..4 and with `is_reuse_same_network`.

  1 / 2  lm_rowref_gather_win / lm_rowref_scatter_win, bit-exact against plain Python loops, in guarded slabs (tests/guards.py): the
         token buffer / the output map are pre-filled with a canary pattern, every logical element must be overwritten and nothing
         outside them may change; the inputs carry NaN guards;
  3      lm_rowref_gather / lm_rowref_scatter == the off_grid = 2 call of the new entries, bit for bit, at config 4's sizes;
  4      the head against oracle/rowref_ref.py on CPU at off_grid 1, 3, 4 with separate and with reused second-stage networks;
  5      TilePipeline, eager and captured, on the config-4 net with off_grid = 3 and reused networks.
"""
import numpy as np
import pytest
import torch

import cases
from gpu_common import _chk, _close, _lib, _s
from guards import NAN, Slab
from lanemapping_amd import synth

pytestmark = pytest.mark.gpu

CONFIG4 = 'Proj28_GFC-T3_RowRef_82_73_laser'
CF = 8


# ================================================================================ 1 / 2. window kernels against plain loops
def _gather_ref(x, corr, L, og):
    """x [B,H,W,8], corr [B,L,H] -> tok [B*L, 8*H*KW]: tok[t][(cf*H + h)*KW + j] = x_pad[b, cf, h, corr + j] over a zero-padded copy."""
    B, H, W, _ = x.shape
    KW = 2 * og + 1
    pad = np.zeros((B, H, W + 2 * og, CF), dtype=np.float32)
    pad[:, :, og:og + W] = x
    tok = np.full((B * L, CF * H * KW), np.float32(NAN))
    for b in range(B):
        for c in range(L):
            for h in range(H):
                for j in range(KW):
                    for cf in range(CF):
                        tok[b * L + c, (cf * H + h) * KW + j] = pad[b, h, corr[b, c, h] + j, cf]
    return tok


def _scatter_ref(x, tok, corr, valid, og):
    """The reference's write-back (:227-230): the selected lanes of a tile in lane order, number n on rows h < H-1-n only (the loop
    variable it leaks shrinks the range by one per lane), later lanes over earlier ones; window entries outside [0, W) have no pixel."""
    B, H, W, _ = x.shape
    L = valid.shape[1]
    KW = 2 * og + 1
    y = x.copy()
    for b in range(B):
        n = 0
        for c in range(L):
            if not valid[b, c]:
                continue
            t = tok[b * L + c].reshape(CF, H, KW)
            for h in range(max(H - 1 - n, 0)):
                for j in range(KW):
                    w = corr[b, c, h] + j - og
                    if 0 <= w < W:
                        y[b, h, w, :] = t[:, h, j]
            n += 1
    return y


def _corr(B, L, H, W, g):
    """Arg-max columns that hit both borders: lane 0 walks 0, W-1, 0, ...; lane 1 the other way round; the rest are random."""
    corr = torch.randint(0, W, (B, L, H), generator=g, dtype=torch.int32)
    ends = torch.tensor([0, W - 1], dtype=torch.int32).repeat(H // 2 + 1)
    corr[:, 0, :] = ends[:H]
    corr[:, 1, :] = ends[1:H + 1]
    return corr


def _in_slab(dev, data, rows, width, dtype=torch.float32, pad=NAN):
    return Slab(dev, rows, width, front=2, back=2, dtype=dtype).fill_input(data, pad)


GATHER_CASES = [(2, 6, 9, 3, 1), (2, 6, 9, 3, 2), (2, 6, 9, 3, 3), (2, 6, 9, 3, 4), (2, 6, 3, 3, 4)]      # the last: window wider than the row


@pytest.mark.parametrize('B,H,W,L,og', GATHER_CASES)
def test_gather_win_bit_exact(dev, B, H, W, L, og):
    """lm_rowref_gather_win against a plain loop over a zero-padded copy; corr includes 0 and W-1, so windows run off both borders
    (W = 3 with off_grid = 4: off both at once).  The token slab starts as canaries between canary guards: every one of the
    B*L*8*H*KW floats is overwritten, no word beyond them changes."""
    KW = 2 * og + 1
    g = torch.Generator().manual_seed(100 * W + og)
    x = torch.randn(B, H, W, CF, generator=g)
    corr = _corr(B, L, H, W, g)
    assert int(corr.min()) == 0 and int(corr.max()) == W - 1
    want = _gather_ref(x.numpy(), corr.numpy(), L, og)
    xs = _in_slab(dev, x, B * H * W, CF)
    cs = _in_slab(dev, corr, B * L, H, dtype=torch.int32, pad=0)
    tok = Slab(dev, B * L, CF * H * KW, front=2, back=2).fill_canary()
    _chk(_lib().lm_rowref_gather_win(_s(), xs.ptr(), cs.ptr(), tok.ptr(), B, H, W, L, og))
    torch.cuda.synchronize()
    tok.check_canary(f'gather_win off_grid={og} W={W}')
    assert np.array_equal(tok.view.cpu().numpy().view(np.int32), want.view(np.int32))
    # lane 0, row 0 has corr = 0: the first off_grid window entries are off the left border and read as zero
    assert float(tok.view.cpu().view(B * L, CF, H, KW)[0, :, 0, :og].abs().max()) == 0.0


@pytest.mark.parametrize('B,H,W,L,og', GATHER_CASES)
def test_scatter_win_bit_exact(dev, B, H, W, L, og):
    """lm_rowref_scatter_win against a loop restating the shrinking range: tile 0 with all L lanes selected and overlapping windows
    (the last covering lane wins; lane n stops at row H-1-n), tile 1 with none (an exact copy of x).  y starts as canaries between
    canary guards; x and tok carry NaN guards."""
    KW = 2 * og + 1
    g = torch.Generator().manual_seed(200 * W + og)
    x = torch.randn(B, H, W, CF, generator=g)
    tok = torch.randn(B * L, CF * H * KW, generator=g)
    corr = _corr(B, L, H, W, g)
    near = corr[:, 1, :] + torch.randint(-1, 2, (B, H), generator=g, dtype=torch.int32)
    corr[:, 2, :] = near.clamp(0, W - 1)                          # lane 2 within one column of lane 1: their windows overlap on every row
    valid = torch.zeros(B, L, dtype=torch.int32)
    valid[0] = 1
    want = _scatter_ref(x.numpy(), tok.numpy(), corr.numpy(), valid.numpy(), og)
    # the case exercises what it claims: rows H-1-n .. H-1 of tile 0 keep x under lane n's window, and some pixel is covered by two lanes
    assert np.array_equal(want[0, H - 1], x.numpy()[0, H - 1]) and not np.array_equal(want[0, 0], x.numpy()[0, 0])
    cover = np.zeros((H, W), dtype=int)
    for c in range(L):
        for h in range(H - 1 - c):
            lo = int(corr[0, c, h]) - og
            cover[h, max(lo, 0):max(min(lo + KW, W), 0)] += 1
    assert cover.max() >= 2
    xs = _in_slab(dev, x, B * H * W, CF)
    ts = _in_slab(dev, tok, B * L, CF * H * KW)
    cs = _in_slab(dev, corr, B * L, H, dtype=torch.int32, pad=0)
    vs = _in_slab(dev, valid, B, L, dtype=torch.int32, pad=0)
    y = Slab(dev, B * H * W, CF, front=2, back=2).fill_canary()
    _chk(_lib().lm_rowref_scatter_win(_s(), xs.ptr(), ts.ptr(), cs.ptr(), vs.ptr(), y.ptr(), B, H, W, L, og))
    torch.cuda.synchronize()
    y.check_canary(f'scatter_win off_grid={og} W={W}')
    got = y.view.cpu().numpy().reshape(B, H, W, CF)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[1].view(np.int32), x.numpy()[1].view(np.int32)), 'no lane selected: y must equal x'


@pytest.mark.parametrize('og', [0, 5, -1])
def test_window_entries_refuse_other_off_grid(dev, og):
    z = torch.zeros(CF * 4 * 9 * 2, device=dev)
    iz = torch.zeros(8, device=dev, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='rowref_gather_win: off_grid'):
        _chk(_lib().lm_rowref_gather_win(_s(), z.data_ptr(), iz.data_ptr(), z.data_ptr(), 1, 2, 2, 1, og))
    with pytest.raises(RuntimeError, match='rowref_scatter_win: off_grid'):
        _chk(_lib().lm_rowref_scatter_win(_s(), z.data_ptr(), z.data_ptr(), iz.data_ptr(), iz.data_ptr(), z.data_ptr(), 1, 2, 2, 1, og))


# ================================================================================ 3. the old entries are the off_grid = 2 call
def test_old_entries_equal_off_grid_2(dev):
    """Random input at config 4's own sizes: lm_rowref_gather == lm_rowref_gather_win(off_grid=2) and lm_rowref_scatter ==
    lm_rowref_scatter_win(off_grid=2), bit for bit."""
    from lanemapping_amd import ops
    B, H, W, L = 2, 144, 144, 12
    g = torch.Generator().manual_seed(52)
    x = torch.randn(B, H, W, CF, generator=g).to(dev)
    corr = _corr(B, L, H, W, g).to(dev)
    tok = torch.randn(B * L, CF * H * 5, generator=g).to(dev)
    valid = (torch.rand(B, L, generator=g) < 0.6).int()
    valid[0, :3] = 1
    valid = valid.to(dev)
    t_old, t_new = torch.full_like(tok, 9.0), torch.full_like(tok, 7.0)
    _chk(_lib().lm_rowref_gather(_s(), ops._ptr(x), ops._ptr(corr), ops._ptr(t_old), B, H, W, L))
    _chk(_lib().lm_rowref_gather_win(_s(), ops._ptr(x), ops._ptr(corr), ops._ptr(t_new), B, H, W, L, 2))
    assert torch.equal(t_old, t_new)
    y_old, y_new = torch.full_like(x, 9.0), torch.full_like(x, 7.0)
    _chk(_lib().lm_rowref_scatter(_s(), ops._ptr(x), ops._ptr(tok), ops._ptr(corr), ops._ptr(valid), ops._ptr(y_old), B, H, W, L))
    _chk(_lib().lm_rowref_scatter_win(_s(), ops._ptr(x), ops._ptr(tok), ops._ptr(corr), ops._ptr(valid), ops._ptr(y_new), B, H, W, L, 2))
    assert torch.equal(y_old, y_new) and not torch.equal(y_old, x)


# ================================================================================ 4. the head against the oracle
SMALL = dict(dim_shared=128, dim_token=256, tr_heads=4, tr_dim_head=64, tr_mlp_dim=512)
THR_EXT = 0.5          # the seeded lane means straddle 0.5 (at config 4's 0.3 every lane is selected)
SEED = 2026            # picked on the CPU: the first of 2021.. at which the oracle meets the conditions asserted in _oracle_case
CLS_GAIN = 4.0         # on cls_c's second convolution: at gain 1 the softmax over 144 columns is so flat that among the 3456 first-stage
                       # rows some top-two gap falls under 1e-4 at every seed


def _small_head(off_grid, reuse):
    from lanemapping_amd.boundary import load_config
    from lanemapping_amd.registry import build_heads
    cfg = load_config(CONFIG4)
    cfg.heads = dict(cfg.heads, off_grid=off_grid, is_reuse_same_network=reuse, thr_ext=THR_EXT, **SMALL)
    head = build_heads(cfg).eval()
    synth.fill_module_(head, SEED, prefix='heads.')
    synth.apply_gains_(head, {f'cls_{c}.2.weight': CLS_GAIN for c in range(12)})
    head.set_lane_embeddings([torch.from_numpy(0.1 * synth.normalish(SEED, SMALL['dim_token'], 100 + c)).float() for c in range(12)])
    return head


def _oracle_case(off_grid, reuse):
    """(head on CPU, input, oracle output, oracle lane selection).  The oracle's discrete decisions must be clear of ties, or the
    comparison would test rounding: asserted here, so a bad seed fails loudly."""
    from oracle import rowref_ref
    head = _small_head(off_grid, reuse)
    sd = {'heads.' + k: v.clone() for k, v in head.state_dict().items()}
    for c in range(12):
        sd[f'heads.emb_{c}'] = getattr(head, f'emb_{c}').clone()
    if reuse:                                                       # the second stage of the oracle reads ext2_c / cls2_c: alias them
        assert not any(k.startswith(('heads.ext2_', 'heads.cls2_')) for k in sd)
        for k in [k for k in sd if k.startswith(('heads.ext_', 'heads.cls_'))]:
            name, rest = k[len('heads.'):].split('_', 1)
            sd[f'heads.{name}2_{rest}'] = sd[k]
    x = torch.from_numpy(cases.head_inputs(SEED, batch=2)[0])
    with torch.no_grad():
        ref = rowref_ref.rowref_forward(sd, x, thr_ext=THR_EXT, off_grid=off_grid, heads=SMALL['tr_heads'], dim_head=SMALL['tr_dim_head'])
    means = torch.stack([ref[f'ext_{c}'][:, :, 0].mean(dim=1) for c in range(12)], dim=1)                       # [B, L]
    assert float((means - THR_EXT).abs().min()) >= 1e-3, 'a lane mean within 1e-3 of thr_ext: pick another seed'
    top2 = torch.stack([torch.topk(ref[f'cls_{c}'], 2, dim=2).values for c in range(12)])
    assert float((top2[..., 0] - top2[..., 1]).min()) > 1e-4, 'a first-stage top-two cls gap <= 1e-4: pick another seed'
    sel = means > THR_EXT
    assert int(sel.sum(dim=1).min()) >= 3 and int((~sel).sum(dim=1).min()) >= 1, f'selected lanes per tile {sel.sum(dim=1).tolist()}'
    assert not torch.equal(ref['_refined'], x)
    return head, x, ref, sel


@pytest.mark.parametrize('reuse', [False, True])
@pytest.mark.parametrize('off_grid', [1, 3, 4])
def test_head_vs_oracle(dev, off_grid, reuse):
    """B = 2, row_size = 144, seeded weights at dim_shared=128, dim_token=256, tr_heads=4, tr_mlp_dim=512 (the head accepts them), against
    oracle.rowref_ref.rowref_forward on CPU with the same off_grid / heads / dim_head; for reused networks the oracle's state dict
    aliases ext2_c / cls2_c to ext_c / cls_c.  ext2, cls2 and the refined feature map with the helper and the 1e-4 of
    test_rowref_head_golden_g8; lane selection and first-stage arg-max columns exactly (the oracle is kept clear of ties)."""
    head, x, ref, sel = _oracle_case(off_grid, reuse)
    head = head.to(dev)
    with torch.no_grad():
        out = head(x.to(dev))
        assert np.array_equal(head._last['selected'], sel.numpy())
        for c in range(12):
            assert torch.equal(out[f'cls_{c}'].argmax(dim=2).cpu(), ref[f'cls_{c}'].argmax(dim=2)), f'cls_{c} argmax'
            _close(out[f'ext_{c}'], ref[f'ext_{c}'], 1e-4, f'ext_{c}')
            _close(out[f'ext2_{c}'], ref[f'ext2_{c}'], 1e-4, f'ext2_{c}')
            _close(out[f'cls2_{c}'], ref[f'cls2_{c}'], 1e-4, f'cls2_{c}')
        _close(head._last['refined'], ref['_refined'], 1e-4, 'refined feature map')
        assert any(k.startswith('s2.') for k in head.packed()) != reuse      # reused networks: one packed copy, the first stage's
        col = head.decode_columns(out)
        dec = head.get_exist_coor_endp_dict(out)
    assert tuple(col.shape) == (2, 12, 144) and tuple(dec['cls'].shape) == (2, 13, 144, 144)
    lines = head.predict_lines()
    for b in range(2):
        assert np.array_equal(lines[b], head.lines_from_columns(col[b].cpu().numpy(), 144))


# ================================================================================ 5. tile pipeline
def test_pipeline_off_grid_3_reused_networks(dev):
    """The config-4 net with heads.off_grid = 3 and is_reuse_same_network = True through TilePipeline on B = 2 synthetic tiles: the
    captured graph replays bit-identically to the eager launches, and the lanes are lines_from_columns of the eager head's columns."""
    from lanemapping_amd.boundary import build_net_from_config, load_config
    from lanemapping_amd.pipeline import TilePipeline
    heads_cfg = dict(load_config(CONFIG4).heads, off_grid=3, is_reuse_same_network=True)
    net = build_net_from_config(CONFIG4, device='cpu', heads=heads_cfg)
    assert net.heads.off_grid == 3 and net.heads.is_reuse_same_network and not hasattr(net.heads, 'ext2_0')
    synth.fill_module_(net, 2021)
    net = net.to(dev)
    eager, graph = TilePipeline(net, use_graph=False), TilePipeline(net, use_graph=True)
    x = torch.from_numpy(synth.bev_batch([2021, 2022], 1152)).to(dev)
    want = eager.run_batch(x)
    got = graph.run_batch(x)
    again = graph.run_batch(x)
    assert len(want) == len(got) == len(again) == 2
    for (la, ea), (lb, eb), (lc, ec) in zip(want, got, again):
        assert np.array_equal(np.asarray(la), np.asarray(lb)) and np.array_equal(np.asarray(ea), np.asarray(eb))
        assert np.array_equal(np.asarray(la), np.asarray(lc)) and np.array_equal(np.asarray(ea), np.asarray(ec))
    assert len(graph._graphs) == 1
    with torch.no_grad():
        raw = net.forward_raw({'proj': x})
        col = net.heads.decode_columns(raw).cpu().numpy()
    assert (col >= 0).any()
    for b in range(2):
        cols = net.heads.lines_from_columns(col[b], 144)
        lanes = np.asarray(want[b][0])
        assert lanes.shape == (72, 144, 2)
        assert np.array_equal(lanes[:12, :, 0], cols) and np.array_equal(lanes[:12, :, 1], (cols > 0).astype(np.float64))
        assert np.all(lanes[12:, :, 0] == -1.0) and np.all(lanes[12:, :, 1] == 0.0)
