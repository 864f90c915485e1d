"""GFC-T / ViT block behind the reference's BACKBONE registry name ``VitSegNet``, and its MLP-Mixer variant ``MixSegNet``.

Drop-in for baseline/models/backbone/vitsegnet.py:132-214 (same kwargs, same state-dict keys:
``to_patch_embedding.1``, ``pos_embedding``, ``transformer.layers.{l}.{0,1}.{norm,fn...}``).
Geometries: square patches 4 / 6 / 8 / 12 / 16 (check_vit_geometry).
Kernels: patch embedding = pxp/stride-p implicit GEMM straight from the NHWC feature map (no patchify
copy) with the positional embedding added in the epilogue; LayerNorm rows; QKV / out-proj / MLP GEMMs
on lm_conv2d_nhwc_mfma_f32 with bias + residual + erf-GELU epilogues; lm_attention_f32.

MixSegNet: drop-in for baseline/models/backbone/mixsegnet.py:34-76 (same kwargs, same state-dict keys
``mixsegnet.{1, 2..depth+1, depth+2, depth+4}``).  Same patch embedding (no positional embedding), channel mixing on the
ViT's GEMM epilogues, token mixing (Conv1d over the token axis, weight on the left) on lm_token_mix_mfma_f32 straight from
the [B*tokens, dim] rows, final LayerNorm, un-patchify, the 1x1 output conv on lm_conv2d_nhwc_small.
"""
import torch
import torch.nn as nn

from . import ops
from .registry import BACKBONE
from .packing import PackedModule


class _PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class _Attention(nn.Module):
    def __init__(self, dim, heads, dim_head):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.dim_head, self.scale = heads, dim_head, dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(0.)) if not (heads == 1 and dim_head == dim) else nn.Identity()


class _FeedForward(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(), nn.Dropout(0.), nn.Linear(hidden, dim), nn.Dropout(0.))


class _Transformer(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim):
        super().__init__()
        self.layers = nn.ModuleList([nn.ModuleList([_PreNorm(dim, _Attention(dim, heads, dim_head)),
                                                    _PreNorm(dim, _FeedForward(dim, mlp_dim))]) for _ in range(depth)])


def transformer_forward(layers, P, prefix, t, B, N, valid=None):
    """t [B*N, dim] -> [B*N, dim]; pre-norm blocks `x = attn(x) + x; x = ff(x) + x` (vitsegnet.py:79-83).  valid: key mask of the
    attention core (ops.attention); everything else is row-wise, rows of unflagged tokens are computed and ignored by the caller."""
    for l, (attn, ff) in enumerate(layers):
        k = f'{prefix}{l}'
        y = ops.layernorm(t, P[k + '.ln1.g'], P[k + '.ln1.b'], attn.norm.eps)
        qkv = ops.linear_mfma(y, P[k + '.qkv'], attn.fn.to_qkv.out_features)
        o = ops.attention(qkv, B, N, attn.fn.heads, attn.fn.dim_head, attn.fn.scale, valid=valid)
        t = ops.linear_mfma(o, P[k + '.proj'], t.shape[1], shift=P[k + '.proj.b'], res=t)
        y = ops.layernorm(t, P[k + '.ln2.g'], P[k + '.ln2.b'], ff.norm.eps)
        y = ops.linear_mfma(y, P[k + '.fc1'], ff.fn.net[0].out_features, shift=P[k + '.fc1.b'], act=ops.ACT_GELU)
        t = ops.linear_mfma(y, P[k + '.fc2'], t.shape[1], shift=P[k + '.fc2.b'], res=t)
    return t


def pack_transformer(layers, P, prefix):
    for l, (attn, ff) in enumerate(layers):
        k = f'{prefix}{l}'
        P[k + '.ln1.g'], P[k + '.ln1.b'] = attn.norm.weight.float().contiguous(), attn.norm.bias.float().contiguous()
        P[k + '.qkv'] = ops.pack_mfma(attn.fn.to_qkv.weight)
        P[k + '.proj'] = ops.pack_mfma(attn.fn.to_out[0].weight)
        P[k + '.proj.b'] = attn.fn.to_out[0].bias.float().contiguous()
        P[k + '.ln2.g'], P[k + '.ln2.b'] = ff.norm.weight.float().contiguous(), ff.norm.bias.float().contiguous()
        P[k + '.fc1'] = ops.pack_mfma(ff.fn.net[0].weight)
        P[k + '.fc1.b'] = ff.fn.net[0].bias.float().contiguous()
        P[k + '.fc2'] = ops.pack_mfma(ff.fn.net[3].weight)
        P[k + '.fc2.b'] = ff.fn.net[3].bias.float().contiguous()


SUPPORTED_PATCHES = (4, 6, 8, 12, 16)
MAX_DIM = 4096


def check_vit_geometry(patch, dim, shared_mlp, blocks=()):
    """Raise NotImplementedError unless the device path covers this VitSegNet geometry; blocks: (heads, dim_head, mlp_dim) per
    transformer block.  The multiples of 32 are the GEMMs' k-slab (every K that lm_conv2d_nhwc_mfma_f32 sees); LayerNorm takes
    D % 32 == 0 up to 4096 except 768, attention dim_head 64."""
    ok = patch in SUPPORTED_PATCHES and dim % (patch * patch) == 0 and dim % 32 == 0 and 0 < dim <= MAX_DIM and dim != 768
    ok = ok and not (shared_mlp and dim // (patch * patch) % 32)
    ok = ok and all(dim_head == 64 and heads >= 1 and not (heads == 1 and dim_head == dim) and mlp_dim > 0 and mlp_dim % 32 == 0
                    for heads, dim_head, mlp_dim in blocks)
    if not ok:
        raise NotImplementedError(
            f'VitSegNet geometry patch={patch}, dim={dim}, is_with_shared_mlp={bool(shared_mlp)}, (heads, dim_head, mlp_dim)='
            f'{sorted(set(blocks))}: the device path covers square patches in {list(SUPPORTED_PATCHES)}, dim a multiple of 32 and of '
            f'patch^2 up to {MAX_DIM} (not 768), dim_head=64 with heads >= 1 (not heads=1 with dim_head=dim), int(dim * expansion_factor) a '
            f'multiple of 32, and with is_with_shared_mlp dim / patch^2 a multiple of 32')


@BACKBONE.register_module
class VitSegNet(PackedModule):
    def __init__(self, image_size=144, patch_h_size=8, patch_w_size=8, channels=64, dim=512, depth=5, heads=16,
                 output_channels=1024, expansion_factor=4, dim_head=64, dropout=0., emb_dropout=0.,
                 is_with_shared_mlp=True, is_with_llm=False, cfg=None):
        super().__init__()
        assert image_size % patch_h_size == 0 and image_size % patch_w_size == 0, \
            'Image dimensions must be divisible by the patch size.'
        if patch_h_size != patch_w_size:
            raise NotImplementedError('square patches only')
        self.patch, self.grid, self.channels, self.dim = patch_h_size, image_size // patch_h_size, channels, dim
        self.to_patch_embedding = nn.Sequential(nn.Identity(), nn.Linear(channels * patch_h_size * patch_w_size, dim))
        self.pos_embedding = nn.Parameter(torch.randn(1, self.grid * self.grid, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.transformer = _Transformer(dim, depth, heads, dim_head, int(dim * expansion_factor))
        self.out_c = dim // (patch_h_size * patch_w_size)
        self.is_with_shared_mlp = bool(is_with_shared_mlp)
        if self.is_with_shared_mlp:
            self.shared_mlp = nn.Conv2d(self.out_c, output_channels, 1)

    def _pack(self):
        P = {}
        lin = self.to_patch_embedding[1]
        p = self.patch
        # Linear weight columns are ordered (p1 p2 c) == (kh kw cin) of a pxp/stride-p conv over NHWC
        w = lin.weight.reshape(self.dim, p, p, self.channels).permute(0, 3, 1, 2)
        P['embed.w'] = ops.pack_mfma(w)
        P['embed.b'] = lin.bias.float().contiguous()
        P['pos'] = self.pos_embedding[0].float().contiguous()
        pack_transformer(self.transformer.layers, P, 'L')
        if self.is_with_shared_mlp:
            P['mlp.w'] = ops.pack_mfma(self.shared_mlp.weight)
            P['mlp.b'] = self.shared_mlp.bias.float().contiguous()
        return P

    def forward(self, img):
        """Goes through the dispatcher: torch.ops.lanemap_hip.vit_backbone (torch_ops.py)."""
        from . import torch_ops
        return torch_ops.vit_backbone(img, torch_ops.stage_weights(self), torch_ops.stage_name(self))

    def _forward_impl(self, img):
        check_vit_geometry(self.patch, self.dim, self.is_with_shared_mlp,
                           [(a.fn.heads, a.fn.dim_head, f.fn.net[0].out_features) for a, f in self.transformer.layers])
        P = self.packed()
        B = img.shape[0]
        N = self.grid * self.grid
        tok = ops.conv_mfma(img, P['embed.w'], self.dim, self.patch, self.patch, self.patch, 0, 1,
                            shift=P['embed.b'], res=P['pos'], res_rows=N)           # [B,dim,G,G] NHWC == [B*N, dim]
        t = tok.permute(0, 2, 3, 1).reshape(B * N, self.dim)
        t = transformer_forward(self.transformer.layers, P, 'L', t, B, N)
        x = ops.unpatchify(t, B, self.grid, self.patch, self.out_c)
        if self.is_with_shared_mlp:
            x = ops.conv_mfma(x, P['mlp.w'], self.shared_mlp.out_channels, shift=P['mlp.b'])
        return x


class _PreNormResidual(nn.Module):
    """mixsegnet.py:15-22: x + fn(norm(x)) (fn registered first: the reference's state-dict order)."""

    def __init__(self, dim, fn):
        super().__init__()
        self.fn = fn
        self.norm = nn.LayerNorm(dim)


def _mixer_ff(dim, expansion_factor, dense):
    return nn.Sequential(dense(dim, dim * expansion_factor), nn.GELU(), nn.Dropout(0.), dense(dim * expansion_factor, dim), nn.Dropout(0.))


def _conv1d_k1(cin, cout):
    return nn.Conv1d(cin, cout, kernel_size=1)


@BACKBONE.register_module
class MixSegNet(PackedModule):
    def __init__(self, image_size=144, channels=64, patch_size=8, dim=512, depth=5, output_channels=1024, expansion_factor=4,
                 dropout=0., cfg=None):
        super().__init__()
        assert (image_size % patch_size) == 0, 'image must be divisible by patch size'
        self.cfg = cfg
        self.patch, self.grid, self.channels, self.dim = patch_size, image_size // patch_size, channels, dim
        self.num_patches = self.grid * self.grid
        self.out_c = dim // (patch_size * patch_size)
        self.output_channels = output_channels
        self.depth = depth
        self.mixsegnet = nn.Sequential(
            nn.Identity(),                                                  # patchify 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)'
            nn.Linear(patch_size * patch_size * channels, dim),
            *[nn.Sequential(_PreNormResidual(dim, _mixer_ff(self.num_patches, expansion_factor, _conv1d_k1)),
                            _PreNormResidual(dim, _mixer_ff(dim, expansion_factor, nn.Linear))) for _ in range(depth)],
            nn.LayerNorm(dim),
            nn.Identity(),                                                  # un-patchify
            nn.Conv2d(self.out_c, output_channels, kernel_size=1))

    @property
    def blocks(self):
        return [self.mixsegnet[2 + l] for l in range(self.depth)]

    def _pack(self):
        P = {}
        lin = self.mixsegnet[1]
        p = self.patch
        # Linear weight columns are ordered (p1 p2 c) == (kh kw cin) of an 8x8/stride-8 conv over NHWC
        P['embed.w'] = ops.pack_mfma(lin.weight.reshape(self.dim, p, p, self.channels).permute(0, 3, 1, 2))
        P['embed.b'] = lin.bias.float().contiguous()
        for l, (tok, ch) in enumerate(self.blocks):
            k = f'L{l}'
            P[k + '.ln1.g'], P[k + '.ln1.b'] = tok.norm.weight.float().contiguous(), tok.norm.bias.float().contiguous()
            P[k + '.tm1'] = ops.pack_token_mix(tok.fn[0].weight)
            P[k + '.tm1.b'] = tok.fn[0].bias.float().contiguous()
            P[k + '.tm2'] = ops.pack_token_mix(tok.fn[3].weight)
            P[k + '.tm2.b'] = tok.fn[3].bias.float().contiguous()
            P[k + '.ln2.g'], P[k + '.ln2.b'] = ch.norm.weight.float().contiguous(), ch.norm.bias.float().contiguous()
            P[k + '.fc1'] = ops.pack_mfma(ch.fn[0].weight)
            P[k + '.fc1.b'] = ch.fn[0].bias.float().contiguous()
            P[k + '.fc2'] = ops.pack_mfma(ch.fn[3].weight)
            P[k + '.fc2.b'] = ch.fn[3].bias.float().contiguous()
        ln = self.mixsegnet[2 + self.depth]
        P['ln.g'], P['ln.b'] = ln.weight.float().contiguous(), ln.bias.float().contiguous()
        conv = self.mixsegnet[4 + self.depth]
        P['out.w'] = ops.pack_small(conv.weight)
        P['out.b'] = conv.bias.float().contiguous()
        return P

    def forward(self, img):
        """Goes through the dispatcher: torch.ops.lanemap_hip.mixer_backbone (torch_ops.py)."""
        from . import torch_ops
        return torch_ops.mixer_backbone(img, torch_ops.stage_weights(self), torch_ops.stage_name(self))

    def _forward_impl(self, img):
        if self.output_channels > 16 or self.out_c % 4:
            raise NotImplementedError(f'MixSegNet output conv {self.out_c}->{self.output_channels}: the hot path covers <= 16 outputs '
                                      'from a multiple of 4 channels')
        P = self.packed()
        B = img.shape[0]
        N = self.num_patches
        tok = ops.conv_mfma(img, P['embed.w'], self.dim, self.patch, self.patch, self.patch, 0, 1, shift=P['embed.b'])
        t = tok.permute(0, 2, 3, 1).reshape(B * N, self.dim)                # [B,dim,G,G] NHWC == [B*N, dim]
        for l, (tm, cm) in enumerate(self.blocks):
            k = f'L{l}'
            y = ops.layernorm(t, P[k + '.ln1.g'], P[k + '.ln1.b'], tm.norm.eps)
            h = ops.token_mix(y, P[k + '.tm1'], tm.fn[0].out_channels, P[k + '.tm1.b'], B, act=ops.ACT_GELU)
            t = ops.token_mix(h, P[k + '.tm2'], N, P[k + '.tm2.b'], B, res=t)
            y = ops.layernorm(t, P[k + '.ln2.g'], P[k + '.ln2.b'], cm.norm.eps)
            y = ops.linear_mfma(y, P[k + '.fc1'], cm.fn[0].out_features, shift=P[k + '.fc1.b'], act=ops.ACT_GELU)
            t = ops.linear_mfma(y, P[k + '.fc2'], self.dim, shift=P[k + '.fc2.b'], res=t)
        t = ops.layernorm(t, P['ln.g'], P['ln.b'], self.mixsegnet[2 + self.depth].eps)
        x = ops.unpatchify(t, B, self.grid, self.patch, self.out_c)
        return ops.conv_small(x, P['out.w'], self.output_channels, shift=P['out.b'])
