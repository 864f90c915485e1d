"""Column-proposal head behind the reference's HEADS registry name ``ColumnProposal2``.

Drop-in for baseline/models/heads/polyline_fpn_vit_vertex_2.py: same constructor kwargs (:66-99), same
state-dict keys (3.95 M parameters, of which only ~0.10 M are live at inference — SURVEY F9; the dead ones
are kept so checkpoints load strictly), same method names and output dictionaries:

  forward(x, x_up, x_endp)                 :309-435  -> proposal_conf, ext2, cls2, offset2, orient
  get_exist_coor_endp_dict(out)            :602-759  -> prop_conf, prop_v_ext, prop_cls_conf, endp, orient, bi_seg,
                                                        semantic_seg, cls_offset
  get_lane_map_numpy_with_label(...)       :761-886  -> lane_maps {coor_label, cls_offset_smooth, endp_by_cls, semantic_line}
  get_lane_map_on_source_image(...)        :926-1083 -> pred_smooth_lane_vertex (vertex packing only, no cv2 overlays)

spatial_att=False (the MixSeg config): the tokens are the raw zero-padded row windows, the bi_seg_proposal conv is skipped
(its parameters stay for strict loading).
Proposal geometries (the reference config's `num_prop = 72, 36, 18` / `prop_width = 2, 4, 8`): SUPPORTED_GEOMETRIES with
prop_half_buff = 4, i.e. prop_fea_width FW = 10, 12 or 16, and dim_shared any multiple of 4 up to 512.
column_att=True (the proposal-attention branch, :317-345; check_column_att): generate_line_proposal, to_token + emb_*,
tr_lane_correlator and line_expand turn the P column proposals into tokens, run the lane transformer across them and expand them
back into a [B,8,144,P] column feature whose bilinear upsampling replaces that of x in the head's concat buffer.  Device route:
the 5x3 conv and each stage's BatchNorm (a diagonal 1x1 conv: it sits between the ReLU and a zero-padded conv, so it cannot be
folded into that conv) and stride-2 conv as lm_conv2d_nhwc_small; to_token + emb as ONE (P x 1) lm_conv2d_nhwc_mfma_f32 over
feat_down (output pixel (b, 0, w) = token row b P + w, emb through res_rows = P); the ViT transformer kernels and LayerNorm;
line_expand as a GEMM whose rows are permuted to (h c); lm_sparse_to_dense_nhwc moves [b][p][h][c] to NHWC [b][h][p][c].
endp_mode='endpoint' (cfg.heads.endp_mode; the reference's "local+global" endpoints, :254-260, :371-373, :650-653): the head computes
its own endpoint map out['endpoint'] [B,1,1152,1152] = endpoint(relu(cat(up(col), x_endp))) from its 16-channel concat buffer and the
FPN's endpoint logits, and the decode reads that map wherever it reads out['endp_est'] otherwise (endp_logits()).  Device route: ONE
kernel, lm_head_endpoint (csrc/head_endpoint.hip), which never builds the [B,17,1152,1152] concatenation; the BatchNorm between the
ReLU and the zero-padded second convolution stays a scale and shift of its own, as in the column_att stages.  With any other
endp_mode (every BASELINE config: 'endp_est') nothing is launched and no 'endpoint' key appears.
Not supported (raise): other geometries, column_att with spatial_att=False or outside check_column_att, the
column_transformer_decoder branch (broken upstream: it uses self.pe / self.line_decoder, which are never built),
view_detail=True (the reference itself raises NameError there).  `prop_bi_seg` ([B,72,1,1152,80], unused downstream) is
not produced.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops, decode, hostpost
from .backbone import _Transformer, _FeedForward, pack_transformer, transformer_forward
from .registry import HEADS
from .packing import PackedModule


class _ConvPool2d(nn.Module):
    """Parameter container of the (dead at inference) `generate_line_proposal` stack (:48-61)."""

    def __init__(self, cin, hidden, cout):
        super().__init__()
        layers = [nn.Conv2d(cin, cin, (5, 3), padding=(2, 1))]
        for a, b in zip([cin] + hidden, hidden + [cout]):
            layers.append(nn.Sequential(nn.ReLU(inplace=True), nn.BatchNorm2d(a), nn.Conv2d(a, b, 3, 2, 1)))
        self.layers = nn.ModuleList(layers)


SUPPORTED_GEOMETRIES = ((72, 2), (36, 4), (18, 8))     # (num_prop, prop_width); prop_half_buff = 4, num_prop * prop_width = 144
SUPPORTED_HALF_BUFF = 4
MAX_DIM_SHARED = 512


def check_geometry(num_prop, prop_width, prop_half_buff, dim_shared):
    """Raise NotImplementedError unless the device path covers this head geometry."""
    if ((num_prop, prop_width) not in SUPPORTED_GEOMETRIES or prop_half_buff != SUPPORTED_HALF_BUFF
            or dim_shared % 4 or not 0 < dim_shared <= MAX_DIM_SHARED):
        raise NotImplementedError(
            f'ColumnProposal2 geometry num_prop={num_prop}, prop_width={prop_width}, prop_half_buff={prop_half_buff}, '
            f'dim_shared={dim_shared}: the device path covers (num_prop, prop_width) in {list(SUPPORTED_GEOMETRIES)} with '
            f'prop_half_buff={SUPPORTED_HALF_BUFF} and dim_shared a multiple of 4 up to {MAX_DIM_SHARED}')


COLUMN_ATT_MAX_DIM_TOKEN = 4096


def check_column_att(spatial_att, dim_token, tr_heads, tr_dim_head, tr_mlp_dim, tr_depth):
    """Raise NotImplementedError, naming the parameter at fault, unless the device path covers this column_att=True head (on top of
    check_geometry).  The multiples of 32 are the GEMMs' k-slab; LayerNorm takes dim_token % 32 == 0 up to 4096 except 768; the
    attention kernels take dim_head 64; heads=1 with dim_head=dim_token has no output projection (to_out is the identity)."""
    bad = None
    if not spatial_att:
        bad = 'spatial_att=False (the proposal tokens without the segmentation attention)'
    elif dim_token % 32 or not 0 < dim_token <= COLUMN_ATT_MAX_DIM_TOKEN or dim_token == 768:
        bad = f'dim_token={dim_token} (a multiple of 32 up to {COLUMN_ATT_MAX_DIM_TOKEN}, not 768)'
    elif tr_dim_head != 64:
        bad = f'tr_dim_head={tr_dim_head} (64)'
    elif tr_heads < 1 or (tr_heads == 1 and tr_dim_head == dim_token):
        bad = f'tr_heads={tr_heads} (>= 1, not 1 with tr_dim_head = dim_token)'
    elif tr_mlp_dim <= 0 or tr_mlp_dim % 32:
        bad = f'tr_mlp_dim={tr_mlp_dim} (a positive multiple of 32)'
    elif tr_depth < 0:
        bad = f'tr_depth={tr_depth} (>= 0)'
    if bad is not None:
        raise NotImplementedError(f'ColumnProposal2 column_att=True with {bad}: the device path covers spatial_att=True, dim_token a '
                                  f'multiple of 32 up to {COLUMN_ATT_MAX_DIM_TOKEN} except 768, tr_dim_head=64, any tr_heads / tr_depth '
                                  'and tr_mlp_dim a multiple of 32')


def _conv1d_stack(cin, hidden, cout):
    return nn.Sequential(nn.Conv1d(cin, hidden, 1), nn.BatchNorm1d(hidden), nn.Conv1d(hidden, cout, 1), nn.Identity())


@HEADS.register_module
class ColumnProposal2(PackedModule):
    def __init__(self, dim_feat=8, row_size=144, dim_shared=512, num_prop=72, prop_width=2, prop_half_buff=4,
                 dim_token=1024, tr_depth=1, tr_heads=16, tr_dim_head=64, tr_mlp_dim=2048, tr_dropout=0.,
                 tr_emb_dropout=0., row_dim_token=64, row_tr_depth=1, row_tr_heads=10, row_tr_dim_head=12,
                 row_tr_mlp_dim=128, row_tr_dropout=0., row_tr_emb_dropout=0., endp_mode='Regr', cls_exp=False,
                 ext_w=1., ext_smooth_w=1., lambda_cls=1., mean_loss_w=0., cls_smooth_loss_w=0., orient_w=1.,
                 endp_loss_w=1., offset_w=1., freeze_endp=False, freeze_ori=False, cfg=None):
        super().__init__()
        self.cfg = cfg
        self.flip_label = cfg.flip_label
        self.num_cls = cfg.number_lanes
        self.num_orients = cfg.number_orients
        self.num_prop, self.prop_width, self.prop_half_buff = num_prop, prop_width, prop_half_buff
        self.row_size, self.endp_mode = row_size, endp_mode
        self.N_s = prop_width
        self.prop_fea_width = prop_width + 2 * prop_half_buff
        self.dim_shared = dim_shared
        self.dim_feat = dim_feat
        self.dim_token, self.tr_depth, self.tr_heads, self.tr_dim_head, self.tr_mlp_dim = dim_token, tr_depth, tr_heads, tr_dim_head, tr_mlp_dim
        self._ca_coords = {}
        hd = dim_feat * 2
        # ---- column_att branch (live only with cfg.column_att) and `endpoint` (live only with endp_mode='endpoint'); reg_ffn /
        # head_upsample_layers are dead, kept for strict checkpoint loading ----
        self.reg_ffn = _FeedForward(dim_feat, dim_feat * 4)
        hidden = {72: [], 36: [2 * dim_feat], 18: [2 * dim_feat, 4 * dim_feat]}.get(num_prop)
        if hidden is not None:
            self.generate_line_proposal = nn.Sequential(_ConvPool2d(dim_feat, hidden, dim_feat * 2 ** (len(hidden) + 1)))
        in_tok = num_prop * dim_feat * prop_width
        self.to_token = nn.Sequential(nn.Identity(), nn.Linear(in_tok, dim_token))
        for i in range(num_prop):
            setattr(self, f'emb_{i}', nn.Parameter(torch.randn(dim_token)))
        self.tr_lane_correlator = nn.Sequential(_Transformer(dim_token, tr_depth, tr_heads, tr_dim_head, tr_mlp_dim),
                                                nn.LayerNorm(dim_token))
        self.line_expand = nn.Sequential(nn.Linear(dim_token, in_tok), nn.Identity())
        self.head_upsample_layers = nn.Sequential(nn.Conv2d(hd, dim_feat, (5, 3), 1, (2, 1)), nn.BatchNorm2d(dim_feat),
                                                  nn.Conv2d(dim_feat, dim_feat, 3, 1, 1), nn.BatchNorm2d(dim_feat))
        self.endpoint = nn.Sequential(nn.Conv2d(hd + 1, dim_feat // 2, 3, 1, 1), nn.ReLU(inplace=True),
                                      nn.BatchNorm2d(dim_feat // 2), nn.Conv2d(dim_feat // 2, 1, 3, 1, 1))
        # ---- live parameters ----
        self.head_common_layers = nn.Sequential(nn.Conv2d(hd, hd, 3, 1, 1), nn.BatchNorm2d(hd),
                                                nn.Conv2d(hd, hd, 3, 2, 1), nn.BatchNorm2d(hd))
        self.proposal_confidence = nn.Sequential(nn.Identity(), nn.Linear(hd * self.prop_fea_width * row_size, 2))
        self.ext2 = _conv1d_stack(hd * self.prop_fea_width, dim_shared, 3)
        self.cls2 = _conv1d_stack(hd * self.prop_fea_width, dim_shared, self.prop_fea_width)
        self.offset2 = _conv1d_stack(hd * self.prop_fea_width, dim_shared, self.prop_fea_width)
        self.orient = nn.Sequential(nn.Conv2d(hd, hd // 2, 3, 1, 1), nn.BatchNorm2d(hd // 2),
                                    nn.Conv2d(hd // 2, self.num_orients, 3, 1, 1))
        self.bi_seg_proposal = nn.Conv2d(hd, 1, 1)

    # -------------------------------------------------------------------------------- packing
    def _pack(self):
        P = {}
        hc = self.head_common_layers
        P['hc0.w'] = ops.pack_small(hc[0].weight)
        P['hc0.s'], P['hc0.b'] = ops.fold_bn(hc[1], hc[0].bias)
        P['hc2.w'] = ops.pack_small(hc[2].weight)
        P['hc2.s'], P['hc2.b'] = ops.fold_bn(hc[3], hc[2].bias)
        P['or0.w'] = ops.pack_small(self.orient[0].weight)
        P['or0.s'], P['or0.b'] = ops.fold_bn(self.orient[1], self.orient[0].bias)
        P['or2.w'] = ops.pack_small(self.orient[2].weight)
        P['or2.b'] = self.orient[2].bias.float().contiguous()
        P['seg.w'] = ops.pack_small(self.bi_seg_proposal.weight)
        P['seg.b'] = self.bi_seg_proposal.bias.float().contiguous()
        P['seg.bias_value'] = float(self.bi_seg_proposal.bias.item())
        stacks = (self.ext2, self.cls2, self.offset2)
        P['w1'] = ops.pack_mfma(torch.cat([s[0].weight[:, :, 0] for s in stacks], dim=0))
        sc, sh = zip(*[ops.fold_bn(s[1], s[0].bias) for s in stacks])
        P['s1'], P['b1'] = torch.cat(sc).contiguous(), torch.cat(sh).contiguous()
        P['w2'] = torch.cat([s[2].weight[:, :, 0] for s in stacks], dim=0).float().contiguous()
        P['b2'] = torch.cat([s[2].bias for s in stacks]).float().contiguous()
        if self.prop_fea_width != 10:        # stage 2 as three 1x1 small convs (ops.head_stage2)
            P['w2.small'] = [ops.pack_small(s[2].weight[:, :, :, None]) for s in stacks]
        lin = self.proposal_confidence[1]
        cw = lin.in_features // self.row_size
        P['conf.w'] = lin.weight.reshape(2, cw, self.row_size).permute(0, 2, 1).reshape(2, -1).float().contiguous()
        P['conf.b'] = lin.bias.float().contiguous()
        return P

    def _pack_column_att(self):
        """Weights of the column_att branch (:317-345), packed on first use: the branch is off in every BASELINE config."""
        P = {}
        layers = self.generate_line_proposal[0].layers
        conv0 = layers[0]
        P['ca.f0.w'] = ops.pack_small(conv0.weight)
        P['ca.f0.b'] = conv0.bias.float().contiguous()
        S = len(layers) - 1
        for i, (_, bn, conv) in enumerate(layers[1:]):
            # BN_i as a 1x1 conv with diagonal weights: a * r + beta once per element, the zero padding of the next conv stays zero
            a, beta = ops.fold_bn(bn)
            P[f'ca.bn{i}.w'] = ops.pack_small(torch.diag(a)[:, :, None, None])
            P[f'ca.bn{i}.b'] = beta
            w, b = conv.weight, conv.bias
            if i == S - 1 and w.shape[0] < 32:      # feat_down feeds a GEMM whose K slab is 32 channels: outputs 16..31 are exact zeros
                w = torch.cat([w, w.new_zeros((32 - w.shape[0],) + tuple(w.shape[1:]))])
                b = torch.cat([b, b.new_zeros(32 - b.shape[0])])
            P[f'ca.s{i}.w'] = ops.pack_small(w)
            P[f'ca.s{i}.b'] = b.float().contiguous()
        cd = layers[-1][2].out_channels
        cdp = max(cd, 32)
        lin = self.to_token[1]
        # Linear over (c h) of feat_down[b, :, :, w] -> a (P x 1) convolution weight [n][c][h][1], channels zero padded to cdp
        wt = lin.weight.reshape(lin.out_features, cd, self.num_prop)
        wt = torch.cat([wt, wt.new_zeros(lin.out_features, cdp - cd, self.num_prop)], dim=1)
        P['ca.tok.w'] = ops.pack_mfma(wt[:, :, :, None])
        P['ca.tok.b'] = lin.bias.float().contiguous()
        P['ca.emb'] = torch.stack([getattr(self, f'emb_{i}') for i in range(self.num_prop)]).float().contiguous()
        pack_transformer(self.tr_lane_correlator[0].layers, P, 'ca.T')
        ln = self.tr_lane_correlator[1]
        P['ca.ln.g'], P['ca.ln.b'] = ln.weight.float().contiguous(), ln.bias.float().contiguous()
        ex = self.line_expand[0]
        C_, R = self.dim_feat, self.row_size
        # rows (c h) -> (h c): the GEMM output row of token (b, p) is then [h][c], one NHWC pixel per h
        P['ca.exp.w'] = ops.pack_mfma(ex.weight.reshape(C_, R, -1).permute(1, 0, 2).reshape(C_ * R, -1))
        P['ca.exp.b'] = ex.bias.reshape(C_, R).t().reshape(-1).float().contiguous()
        return P

    def _pack_endpoint(self):
        """Operands of lm_head_endpoint (:254-260), packed on first use: the mode is off in every BASELINE config."""
        ep = self.endpoint
        return {'ep': ops.pack_head_endpoint(ep[0], ep[2], ep[3])}

    def endpoint_mode(self):
        """True when the endpoints are decoded from the head's own map (cfg.heads.endp_mode == 'endpoint', :650-653)."""
        heads_cfg = getattr(self.cfg, 'heads', None)
        return getattr(heads_cfg, 'endp_mode', self.endp_mode) == 'endpoint'

    def endp_logits(self, out):
        """The endpoint logits [B,1,H,W] the decode reads: out['endpoint'] in endpoint mode, the FPN's out['endp_est'] otherwise."""
        return out['endpoint'] if self.endpoint_mode() else out['endp_est']

    def _column_coords(self, B, device):
        """lm_sparse_to_dense_nhwc coordinates (b, 0, h, p) of the line_expand row (b P + p) 144 + h; built once per (B, device)
        with device arange, outside any graph capture (TilePipeline runs a batch shape eagerly before it captures it)."""
        key = (B, str(device))
        t = self._ca_coords.get(key)
        if t is None:
            P_, R = self.num_prop, self.row_size
            b = torch.arange(B, device=device, dtype=torch.int32).view(B, 1, 1).expand(B, P_, R)
            p = torch.arange(P_, device=device, dtype=torch.int32).view(1, P_, 1).expand(B, P_, R)
            h = torch.arange(R, device=device, dtype=torch.int32).view(1, 1, R).expand(B, P_, R)
            t = torch.stack([b, torch.zeros_like(b), h, p], dim=-1).reshape(-1, 4).contiguous()
            self._ca_coords[key] = t
        return t

    def _column_att_features(self, x, P):
        """:317-341 -> colfeat [B,8,144,P] (NHWC-stored) and the intermediates (feat_down, tokens) for the tests."""
        B = x.shape[0]
        Np, R, C_ = self.num_prop, self.row_size, self.dim_feat
        f = ops.conv_small(x, P['ca.f0.w'], C_, 5, 3, 1, (2, 1), shift=P['ca.f0.b'], act=ops.ACT_RELU)   # read only through the ReLU
        S = len(self.generate_line_proposal[0].layers) - 1
        for i in range(S):
            cin = f.shape[1]
            f = ops.conv_small(f, P[f'ca.bn{i}.w'], cin, shift=P[f'ca.bn{i}.b'])
            cout = P[f'ca.s{i}.b'].numel()
            f = ops.conv_small(f, P[f'ca.s{i}.w'], cout, 3, 3, 2, 1, shift=P[f'ca.s{i}.b'],
                               act=ops.ACT_RELU if i < S - 1 else ops.ACT_NONE)
        feat_down = f                                                                    # [B, max(Cd, 32), P, P]
        D = P['ca.tok.b'].numel()
        tok = ops.conv_mfma(feat_down, P['ca.tok.w'], D, kh=Np, kw=1, shift=P['ca.tok.b'], res=P['ca.emb'], res_rows=Np)
        t = tok.permute(0, 2, 3, 1).reshape(B * Np, D)                                  # [B,1,P,D] NHWC = token rows b P + w
        t = transformer_forward(self.tr_lane_correlator[0].layers, P, 'ca.T', t, B, Np)
        t = ops.layernorm(t, P['ca.ln.g'], P['ca.ln.b'], self.tr_lane_correlator[1].eps)
        e = ops.linear_mfma(t, P['ca.exp.w'], C_ * R, shift=P['ca.exp.b'])              # [B*P, (h c)]
        colfeat = ops.sparse_to_dense(e.view(B * Np * R, C_), self._column_coords(B, x.device), B, (1, R, Np), C_, False)
        return colfeat, feat_down, t

    # -------------------------------------------------------------------------------- forward
    def forward(self, x, x_up, x_endp=None, col=None):
        """x [B,8,144,144], x_up [B,8,288,288] -> raw head outputs (live sub-graph).
        `col`: optional pre-assembled [B,16,288,288] buffer whose channels 8..15 already hold x_up.
        Goes through the dispatcher: torch.ops.lanemap_hip.colprop_head (torch_ops.py) and, in endpoint mode, colprop_endpoint on the
        buffer colprop_head has completed and x_endp [B,1,1152,1152] -> out['endpoint']."""
        from . import torch_ops
        if col is None:
            col = ops.new_act(x.shape[0], 16, x_up.shape[2], x_up.shape[3], x.device)
            col[:, 8:16].copy_(x_up)
        self.b_size = x.shape[0]
        conf, ext2, cls2, off2, orient = torch_ops.colprop_head(x, col, torch_ops.stage_weights(self), torch_ops.stage_name(self))
        out = {'proposal_conf': conf, 'ext2': ext2, 'cls2': cls2, 'offset2': off2, 'orient': orient}
        if self.endpoint_mode():
            if x_endp is None:
                raise ValueError("ColumnProposal2 with endp_mode='endpoint' needs x_endp (the FPN's endpoint logits)")
            out['endpoint'] = torch_ops.colprop_endpoint(col, x_endp, torch_ops.stage_weights(self), torch_ops.stage_name(self))
        return out

    def _endpoint_impl(self, col, x_endp):
        """:371-373 on the completed concat buffer; the up-sampling to (8 * 144)^2 that follows upstream is the identity at x_endp's size."""
        P = self.packed()
        if 'ep' not in P:
            with torch.no_grad():
                P.update(self._pack_endpoint())
        return ops.head_endpoint(col, x_endp, P['ep'])

    def _forward_impl(self, x, x_up, x_endp=None, col=None):
        cfg = self.cfg
        if cfg.column_transformer_decoder:
            raise NotImplementedError('column_transformer_decoder is broken upstream (it uses self.pe / self.line_decoder, which the '
                                      'reference never builds)')
        check_geometry(self.num_prop, self.prop_width, self.prop_half_buff, self.dim_shared)
        if cfg.column_att:
            check_column_att(cfg.spatial_att, self.dim_token, self.tr_heads, self.tr_dim_head, self.tr_mlp_dim, self.tr_depth)
        P = self.packed()
        if cfg.column_att and 'ca.tok.w' not in P:
            with torch.no_grad():
                P.update(self._pack_column_att())
        B, _, h, w = x.shape
        self.b_size = B
        hd = 16
        if col is None:
            col = ops.new_act(B, hd, x_up.shape[2], x_up.shape[3], x.device)
            col[:, 8:16].copy_(x_up)
        if cfg.column_att:
            colfeat = self._column_att_features(x, P)[0]
            ops.upsample_nhwc(colfeat, col.shape[2:], out=col[:, 0:8])                         # :341
        else:
            ops.upsample_nhwc(x, col.shape[2:], out=col[:, 0:8])                               # :359
        r = ops.conv_small(col, P['hc0.w'], hd, 3, 3, 1, 1, scale=P['hc0.s'], shift=P['hc0.b'])
        row = ops.conv_small(r, P['hc2.w'], hd, 3, 3, 2, 1, scale=P['hc2.s'], shift=P['hc2.b'])   # :376
        o = ops.conv_small(row, P['or0.w'], hd // 2, 3, 3, 1, 1, scale=P['or0.s'], shift=P['or0.b'])
        orient = ops.conv_small(o, P['or2.w'], self.num_orients, 3, 3, 1, 1, shift=P['or2.b'])      # :380
        if cfg.spatial_att:
            seg = ops.conv_small(col, P['seg.w'], 1, shift=P['seg.b'], pre_relu=True)               # :400 (once)
            tok = ops.head_tokens(seg, row, self.num_prop, self.prop_width, self.prop_half_buff, P['seg.bias_value'])
        else:                                                                                       # :403-404 raw row window
            tok = ops.head_tokens(None, row, self.num_prop, self.prop_width, self.prop_half_buff, 0.)
        D = self.dim_shared
        hid = torch.empty((tok.shape[0], -(-3 * D // 64) * 64), device=x.device, dtype=torch.float32)   # 320 columns at D = 100
        ops.linear_mfma(tok, P['w1'], 3 * D, scale=P['s1'], shift=P['b1'], out=hid)
        ext2, cls2, off2 = ops.head_stage2(hid, D, P['w2'], P['b2'], B, self.num_prop, h, w_small=P.get('w2.small'))
        conf = ops.head_proposal_conf(tok, P['conf.w'], P['conf.b'], B, self.num_prop)
        return {'proposal_conf': conf, 'ext2': ext2, 'cls2': cls2, 'offset2': off2, 'orient': orient}

    # -------------------------------------------------------------------------------- decode / assembly
    def decode_compact(self, out):
        """Device decode + endpoint clustering, compact form (what the runner and bench use)."""
        return decode.decode_compact(out, self.cfg, self.num_cls, self.prop_width, self.prop_half_buff,
                                     endp_logits=self.endp_logits(out))

    def get_exist_coor_endp_dict(self, out):
        if getattr(self.cfg, 'view_detail', False):
            raise NotImplementedError('view_detail=True is unsupported (the reference raises NameError there)')
        c = self.decode_compact(out)
        self._compact = c
        return decode.compact_to_reference_dict(c)

    def get_lane_map_numpy_with_label(self, output, data, is_flip=True, is_img=False, is_get_1_stage_result=False,
                                      is_gt_avai=True):
        B = output['prop_conf'].shape[0]
        lane_maps = {'coor_label': [], 'cls_offset_smooth': [], 'endp_by_cls': [], 'semantic_line': []}
        if is_gt_avai:
            lane_maps['coor_label'] = [data['lc_coor_raw'][b].cpu().numpy() for b in range(B)]
        pc = output['prop_conf'].float().cpu().numpy()
        ve = output['prop_v_ext'].float().cpu().numpy()
        co = output['cls_offset'].double().cpu().numpy()
        comp = getattr(self, '_compact', None)
        if comp is not None and comp.get('bi_seg_rows') is not None and comp['bi_seg'] is output.get('bi_seg'):
            rows = comp['bi_seg_rows'].cpu().numpy()
        else:
            rows = output['bi_seg'][:, 3::8, :].float().cpu().numpy()
        for b in range(B):
            e = output['endp'][b]
            ep = np.stack(np.nonzero(e.cpu().numpy() if torch.is_tensor(e) else e), axis=1).astype(np.int32)
            lanes, kept = hostpost.assemble_polylines(pc[b], ve[b], co[b], rows[b], ep, self.cfg.proposal_obj_thre)
            emap = np.zeros((self.row_size * 8, self.row_size * 8), dtype=np.float32)
            emap[kept[:, 0], kept[:, 1]] = 1.0
            lane_maps['cls_offset_smooth'].append(lanes)
            lane_maps['endp_by_cls'].append(emap)
            lane_maps['semantic_line'].append(hostpost.raster_semantic_map(lanes))
        return lane_maps

    def get_lane_map_on_source_image(self, output, data, is_img=True):
        """Only the vertex packing (row = 3 + 8 i, col, semantic) of :997-1000,1056; overlays are out of scope."""
        packed = []
        for lanes in output['lane_maps']['cls_offset_smooth']:
            v = np.zeros((lanes.shape[0], self.row_size, 3))
            v[:, :, 0] = np.arange(3, self.row_size * 8, 8)
            v[:, :, 1:] = lanes
            packed.append(v)
        return {'pred_smooth_lane_vertex': packed}
