/* lanemap_hip.h — C ABI of liblanemap_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the inference hot path of WHU-USI3DV/LaneMapping.  The reference is pure Python
 * (torch.nn modules built through a registry); what a maintainer binds from the reference side
 * is therefore a ctypes stub per torch.nn call site.  Every entry point:
 *   - takes plain pointers + sizes (device pointers unless the name says host), no torch types;
 *   - launches on the hipStream_t passed as `stream` (NULL = default stream) and returns immediately;
 *   - returns 0 on success, non-zero on error (lm_last_error() gives the message; nothing is thrown);
 *   - borrows its inputs (const), never frees or allocates caller-visible memory.
 * Streams and graphs: an entry enqueues on `stream` and on no other stream.  Every entry may be captured into a HIP graph (after one
 * eager call of the same shape) except lm_strip_bin_points, lm_strip_plan_create, lm_tile_ground, lm_ground_select,
 * lm_tile_intensity_window, lm_tile_intensity_cells, lm_tile_intensity_apply and lm_drape_vertices, which copy host memory of the call to the device or synchronise the stream: on a capturing stream they return
 * LM_ERR_ARG with their name and the reason before touching it, and the capture stays valid.  Measured: tests/test_gpu_streams.py
 * (single-stream captures, three replays each; captures with parallel branches were not measured).
 * Activations are fp32, NHWC ("pixel-major rows", channel stride 1); `ld*` = floats between consecutive pixels.
 * Citations are file:line in the reference (relative to its repo root).
 */
#ifndef LANEMAP_HIP_H
#define LANEMAP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { LM_OK = 0, LM_ERR_ARG = 1, LM_ERR_HIP = 2, LM_ERR_NO_DEVICE = 3, LM_ERR_CAPACITY = 4 };
enum { LM_ACT_NONE = 0, LM_ACT_RELU = 1, LM_ACT_GELU = 2 };

int lm_abi_version(void);
const char* lm_last_error(void);          /* thread-local, valid until the next failing call */
int lm_device_count(void);

/* ---- matrix-core convolution / GEMM -------------------------------------------------------------------------
 * y[m,n] = act((sum_{tap,c} x[pix(m,tap),c] * wp[tap][n][c]) * scale[n] + shift[n] + res[m % res_rows, n])
 * Replaces every nn.Conv2d with Cin%32==0 of FPNWrapper (baseline/models/pcencoder/postprojector.py:463-511,
 * 563-655; BasicBlock :299-338 with BN folded into scale/shift), every nn.Linear of VitSegNet
 * (baseline/models/backbone/vitsegnet.py:32-35,51-56,165; patch embedding = 8x8 stride-8 case) and the first
 * Conv1d+BN1d of ext2/cls2/offset2 (baseline/models/heads/polyline_fpn_vit_vertex_2.py:206-228).
 * wp: [KH*KW][CoutP][Cin], CoutP = Cout rounded up to 128 (zero rows).  scale/shift/res may be NULL.
 * res_rows == 0: residual has one row per output pixel; > 0: row index is m % res_rows (positional embedding). */
int lm_conv2d_nhwc_mfma_f32(void* stream, const float* x, int ldx, const float* wp, int CoutP,
                            const float* scale, const float* shift, const float* res, int ldr, int res_rows,
                            float* y, int ldy, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                            int stride, int pad_h, int pad_w, int dil, int act);
/* Same convolution with a COARSE residual [B][Hr][Wr][ldr] added through bilinear (align_corners=True) interpolation to Ho x Wo:
 * `_upsample_add(p_coarse, latlayer(c))` of the FPN (postprojector.py:549-561, 595-601) without writing the upsampled map.
 * Cout, ldy, ldr multiples of 4.  Bit-identical to lm_upsample_bilinear_nhwc + lm_conv2d_nhwc_mfma_f32(res = that map). */
int lm_conv2d_nhwc_mfma_resup_f32(void* stream, const float* x, int ldx, const float* wp, int CoutP, const float* scale,
                                  const float* shift, const float* res_coarse, int ldr, int Hr, int Wr, float* y, int ldy,
                                  int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_h, int pad_w,
                                  int dil, int act);

/* Winograd F(4x4,3x3) on the fp32 matrix cores (csrc/conv_wino44.hip): the 3x3 / stride-1 layers (postprojector.py:322-338,597-647) with 36
 * products per 4x4 output block instead of 144 (3x3 / stride 1 / pad == dilation), exact fp32 MFMA, no transformed tensor in HBM.
 * Error at the level of a re-ordered direct sum (transform constants up to 8 and down to 1/24: profiles/r3_f44_numerics_study.txt);
 * lm_conv3x3_winograd44_twin_f32 is the materialising twin (V and M in a workspace, three plain kernels) with identical bits.
 * wu_frag: U = G g G^T (fp64 -> fp32) per wave fragment, [36][Cin/8][CoutP/32][64 lanes][4]:
 *   wu_frag[xi][u][nt][lane][e] = U[xi][nt*32 + (lane & 31)][8 u + 4 (lane >> 5) + e], CoutP % 64 == 0, Cin % 16 == 0.
 * wu (twin): U as [36][CoutP][Cin].  gn_partial: [B][lm_winograd44_gn_chunks][Cout][2] doubles -> lm_gn_finalize. */
int lm_winograd44_supported(int H, int W, int Cin, int dil);
/* the same for an input of pixel stride ldx floats: 0 as well when an image of it spans 2^31 bytes or more (32-bit offsets in the patch loads) */
int lm_winograd44_supported_ld(int H, int W, int Cin, int dil, int ldx);
int lm_winograd44_gn_chunks(int H, int W, int dil);
long lm_winograd44_tiles(int B, int H, int W, int dil);
long lm_winograd44_twin_workspace_bytes(int B, int H, int W, int Cin, int CoutP, int dil);
int lm_conv3x3_winograd44_f32(void* stream, const float* x, int ldx, const float* wu_frag, int CoutP, const float* scale,
                              const float* shift, const float* res, int ldr, float* y, int ldy, int B, int H, int W,
                              int Cin, int Cout, int dil, int act, double* gn_partial);
int lm_conv3x3_winograd44_twin_f32(void* stream, const float* x, int ldx, const float* wu, int CoutP, const float* scale,
                                   const float* shift, const float* res, int ldr, float* y, int ldy, int B, int H, int W,
                                   int Cin, int Cout, int dil, int act, void* workspace, long workspace_bytes);
/* SECOND LINE of the same convolution (never the default path; round 6): the Winograd-domain products on the fp16 matrix pipe with
 * fp32-accurate products - every fp32 operand x = hi + lo in two fp16 terms (22 bits), v u ~= v_hi u_hi + v_hi u_lo + v_lo u_hi as three
 * v_mfma_f32_32x32x8_f16 with fp32 accumulation.  The caller scales U by a power of two u_scale (max |U| u_scale ~ 2^13), packs its
 * fragments as for lm_conv3x3_winograd44_f32 and splits them ONCE with lm_wino44_split_fragments (n_quads = elements / 4); post = 1 / u_scale
 * is folded into the epilogue's scale (exact).  Needs |activation| < ~650 (fp16 range of the transformed input; not checked).
 * lm_conv3x3_winograd44_split_twin_f32: the materialising twin with identical bits (wu = U * u_scale as [36][CoutP][Cin] fp32). */
int lm_wino44_split_fragments(void* stream, const float* frag, float* out, long n_quads);
int lm_conv3x3_winograd44_split_f32(void* stream, const float* x, int ldx, const float* wu_split, int CoutP, const float* scale,
                                    const float* shift, const float* res, int ldr, float* y, int ldy, int B, int H, int W,
                                    int Cin, int Cout, int dil, int act, double* gn_partial, float post);
int lm_conv3x3_winograd44_split_twin_f32(void* stream, const float* x, int ldx, const float* wu, int CoutP, const float* scale,
                                         const float* shift, const float* res, int ldr, float* y, int ldy, int B, int H, int W,
                                         int Cin, int Cout, int dil, int act, void* workspace, long workspace_bytes, float post);

/* Same convolution + first pass of GroupNorm(C,C) (postprojector.py:512-515,608-647): also writes per (image, 64-row
 * chunk, channel) sum / sum of squares of the outputs, gn_partial [B][Ho*Wo/64][Cout][2] doubles -> lm_gn_finalize. */
int lm_conv2d_nhwc_mfma_f32_gnstats(void* stream, const float* x, int ldx, const float* wp, int CoutP, const float* shift,
                                    float* y, int ldy, double* gn_partial, int B, int H, int W, int Cin, int Cout,
                                    int KH, int KW, int stride, int pad_h, int pad_w, int dil);
int lm_gn_finalize(void* stream, const double* partial, float* stats, int B, int HW, int C, int nchunk, float eps);
/* same values, laid out per channel group: stats [split][B][C / split][2] (two branches sharing one merged convolution) */
int lm_gn_finalize_split(void* stream, const double* partial, float* stats, int B, int HW, int C, int nchunk, float eps, int split);

/* ---- thin layers ---------------------------------------------------------------------------------------------
 * stem: relu(bn1(conv1(x))) for planar x [B,3,H,W] -> NHWC [B,H/2,W/2,64]; w_k64 = [7][7][3][64]
 * (postprojector.py:458-460,566).  maxpool: 3x3 stride 2 pad 1 (:461,567).
 * small: direct conv for Cout <= 16 (feature_layer/output_layer_* :509-511,628-651; head_common_layers,
 * orient, bi_seg_proposal heads/polyline_fpn_vit_vertex_2.py:183-189,232-237,249); w_tc16 = [KH*KW][Cin][16];
 * y = act(conv(pre_relu ? relu(x) : x) * scale + shift).  Cout = 32, 48 or 64 (generate_line_proposal :48-61):
 * w_tc16 = Cout/16 consecutive [KH*KW][Cin][16] blocks, block i holding outputs 16 i .. 16 i + 15. */
int lm_stem_conv7x7_bn_relu(void* stream, const float* x_chw, const float* w_k64, const float* scale,
                            const float* shift, float* y_nhwc, int B, int H, int W);
/* The stem on a u8 HWC tile [B][H][W][3] as the rasteriser / PNG reader emit it (u8 / 255 = the reference's to_tensor,
 * datasets/laserlane_proposals.py:85-98, applied while staging): same bits as tile_ingest + the f32 stem, a quarter of the bytes. */
int lm_stem_conv7x7_bn_relu_u8(void* stream, const unsigned char* x_hwc3, const float* w_k64, const float* scale,
                               const float* shift, float* y_nhwc, int B, int H, int W);
int lm_maxpool3x3s2_nhwc(void* stream, const float* x, float* y, int B, int H, int W, int C);
int lm_conv2d_nhwc_small(void* stream, const float* x, int ldx, const float* w_tc16, const float* scale,
                         const float* shift, float* y, int ldy, int B, int H, int W, int Cin, int Cout,
                         int KH, int KW, int stride, int pad_h, int pad_w, int pre_relu, int act);

/* ---- normalisation / resampling (postprojector.py:512-515,541-561,608-651; vitsegnet.py:20-26,180) ----------
 * gn_stats: per-(b,c) mean, rstd of GroupNorm(C,C) -> stats [B][C][2]; workspace from lm_gn_stats_workspace_bytes.
 * gn_relu_upsample: y (= | +=) bilinear_align_corners(relu(gn(x))) to Ho x Wo.
 * upsample_bilinear_*: F.interpolate(mode='bilinear', align_corners=True); `add` (optional) is summed in. */
int lm_gn_stats(void* stream, const float* x, double* workspace, float* stats, int B, int HW, int C, float eps);
long lm_gn_stats_workspace_bytes(int B, int HW, int C);
int lm_gn_relu_upsample(void* stream, const float* x, const float* stats, const float* gamma, const float* beta,
                        float* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int accumulate);
/* y = ((t0 + t1) + t2), t_k = bilinear_align_corners(relu(gn(x[k]; stats[k], gamma, beta))) from Hi[k] x Wi[k] to Ho x Wo, n <= 3
 * terms sharing gamma / beta: `s2 + s3 + s4` of one semantic branch (postprojector.py:615-621, :641-647) in one pass. */
int lm_gn_relu_upsample_sum(void* stream, int n, const float* const* x, const float* const* stats, const int* Hi, const int* Wi,
                            const int* ldx /* floats between pixels per term, NULL = C */, const float* gamma, const float* beta,
                            float* y, int B, int Ho, int Wo, int C);
/* The same sum followed by a 1x1 convolution y1[pixel][0..cout) = sum[pixel][:] @ w + bias (cout <= 8; w_c16 = [C][16] layout of
 * lm_conv2d_nhwc_small; C/4 a power of two <= 64): feature_layer / output_layer_endp (postprojector.py:628-651).  y may be NULL: the
 * C-channel sum is then never written. */
int lm_gn_relu_upsample_sum_conv1x1(void* stream, int n, const float* const* x, const float* const* stats, const int* Hi, const int* Wi,
                                    const int* ldx, const float* gamma, const float* beta, float* y, int B, int Ho, int Wo, int C,
                                    const float* w_c16, const float* bias, int cout, float* y1, int ldy1);
int lm_upsample_bilinear_nhwc(void* stream, const float* x, int ldx, const float* add, int lda, float* y, int ldy,
                              int B, int Hi, int Wi, int Ho, int Wo, int C);
int lm_upsample_bilinear_to_chw(void* stream, const float* x, int ldx, float* y_chw, int B, int Hi, int Wi,
                                int Ho, int Wo, int C);
/* nn.LayerNorm over rows of D floats: D % 32 == 0, 32 <= D <= 4096, D != 768 */
int lm_layernorm_rows(void* stream, const float* x, const float* gamma, const float* beta, float* y,
                      long rows, int D, float eps);
int lm_unpatchify(void* stream, const float* tokens, float* y_nhwc, int B, int G, int P, int C);
/* MLP-Mixer token mixing (mixsegnet.py:24-31,55-58: Conv1d(K -> M, kernel 1) over the token axis of every channel):
 * y[b] = act(W x[b] + bias) (+ res[b]) for b < B.  x [B*K][N], res / y [B*M][N] row-major (N % 4 == 0, 16-byte aligned);
 * wt = W^T zero padded to [ceil(K/16)*16][ldw], ldw = M rounded up to a multiple of 128; bias [M] (one value per output token);
 * act LM_ACT_NONE or LM_ACT_GELU (erf); res may be NULL.  Exact fp32 (v_mfma_f32_32x32x2_f32). */
int lm_token_mix_mfma_f32(void* stream, const float* x, const float* wt, int ldw, const float* bias, const float* res, float* y,
                          int B, int M, int K, int N, int act);

/* ---- attention core: softmax(q k^T * scale) v per (batch, head); qkv = [B*N][3*heads*64] (vitsegnet.py:58-68).  Any N >= 1, routed by N
 * alone: 321 <= N <= 352 (the ViT block's 324 tokens) runs on the matrix cores with the whole head's K / V in LDS; every other N <= 380
 * runs the VALU kernel, whose LDS (404 N + 9792 dynamic + 272 static bytes) reaches 163584 of the CU's 163840 bytes at N = 380; N >= 381
 * (ViT patches 6 / 4) streams K / V through LDS with an online softmax.  Deterministic, no workspace. */
int lm_attention_f32(void* stream, const float* qkv, float* out, int B, int N, int heads, int dim_head, float scale);
/* the same with a key mask, valid [B][N] ints (N <= 64): per batch element only the flagged tokens are keys, compacted in token order
 * (row_shared_not_reduc_ref.py:199-215: the transformer runs over the data-dependent subset of the lane tokens) */
int lm_attention_masked_f32(void* stream, const float* qkv, float* out, const int* valid, int B, int N, int heads, int dim_head, float scale);

/* ---- column-proposal head (heads/polyline_fpn_vit_vertex_2.py:390-421) ----------------------------------------
 * tokens: tok[(b,p,h), c*10+w] = avg_pool8(up(seg window p))[h,w] * row_fea_pad[b,c,h,2p+w]   (:392-405)
 * stage2: second Conv1d of ext2/cls2/offset2 (:210,218,226); proposal_conf: Linear(23040 -> 2) (:200-204) */
int lm_head_tokens(void* stream, const float* seg, const float* row_nhwc16, float* tok, float seg_bias,
                   int B, int P, int Hr, int Wr, int prop_width, int half_buff);
/* spatial_att=False (polyline_fpn_vit_vertex_2.py:403-404): the tokens are the raw zero-padded row window, no seg map */
int lm_head_tokens_window(void* stream, const float* row_nhwc16, float* tok, int B, int P, int Hr, int Wr, int prop_width, int half_buff);
int lm_head_stage2(void* stream, const float* hid, int ldh, int D, const float* w2, const float* b2,
                   float* ext2, float* cls2, float* off2, long M);
int lm_head_proposal_conf(void* stream, const float* tok, const float* wt, const float* bias, float* conf,
                          int BP, int L);

/* ---- heads.endp_mode = 'endpoint' (heads/polyline_fpn_vit_vertex_2.py:254-260, :371-373): the head's own endpoint map, one fused kernel
 *   out [B][1][H][W] = conv3x3(t; w2, pad 1) + b2,   t = bn_scale * relu(conv3x3(a; W1, pad 1) + b1) + bn_shift (0 outside the image),
 *   a = relu(cat(bilinear_align_corners(col -> H x W), x_endp)) (0 outside the image)
 * col: NHWC [B][h][w][ldc], its first 16 channels (ldc >= 16: a slice of a wider buffer); x_endp [B][1][H][W]; w1p = W1 [4][17][3][3]
 * as [17][3][3][4]; b1, bn_scale, bn_shift [4]; w2 [4][3][3]; b2 [1].  Any h, w, H, W >= 1 (scale (h - 1) / (H - 1), 0 where H = 1).
 * The [B,17,H,W] concatenation is never built; exact fp32 in a fixed order, so a tile's map does not depend on B or on its place in
 * the batch.  lm_head_endpoint_tile: the edge of the output tile one workgroup owns (the sizes the tests straddle).
 * NOTE on the name `hip_stream`: as for lm_strip_bin_points below - tests/test_bounds_inventory_cpu.py finds device entries by the spelling
 * `stream` and demands their guarded-buffer case in tests/test_gpu_1_bounds.py; this entry's case is
 * tests/test_gpu_endpoint_mode.py::test_head_endpoint_kernel_bounds, which that inventory does not read. */
int lm_head_endpoint_tile(void);
int lm_head_endpoint(void* hip_stream, const float* col, int ldc, const float* x_endp, const float* w1p, const float* b1,
                     const float* bn_scale, const float* bn_shift, const float* w2, const float* b2, float* out, int B, int h, int w,
                     int H, int W);

/* ---- decode (heads/polyline_fpn_vit_vertex_2.py:602-759; postprojector.py:115-183) ---------------------------
 * proposals: :610, :694-697, :701-702, :726-738.  orient: :615.  semantic: :627-632 (raw_mode=1: :122-127).
 * endp_topk: sigmoid of logits cropped by `clip` px, K best in (score desc, flat index asc) order (:647-668);
 * out_status[b] = 1 if more tied scores than the candidate buffer holds. */
int lm_decode_proposals(void* stream, const float* pconf, const float* ext2, const float* cls2, const float* off2,
                        float* prop_conf, float* v_ext, float* cls_conf, int* cls_idx, double* cls_offset,
                        int B, int P, int R, float exist_thre, int prop_width, int half_buff);
int lm_decode_orient(void* stream, const float* x_nhwc, int ldx, int C, unsigned char* y, long pixels);
int lm_decode_semantic(void* stream, const float* logit_chw3, unsigned char* sem, float* biseg, float* rows,
                       int B, int H, int W, float thre, int raw_mode);
long lm_endp_topk_workspace_bytes(int B);
int lm_endp_topk(void* stream, const float* endp_logit, void* workspace, int* out_idx, float* out_score,
                 int* out_status, int B, int H, int W, int clip, int K);

/* Gathers up to 8 device segments (bytes[s] % 4 == 0) into one block at dst + dst_offsets[s] (% 16 == 0): the decode outputs the host
 * post-processing reads (prop_conf, v_ext, cls_offset, rows, idx, status) then travel in ONE device-to-host copy per batch - the per-batch
 * body of Runner.infer_lane_coordinate_endpoint_semantics (baseline/engine/runner.py:725-740) moves them with one .cpu() per tensor. */
int lm_pack_segments(void* stream, int n, const void* const* src, const long* bytes, const long* dst_offsets, void* dst);


/* ---- LAS -> BEV rasteriser and tile ingest (build-defined, parity unpinned: the reference has no rasteriser;
 * pinned pieces: datasets/laserlane_proposals.py:85-98,618-636; utils/coor_img2pc.py:127-183;
 * utils/io_utils.py:125-150) */
typedef struct {
    float quat[4];            /* [w,x,y,z] = las_rotation_trans_quan[3:7] */
    float trans[3];           /* las_rotation_trans_quan[0:3] */
    float bev_img_offset[2];
    float img_reso[2];
    float local_min_ele;
    float ele_reso;
    float inten_lo, inten_hi; /* 800, 33000 */
} LmRasterParams;
/* points: device [sum N][4] f32 {x,y,z,raw intensity}; tile_offsets: HOST [B+1] point index of each tile's first
 * record; params: HOST [B]; out_chw [B][3][H][W] f32 (= u8/255), out_hwc_u8 [B][H][W][3] (either may be NULL).
 * Tile size: H a multiple of 16 or 12 with at most 96 bands of that many rows, and one band image (rows * W * 4 bytes) within the CU's
 * 160 KB of LDS: rows * W <= 40960, i.e. W <= 2560 where H is a multiple of 16 and W <= 3413 where H is a multiple of 12.  Any other
 * size is refused with LM_ERR_ARG before anything is launched, and lm_bev_raster_workspace_bytes returns 0 for it. */
long lm_bev_raster_workspace_bytes(int B, long max_points_per_tile, int H, int W);
int lm_bev_raster_batch(void* stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params,
                        int B, void* workspace, long workspace_bytes, float* out_chw, unsigned char* out_hwc_u8,
                        int H, int W);
/* bev_raster_batch_scaled: lm_bev_raster_batch with a per-tile intensity scale.  inten_scale: HOST [B] or NULL.  Where it is given and
 * positive it replaces the tile's derived scale 255 / inten_hi: I = clamp(floor((clip(i, inten_lo, inten_hi) - inten_lo) * scale + .5),
 * 1, 255), so that a window lo..hi can be stretched over the whole channel (scale = white / (hi - lo)); NULL or a non-positive entry: the
 * derived scale, i.e. lm_bev_raster_batch, which is this call with NULL.  The scale is a per-tile kernel argument either way: host side
 * only, the kernels are the same.  Bounds cases: tests/test_gpu_intensity.py::test_scaled_raster_guards (see the NOTE on `hip_stream`
 * under the ground model below). */
int lm_bev_raster_batch_scaled(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params,
                               int B, void* workspace, long workspace_bytes, float* out_chw, unsigned char* out_hwc_u8,
                               int H, int W, const float* inten_scale);
int lm_tile_ingest_u8(void* stream, const unsigned char* src_hwc, float* dst_chw, int B, int H, int W, int C);

/* ---- strip binning (csrc/strip.hip): one cloud + T tile windows -> the per-tile point ranges lm_bev_raster_batch takes ------------
 * A survey strip arrives as one cloud and a tile layout (one parameter file per 1152 x 1152 window; windows overlap and may be rotated).
 * binned = the points of tile 0, then tile 1, ... ; a point is in tile t exactly when the rasteriser would not drop it for t (the same
 * window test on the same host-derived constants), possibly in several tiles or in none; inside a tile the cloud's order is kept.
 * Deterministic: count, scan (lm_exclusive_scan_u32's kernels), scatter; every slot reserved by a prefix, no atomics.
 * points: device [N][4] f32, N <= 2^31 - 1; params: HOST [T], T <= 4096; counts [T], offsets [T+1]: DEVICE int64; offsets_host: HOST
 * [T+1] or NULL; binned: device [capacity][4] f32.  [z_lo, z_hi]: the range of z the point-to-tile grid is built for (tilted tiles: it
 * must be finite; points outside it are still binned correctly, only slower; -inf / +inf when no tile is tilted).
 * NOTE on the name `hip_stream`: every other entry calls this parameter `stream`.  tests/test_bounds_inventory_cpu.py finds device entries by
 * that spelling and demands a guarded-buffer case for each in tests/test_gpu_1_bounds.py; this entry's case is
 * tests/test_gpu_strip.py::test_strip_bin_guards, which that inventory does not read.  To be renamed to `stream` together with a
 * BOUNDS_EXEMPT line (or a moved case) in test_gpu_1_bounds.py.
 * UNLIKE the other entries this one synchronises its stream once: offsets[T] = the number of binned points is read back before the
 * scatter; if it exceeds `capacity`, nothing is written to binned and LM_ERR_CAPACITY is returned (offsets / offsets_host are valid:
 * allocate offsets[T] points and call again).  More than 8 tiles reaching into one grid cell is refused (LM_ERR_ARG, the message has the
 * cell): the limit counts tiles per cell - cells of a quarter of the smallest footprint, halved up to three times - not tiles per point.
 * lm_strip_build_grid: the HOST routine behind the point-to-tile lookup (no GPU is touched): a uniform grid of nx x ny cells of size
 * `cell` from (x0, y0) over the union of the tile footprints; cells (NULL: geometry only) receives [ny][nx][8] tile indices, 0xFFFF =
 * none, a superset of the tiles whose window a point of that cell with z in [z_lo, z_hi] can fall into. */
typedef struct {
    double x0, y0, cell;
    int nx, ny;
} LmStripGrid;
int lm_strip_build_grid(const LmRasterParams* params, int T, int H, int W, double z_lo, double z_hi, LmStripGrid* grid,
                        unsigned short* cells, long cells_cap);
long lm_strip_bin_workspace_bytes(long N, int T);
int lm_strip_bin_points(void* hip_stream, const float* points_xyzi, long N, const LmRasterParams* params, int T, int H, int W,
                        double z_lo, double z_hi, void* workspace, long workspace_bytes, long* counts, long* offsets,
                        long* offsets_host, float* binned, long capacity);

/* ---- strip binning, chunk by chunk (csrc/strip.hip): the same binned / offsets pair for a strip that is never held as one cloud ------
 * lm_strip_bin_points needs the whole cloud on the device beside its output.  The chunked form takes the strip as consecutive chunks,
 * twice: pass A counts every chunk into one running row of per-tile counts; the caller reads that row once, lays out binned by its
 * exclusive prefix - for all tiles, or for a run of consecutive tiles at a time - and pass B scatters every chunk behind per-tile cursors.
 * Inside a tile the points keep the order of the chunks, and inside a chunk their own: bit for bit what lm_strip_bin_points gives for
 * the chunks concatenated, whatever the chunk sizes (the membership test never depends on the lookup grid, and a slot depends only on
 * the number of points of the tile before the point).  The kernels are those of lm_strip_bin_points: strip_pass_kernel counts, the scan
 * is lm_exclusive_scan_u32's, strip_pass_kernel scatters, reading the cursors where it reads offsets there; the instantiation that
 * scatters behind cursors also checks every slot against `capacity`.  A one-workgroup kernel (a tile per thread and step, no atomics, no
 * LDS) adds the chunk's per-tile totals to the running row, in stream order.
 * THE PLAN.  The host grid and the tile constants of a layout do not depend on the chunk; with hundreds of chunks per strip they are
 * built and uploaded once, by lm_strip_plan_create, into `consts` - DEVICE memory of the caller (lm_strip_plan_consts_bytes(T, nx ny) bytes
 * for the nx x ny cells lm_strip_build_grid reports, 16-byte aligned) that must stay alive and untouched while the plan is used.  The handle itself is host memory, freed by
 * lm_strip_plan_destroy (NULL is LM_OK).  A plan for a sub-list of `params` bins into those tiles only.  plan_create refuses what
 * lm_strip_bin_points refuses of the shared arguments (T outside 1 .. 4096, more than 8 tiles reaching into one grid cell, a tilted tile
 * with an infinite z range, a degenerate tile), copies host memory to the device and synchronises the stream, so it also refuses a
 * capturing stream; the other entries are asynchronous, read nothing back and may be captured.
 * lm_strip_bin_count:   points DEVICE [N][4] f32, 16-byte aligned, N <= 2^31 - 1 PER CHUNK (the strip's total is not bounded);
 *         workspace DEVICE, lm_strip_chunk_workspace_bytes(N, T) bytes; counts_accum DEVICE [T] int64, owned and zeroed by the caller:
 *         counts_accum[t] += the chunk's points of tile t.
 * lm_strip_bin_scatter: cursors DEVICE [T] int64, in and out.  The point of tile t with rank r among the chunk's points of t goes to
 *         binned[cursors[t] + r]; afterwards cursors[t] has grown by the chunk's count of t.  binned DEVICE [capacity][4] f32.  A slot
 *         outside [0, capacity) is NOT written; 1 is stored to err (DEVICE, one int, zeroed by the caller; a vector store) instead, and
 *         the cursors advance all the same.  Whatever the cursors hold, nothing is written outside binned[0 .. capacity).
 * N = 0 is LM_OK and launches nothing.  Refused with LM_ERR_ARG and a message that names the argument: a plan that is no handle, N,
 * null or misaligned points / workspace / counts_accum / cursors / binned / err, a workspace too small, a negative capacity.
 * NOTE on the place of `hip_stream`: as for lm_line_hist_points below, these entries take the stream as their LAST parameter: the
 * inventories of tests/test_stream_inventory_cpu.py, tests/test_bounds_inventory_cpu.py and tests/lds_state.py find entries by the stream
 * in first place and hold each to a literal table inside an existing test file.  The cases those tables would name - guarded buffers, a
 * side stream, poisoned LDS before strip_pass_kernel<true, true> - are in tests/test_gpu_strip_stream.py.  For the same reason
 * strip_advance_kernel declares no __shared__. */
long lm_strip_plan_consts_bytes(int T, long n_cells);
int lm_strip_plan_create(const LmRasterParams* params, int T, int H, int W, double z_lo, double z_hi, void* consts, long consts_bytes,
                         void** plan, void* hip_stream);
int lm_strip_plan_destroy(void* plan);
long lm_strip_chunk_workspace_bytes(long N, int T);
int lm_strip_bin_count(const void* plan, const float* points_xyzi, long N, void* workspace, long workspace_bytes, long* counts_accum,
                       void* hip_stream);
int lm_strip_bin_scatter(const void* plan, const float* points_xyzi, long N, void* workspace, long workspace_bytes, long* cursors,
                         float* binned, long capacity, int* err, void* hip_stream);

/* ---- per-tile ground model (csrc/ground.hip): a coarse grid of ground heights under every tile, and the selection of points by their
 * height above it.  Both entries take the (points, tile_offsets, params) triple of lm_bev_raster_batch: points DEVICE [sum N][4] f32
 * (16-byte aligned), tile_offsets HOST [B+1] (non-decreasing), params HOST [B]; 1 <= B <= 4096 in one call, at most 2^31 - 1 points
 * between tile_offsets[0] and tile_offsets[B].  A point counts for tile b exactly when the rasteriser keeps it for b (the shared window
 * test of csrc/raster_xf.h) AND its tile-frame height vz - the value the rasteriser turns into G - is finite.
 * The cell grid is Gy = ceil(H / cell_px) by Gx = ceil(W / cell_px), 8 <= cell_px <= 128, at most 32768 cells per tile; the cell of a
 * point is (row / cell_px, col / cell_px) of its pixel.
 * tile_ground:  cell_min [B][Gy][Gx] f32 (may be NULL) = the smallest vz of the cell's points, NaN = no point.  Minima are taken on an
 *               order-preserving integer key of the float (so -0.0 < +0.0) with integer atomics: the same bits every run.
 *               ground   [B][Gy][Gx] f32 = the LOWER MEDIAN (element (k - 1) / 2 of the k values in ascending order) of the non-empty
 *               cells among the 3 x 3 neighbourhood clipped at the grid edge, NaN when all of them are empty.  A cell that holds a point
 *               always gets a finite ground; a single outlier cell among filled neighbours does not show.
 *               ground_min [B] f32 = the minimum of the tile's finite ground cells, +inf for a tile without any.
 *               workspace: device, lm_tile_ground_workspace_bytes(B, H, W, cell_px) bytes (0 = unsupported arguments).  Asynchronous.
 * ground_select: a point of tile b is kept when it counts for b (above) and h_lo <= vz - ground[b][cell] <= h_hi, one f32 subtraction;
 *               -inf / +inf switch a side off, a NaN bound or h_lo > h_hi is refused; a NaN ground keeps nothing.  ground is
 *               tile_ground's output for the same B, H, W, cell_px.  points_out: DEVICE [tile_offsets[B] - tile_offsets[0]][4], a buffer
 *               of its own; rows [out_offsets[b], out_offsets[b+1]) receive tile b's kept points in their input order, bit for bit; rows
 *               from out_offsets[B] on are not written.  out_offsets: DEVICE [B+1] int64, out_offsets[0] = 0.  out_offsets_host: HOST
 *               [B+1] or NULL; when given, the stream is synchronised once (as lm_strip_bin_points does) and it holds the same numbers.
 *               Count per 256-point block (blocks never straddle two tiles), exclusive scan (lm_exclusive_scan_u32's kernels), emit to
 *               block offset + ballot rank: no atomics, the same bits every run.  workspace: device,
 *               lm_ground_select_workspace_bytes(N, B) bytes with N = tile_offsets[B] - tile_offsets[0].
 * Bad arguments are refused with LM_ERR_ARG and a message that names the argument (cell_px, h_lo, h_hi, tile_offsets, B).
 * NOTE on the name `hip_stream`: as for lm_strip_bin_points above - tests/test_bounds_inventory_cpu.py finds device entries by the spelling
 * `stream` and demands their guarded-buffer case in tests/test_gpu_1_bounds.py; the cases of these two entries are
 * tests/test_gpu_ground.py::test_tile_ground_guards and ::test_ground_select_guards, which that inventory does not read. */
long lm_tile_ground_workspace_bytes(int B, int H, int W, int cell_px);
int lm_tile_ground(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H,
                   int W, int cell_px, void* workspace, long workspace_bytes, float* ground, float* ground_min, float* cell_min);
long lm_ground_select_workspace_bytes(long N, int B);
int lm_ground_select(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H,
                     int W, int cell_px, const float* ground, float h_lo, float h_hi, void* workspace, long workspace_bytes,
                     float* points_out, long* out_offsets, long* out_offsets_host);

/* ---- intensity window per tile or group of tiles (csrc/intensity.hip): two percentiles of the intensities of the points a tile keeps,
 * for a rasteriser window that fits the scanner and the strip instead of the reference's constants 800 / 33000.
 * (points, tile_offsets, params, B, H, W) as for lm_tile_ground; fewer than 2^32 points between tile_offsets[0] and tile_offsets[B] (the
 * counters are 32-bit).  group: HOST [B], values in 0..G-1: the tiles of a group are counted together; NULL: tile b is group b, G == B.
 * 1 <= G <= B <= 4096.  q_lo_ppm, q_hi_ppm: the two quantiles in parts per million, 0 <= q_lo_ppm <= q_hi_ppm <= 1000000.
 * A point counts for tile b exactly when the rasteriser keeps it for b (the shared window test of csrc/raster_xf.h) and its intensity
 * p[3] is not NaN.  Its key is k = (int)floorf(fminf(fmaxf(i, 0), 65535)): LAS intensities are u16, so the key is the intensity;
 * non-integer, negative, larger and infinite values clamp.  With n = the counted points of group g over all its tiles:
 *   window [G][2] int32, DEVICE: window[g][0] = the key of 0-based rank (n - 1) * q_lo_ppm / 1000000 (64-bit integer floor division) among
 *                 the group's keys in ascending order - the lower order statistic, a value that occurs in the data; window[g][1] the same
 *                 with q_hi_ppm; (-1, -1) for n = 0
 *   count [G] int64, DEVICE: n
 *   coarse_hist [G][4096] u32, DEVICE, or NULL: the number of counted points with k >> 4 == bin
 * Exact: a histogram of k >> 4 per group (LDS, then integer atomic adds), the two coarse bins that hold the ranks, a second pass that
 * counts the 16 keys of each of the two bins.  Integer adds are order independent: the same bits on every run and stream.  Asynchronous,
 * no host synchronisation.  workspace: device, 16-byte aligned, lm_tile_intensity_workspace_bytes(B, G) bytes (0 = unsupported arguments).
 * Bad arguments are refused with LM_ERR_ARG and a message that names the argument (B, G, group, q_lo_ppm, q_hi_ppm, tile_offsets,
 * workspace, null pointer).
 * NOTE on the name `hip_stream`: as for lm_tile_ground above; the guarded-buffer case is tests/test_gpu_intensity.py::
 * test_tile_intensity_window_guards. */
long lm_tile_intensity_workspace_bytes(int B, int G);
int lm_tile_intensity_window(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B,
                             int H, int W, const int* group, int G, int q_lo_ppm, int q_hi_ppm, void* workspace, long workspace_bytes,
                             int* window, long* count, unsigned* coarse_hist);

/* ---- intensity balance per ground cell (csrc/intensity.hip).  A mobile scanner's intensity falls with range: under any single window
 * the outer lanes of a strip rasterise as dark paint on black and the near lane as grey asphalt brighter than that paint.  So before
 * the window is fitted, the binned points are balanced: a local asphalt level per cell, a gain per cell towards one reference level,
 * and every point's intensity multiplied by the gain interpolated between the cell centres.  THE RULE (one definition: this text;
 * tests/balance_ref.py restates it in numpy):
 * WHICH POINTS COUNT.  (points, tile_offsets, params, B, H, W) as for lm_tile_ground, at most 2^31 - 1 points between tile_offsets[0]
 *     and tile_offsets[B].  A point counts for tile b when the window test of csrc/raster_xf.h, lm_point_window, keeps it for b and its intensity p[3] is
 *     not NaN.  Its key is lm_tile_intensity_window's: k = (int)floorf(fminf(fmaxf(i, 0), 65535)).  Its cell is (row / cell_px,
 *     col / cell_px) on lm_tile_ground's grid Gy = ceil(H / cell_px) by Gx = ceil(W / cell_px); 16 <= cell_px <= 128, at most 32768
 *     cells per tile.
 * LEVEL, COUNT, MODEL (lm_tile_intensity_cells; all DEVICE [B][Gy][Gx] int32).
 *     count[b][cy][cx] = n, the counted points of the cell.
 *     level[b][cy][cx] = the key of 0-based rank (n - 1) * q_ppm / 1000000 (64-bit integer floor division) among the cell's n keys in
 *         ascending order; q_ppm = 500000 is the lower median - the asphalt level, paint being the minority of a road cell.  -1 for
 *         n = 0.
 *     A cell is KNOWN when n >= min_points.
 *     model[b][cy][cx] = the LOWER MEDIAN (element (k - 1) / 2 of the k values in ascending order) of `level` over the known cells of
 *         the 3 x 3 neighbourhood clipped at the grid edge, the cell itself included; -1 when none is known.  lm_tile_ground's
 *         smoothing on integers: a cell that is mostly paint (a crossing, hatching) does not dim itself.
 *     Exact in two levels of 256 x 256 keys: rows of 256 u32 counters per cell in the workspace, added to with integer global atomics
 *     (the lanes of a wave that hit one counter are merged first); a wave per cell finds the bin of the rank with a prefix sum over
 *     its lanes.  Integer adds only: the same bits on every run, whatever the order of the points.
 *     workspace: device, 16-byte aligned, lm_tile_intensity_cells_workspace_bytes(B, H, W, cell_px) bytes - 1 KiB per cell, so callers
 *     with many tiles call in groups of tiles (0 = unsupported arguments).
 * GAINS are host policy (las_io.balance_gains): for a known model and a reference level r > 0, clip((f32)r / (f32)max(model, 1),
 *     1 / max_gain, max_gain), else 1; float32.
 * APPLY (lm_tile_intensity_apply).  gains DEVICE [B][Gy][Gx] f32; out DEVICE [tile_offsets[B]][4] f32 (rows from tile_offsets[0] on are
 *     written), 16-byte aligned; it may be points_xyzi itself.  For a point that counts, at pixel (row, col):
 *         u  = (f32)(2 col + 1 - cell_px) / (f32)(2 cell_px), clamped to [0, Gx - 1]       the position between the cell centres
 *         x0 = floor(u), fx = u - x0, x1 = min(x0 + 1, Gx - 1); v, y0, fy, y1 the same from row and Gy
 *         g  = (g[y0][x0] (1 - fx) + g[y0][x1] fx) (1 - fy) + (g[y1][x0] (1 - fx) + g[y1][x1] fx) fy
 *         i' = fminf(i g, 65535)
 *     every operation rounded on its own (__fmul_rn, __fadd_rn, __fsub_rn, __fdiv_rn: no contraction decides a bit).  x, y and z are
 *     stored back as they are; a point that does not count is stored back unchanged in every bit.  Bilinear between the cell centres,
 *     so no cell seam appears in the image - a step at a seam would look like a line to the network.  One streaming pass, 16 bytes
 *     read and 16 written per point.  workspace: device, 16-byte aligned, lm_tile_intensity_apply_workspace_bytes(B) bytes.
 * Both entries copy the tile table from host memory of the call: asynchronous, no synchronisation, and a capturing stream is refused
 * by name.  B = 0 is LM_OK and touches nothing.  Refused with LM_ERR_ARG and a message that names the argument, before anything is
 * launched or written: B outside 1 .. 4096; cell_px outside 16 .. 128 or more than 32768 cells; q_ppm outside 0 .. 1000000;
 * min_points < 0; a null or misaligned pointer (points, workspace: 16 bytes; level, count, model, gains: 4; out: 16); a workspace too
 * small; decreasing tile_offsets.
 * NOTE on the place of `hip_stream`: LAST, as for lm_line_hist_points below and for the same reason: the inventories of
 * tests/test_stream_inventory_cpu.py, tests/test_bounds_inventory_cpu.py and tests/lds_state.py find entries by the stream in first
 * place and hold each to a literal table inside an existing test file.  The cases those tables would name - guarded buffers around
 * every operand and the workspace, a side stream beside a busy default stream, the refusal on a capturing stream - are in
 * tests/test_gpu_balance.py.  For the same reason none of the kernels of these entries declares __shared__. */
long lm_tile_intensity_cells_workspace_bytes(int B, int H, int W, int cell_px);
int lm_tile_intensity_cells(const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H, int W,
                            int cell_px, int q_ppm, int min_points, void* workspace, long workspace_bytes, int* level, int* count,
                            int* model, void* hip_stream);
long lm_tile_intensity_apply_workspace_bytes(int B);
int lm_tile_intensity_apply(const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H, int W,
                            int cell_px, const float* gains, void* workspace, long workspace_bytes, float* out, void* hip_stream);

/* ---- vertex heights from the points (csrc/drape.hip): a pixel-scale ground model around the polyline vertices of every tile.
 * (points, tile_offsets, params, H, W) as for lm_tile_ground, 0 <= B <= 4096, H and W at most 32768.  vertices_rc: HOST [V][2] int32
 * (row, col), the vertex pixels of tile 0, then tile 1, ...; vertex_offsets: HOST [B+1], vertex_offsets[0] = 0, non-decreasing,
 * V = vertex_offsets[B]; at most 16384 vertices per tile; every vertex satisfies 0 <= row < H, 0 <= col < W.  0 <= radius_px = R <= 8.
 * A point counts for tile b exactly when the rasteriser keeps it for b (the shared window test of csrc/raster_xf.h) and its tile-frame
 * height vz - the quantity G * ele_reso + local_min_ele approximates - is finite.  Vertex v of tile b owns (2R+1)^2 slots; slot (i, j),
 * i, j in -R..R, is the smallest vz (on lm_tile_ground's order-preserving integer key: -0.0 < +0.0) over the tile's points in pixel
 * (row + i, col + j); a window pixel outside the tile stays empty.  One point serves every vertex whose window holds its pixel.
 *   z [V] f32, DEVICE: the LOWER MEDIAN (element (k - 1) / 2 of the k non-empty slots in ascending order), NaN for k = 0
 *   npix [V] int32, DEVICE: k
 *   pixel_min [V][2R+1][2R+1] f32, DEVICE, or NULL: the slots, NaN = empty
 * Integer atomic min on slots preset to all-ones: order independent, the same bits every run.  Asynchronous; no read-back.
 * workspace: device, 16-byte aligned, lm_drape_workspace_bytes(V, B, R) bytes (0 = unsupported arguments).  B = 0 or V = 0: LM_OK, nothing
 * is launched or written.  Bad arguments are refused with LM_ERR_ARG and a message that names the argument (radius_px, B, tile_offsets,
 * vertex_offsets, vertex, workspace, null pointer) before anything is launched.
 * NOTE on the name `hip_stream`: as for lm_tile_ground above; the guarded-buffer case is tests/test_gpu_drape.py::
 * test_drape_vertices_guards. */
long lm_drape_workspace_bytes(long n_vertices, int B, int radius_px);
int lm_drape_vertices(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H,
                      int W, const int* vertices_rc, const long* vertex_offsets, int radius_px, void* workspace, long workspace_bytes,
                      float* z, int* npix, float* pixel_min);

/* ---- gap fill of sparse tiles (csrc/gapfill.hip): the stage between the rasteriser and the network for scanners that deliver fewer
 * returns than pixels.  tiles_hwc_u8: DEVICE u8 [B][H][W][3], lm_bev_raster_batch's out_hwc_u8 or a decoded PNG; 1 <= B <= 4096,
 * 1 <= H, W <= 32768.  A pixel is EMPTY when its three bytes are 0 (the reference's R + G + B < 1); its VALUE is R << 16 | G << 8 | B.
 *   gap   of an empty pixel p for a maximal radius Rmax: the smallest d2 = dr^2 + dc^2 over the non-empty pixels q of the SAME tile with
 *         d2 <= Rmax^2 - a disc: with Rmax = 1 the four edge neighbours count, the diagonal ones do not.  Pixels outside the tile do not
 *         exist (no wrap into the next row, the neighbouring tile of the batch or padding).  An empty pixel without such a q is FAR.
 *   ring  k of an empty, non-far pixel: the smallest integer with k^2 >= gap (1 for d2 = 1, 2 for 2..4, 3 for 5..9, ...).
 * tile_gap_hist: hist DEVICE u32 [B][max_radius_px + 2], 1 <= max_radius_px = Rmax <= 8, zeroed by the call on the stream:
 *         hist[b][0] = the non-empty pixels, hist[b][k], k = 1..Rmax, = the empty pixels of ring k, hist[b][Rmax + 1] = the far pixels;
 *         every row sums to H W.  Integer atomic adds: order independent, the same bits every run.
 * tile_gap_fill: radius_px HOST int [B], 0 <= radius_px[b] = r <= 8 per tile.  A non-empty pixel keeps its three bytes; an empty pixel
 *         with gap <= r^2 takes the three bytes of the q of smallest d2 within the disc of radius r, ties in d2 to the LARGEST value
 *         (brightest first, then highest elevation: the rule by which the rasteriser itself settles a pixel, so the result is unique by
 *         value); every other pixel stays empty.  Sources are always pixels of the INPUT: no cascading, and out_hwc_u8 [B][H][W][3] is a
 *         buffer of its own that must not overlap the input (refused, exact aliasing included).  r = 0 is a copy.
 * Both are asynchronous, read nothing back to the host and need no workspace.  Bad arguments are refused with LM_ERR_ARG and a message that
 * names the argument (B, H, W, max_radius_px, radius_px[b], null pointer, out_hwc_u8) before anything is launched.
 * NOTE on the name `hip_stream`: as for lm_tile_ground above - tests/test_bounds_inventory_cpu.py finds device entries by the spelling
 * `stream` and demands their guarded-buffer case in tests/test_gpu_1_bounds.py; the cases of these two entries are
 * tests/test_gpu_gapfill.py::test_tile_gap_hist_guards and ::test_tile_gap_fill_guards, which that inventory does not read. */
int lm_tile_gap_hist(void* hip_stream, const unsigned char* tiles_hwc_u8, int B, int H, int W, int max_radius_px, unsigned* hist);
int lm_tile_gap_fill(void* hip_stream, const unsigned char* tiles_hwc_u8, int B, int H, int W, const int* radius_px,
                     unsigned char* out_hwc_u8);

/* ---- host-side tail (HOST pointers; no GPU is touched) --------------------------------------------------------
 * endp_cluster: heads/polyline_fpn_vit_vertex_2.py:661-688 + :903-924.
 * polyline_assemble: :805-861 + baseline/utils/polyline_utils.py (whole file) + :1091-1115.
 * raster_polylines: polyline_utils.py:610-638 (own Bresenham instead of cv2.line). */
int lm_endp_cluster(const int* topk_idx, int n_avail, int Wc, int clip, int k0, int k_step, int k_max, int radius,
                    int min_clusters, int* out_hw, int max_out, int* n_out, int* k_used);
int lm_polyline_assemble(const float* prop_conf, const float* prop_v_ext, const double* cls_offset,
                         const float* bi_seg_rows, const int* endp_hw, int n_endp, int P, int R, float obj_thre,
                         int min_vertices, double* out_lanes, int* endp_keep);
int lm_raster_polylines(const double* lanes, int P, int R, unsigned char* out);
/* One segment of that rasteriser (cv2.line, thickness 1, LINE_8, restated from OpenCV's LineIterator: csrc/postproc.cpp) on a 1152 x 1152 map. */
int lm_line8(unsigned char* out, int x1, int y1, int x2, int y2, int colour);
int lm_trace_lines(const double* cols, int n, int R, const float* seg_rows, double* out);   /* polyline_utils.py:222-387 */
/* BEV polylines -> LAS frame: baseline/utils/coor_img2pc.py:127-183 (+ :22-53, :59-73, :94-122).  bev_hwc [H][W][C] u8 is
 * modified in place (elevation fill of empty vertex pixels, like the reference); img_seqs [L][Vmax][2] (row, col);
 * params13 = img_reso[2], bev_img_offset[2], ele_reso, local_min_ele, las_rotation_trans_quan[7]; out [L][Vmax][3]. */
int lm_polyline_backproject(unsigned char* bev_hwc, int H, int W, int C, const double* img_seqs, const int* seq_lens, int L,
                            int Vmax, const double* params13, const double* las_read_offset, double* out);
/* The same with vertex heights given from outside (lm_drape_vertices).  vertex_z: [L][Vmax] f32, a value that is not finite (NaN) =
 * no height for this vertex; fit: 1 = the least-squares line over the vertex index (step 3 of the reference), 0 = none.
 *   1) the elevation fill runs only for the vertices without a height (and mutates the tile only there)
 *   2) z = (double)vertex_z where it is finite, G * ele_reso + local_min_ele elsewhere; padding slots beyond seq_lens[l] keep the G rule
 *   3) only with fit = 1      4) unchanged
 * With every vertex_z NaN and fit = 1 the output and the tile are bit-identical to lm_polyline_backproject's. */
int lm_polyline_backproject_z(unsigned char* bev_hwc, int H, int W, int C, const double* img_seqs, const int* seq_lens, int L,
                              int Vmax, const double* params13, const double* las_read_offset, double* out,
                              const float* vertex_z, int fit);

/* ---- evaluation: Lee-Kashyap-Chu thinning of a 2-D binary image, the skeletonisation inside the reference's semantic-line F1
 * (baseline/utils/metric_utils.py:415-481 -> skimage.morphology.skeletonize(method='lee')).  PARITY UNPINNED (skimage absent: the
 * published algorithm is restated, csrc/skeleton.cpp).  img [H][W] u8 (nonzero = object) is thinned in place to 0 / 1; returns the
 * number of deleted pixels, -1 on bad arguments. */
long lm_skeletonize_lee_2d(unsigned char* img, int H, int W);

/* ---- cross-tile merge of LAS-frame polylines into map-level lines (baseline/utils/merge_lines.py) ------------------------
 * Streaming host merger: create, one lm_merge_add_tile per tile in sorted file-name order (n polylines, points concatenated
 * [sum lens][3] doubles, every polyline >= 2 vertices; n = 0 for a tile without usable lines), lm_merge_finish (returns the
 * number of merged lines, *total_points their vertex count), lm_merge_result (points [total][3], lens [count]), destroy.
 * merge_lines :166-291, merge_2_seqs :67-104, merge_2_reversed_seqs :106-132, helpers :17-65 / :157-164;
 * lm_downsample_seq = downsample_seqs :133-153 (out holds up to n + 1 points, returns the number kept). */
void* lm_merge_create(void);
void lm_merge_destroy(void* merger);
int lm_merge_add_tile(void* merger, const double* points, const int* lens, int n);
long lm_merge_finish(void* merger, long* total_points);
int lm_merge_result(void* merger, double* points, int* lens);
int lm_downsample_seq(const double* seq, int n, double dist_min, double* out);

/* ---- K-Lane "RowRef" head, config 4 (baseline/models/heads/row_shared_not_reduc_ref.py) ------------------------
 * softmax_rows :179-180,239-240 (in place); select :199-204; gather :207-211; scatter :227-230 (shrinking-range quirk);
 * decode :334-363.  Layouts: x [B,H,W,8] NHWC, ext [B,H,L,2], cls [B,H,L,W], tokens on the fixed grid t = b * L + lane,
 * [B*L][8*H*KW] in (c h w) order, KW = 2*off_grid + 1 (5 in config 4); valid [B][L] = the reference's lane selection (mean existence >
 * thr_ext), computed on the device.
 * gather_win / scatter_win: the window kernels at the head's `off_grid` (:93, :133-134), 1..4 (any other value: LM_ERR_ARG naming
 * off_grid).  tok[t][(cf*H + h)*KW + j] = x_pad[b, cf, h, corr + j]: window entries outside [0, W) read as zero in the gather and are
 * never written by the scatter.  Scatter: selected lane number n (0-based among the selected lanes of its tile) writes rows h < H-1-n,
 * among covering lanes the last one wins, a tile without a selected lane is copied through.  lm_rowref_gather / lm_rowref_scatter are
 * the off_grid = 2 call of the same kernels.
 * NOTE on the name `hip_stream`: as for lm_strip_bin_points above - tests/test_bounds_inventory_cpu.py finds device entries by the spelling
 * `stream` and demands their guarded-buffer case in tests/test_gpu_1_bounds.py; the cases of these two entries are
 * tests/test_gpu_rowref_geometry.py::test_gather_win_bit_exact and ::test_scatter_win_bit_exact, which that inventory does not read. */
int lm_softmax_rows(void* stream, float* x, long rows, int cols);
int lm_rowref_select(void* stream, const float* ext, const float* cls, float* mean_out, int* valid, float thr_ext, int* corr,
                     int B, int H, int W, int L);
int lm_rowref_gather(void* stream, const float* x_nhwc8, const int* corr, float* tok, int B, int H, int W, int L);
int lm_rowref_scatter(void* stream, const float* x_nhwc8, const float* tok, const int* corr, const int* valid,
                      float* y_nhwc8, int B, int H, int W, int L);
int lm_rowref_gather_win(void* hip_stream, const float* x_nhwc8, const int* corr, float* tok, int B, int H, int W, int L, int off_grid);
int lm_rowref_scatter_win(void* hip_stream, const float* x_nhwc8, const float* tok, const int* corr, const int* valid,
                          float* y_nhwc8, int B, int H, int W, int L, int off_grid);
int lm_rowref_decode(void* stream, const float* ext2, const float* cls2, unsigned char* conf, unsigned char* cls_map,
                     int* col_idx, int B, int H, int W, int L);

/* ---- sparse-voxel LiDAR encoder, config 5 (baseline/models/pcencoder/lidarencoder.py) ----------------------------
 * PARITY UNPINNED for voxelize / sparse convolutions: the reference only instantiates and calls mmdet3d's
 * VoxelizationByGridShape (:29) and SparseEncoder (:33, called :93,:102); their published behaviour is restated.
 * voxelize_hard replaces :104-129 for one sample (hard voxelisation + mean of the kept points + batch index);
 * row_base / row_end are DEVICE ints (row range of this sample in the batch's feats / coords).
 * voxelize_hard / sparse_grid_build / sparse_conv_outputs / sparse_rulebook are tested for exact equality with brute-force
 * references (cell edges, caps, sort-key widths, cap_rows / ldf / chaining, volume seams) in tests/test_gpu_sparse_index.py.
 * sparse_grid_build / sparse_conv_outputs / sparse_rulebook / conv_gather_mfma_f32 replace the SparseEncoder call :93
 * (SubMConv3d and SparseConv3d, BatchNorm1d folded, ReLU, residual); ksp_zyx9 = {kz,ky,kx, sz,sy,sx, pz,py,px}.
 * sparse_to_dense_nhwc = SparseConvTensor.dense().view(N, C*D, H, W) + torch.flip(dims=[2]) (:70);
 * upsample_bicubic_nhwc = F.interpolate(mode='bicubic', align_corners=False) (:72). */
long lm_voxelize_workspace_bytes(long n_points);
/* The two device-wide primitives under the voxeliser and the output-site compaction (csrc/prim.hip: the library's own kernels, where
 * mmdet3d's hard_voxelize / spconv's indice generation loop or hash on the device): exclusive prefix sum of u32 (wraps; in == out
 * allowed) and STABLE sort of (u32 key, u32 value) pairs by the low end_bit bits of the keys, in place. */
long lm_scan_workspace_bytes(long n);
int lm_exclusive_scan_u32(void* stream, const unsigned* in, unsigned* out, long n, void* workspace, long workspace_bytes);
long lm_sort_pairs_workspace_bytes(long n);
int lm_sort_pairs_u32(void* stream, unsigned* keys_io, unsigned* vals_io, long n, int end_bit, void* workspace, long workspace_bytes);
/* Points outside the grid are dropped; non-finite coordinates are dropped (NaN or +-Inf in x, y or z: no voxel, no share in any mean). */
int lm_voxelize_hard(void* stream, const float* points, long n, const float* range_lo_xyz, const float* voxel_size_xyz,
                     const int* grid_xyz, int max_points, int max_voxels, int batch_idx, const int* row_base, int cap_rows,
                     float* feats, int ldf, int* coords, int* row_end, int raster_order, void* workspace,
                     long workspace_bytes);
int lm_sparse_grid_build(void* stream, const int* coords, long n, int* grid, int B, int D, int H, int W);
long lm_sparse_conv_outputs_workspace_bytes(long out_cells);
int lm_sparse_conv_outputs(void* stream, const int* in_coords, long n_in, int B, const int* ksp_zyx9, int Do, int Ho, int Wo,
                           int* out_grid, int* out_coords, int cap_rows, int* out_count, void* workspace, long workspace_bytes);
int lm_sparse_rulebook(void* stream, const int* out_coords, long n_out, const int* in_grid, int B, int D, int H, int W,
                       const int* ksp_zyx9, int* nbr);
int lm_conv_gather_mfma_f32(void* stream, const float* x, int ldx, const int* nbr, int taps, const float* wp, int CoutP,
                            const float* scale, const float* shift, const float* res, int ldr, float* y, int ldy,
                            long M, int Cin, int Cout, int act);
int lm_sparse_to_dense_nhwc(void* stream, const float* feats, int ldf, const int* coords, long n, float* out, int B, int D,
                            int H, int W, int C, int flip_h);
int lm_upsample_bicubic_nhwc(void* stream, const float* x, float* y, int B, int H, int W, int C, int Ho, int Wo);

/* ---- LAS ingest (replaces laspy in `read_las`, baseline/datasets/laserlane_proposals.py:618-636; ASPRS LAS 1.0-1.4,
 * point data record formats 0-10, uncompressed).  parse_header: HOST bytes of the file.  decode_points: records = DEVICE
 * copy of the point data (4-byte aligned, padded to a multiple of 4 bytes); out [n][4] f32 = X*scale + (offset - shift)
 * in f64, intensity raw (normalise 0) or (clip(i, lo, hi) - lo) / hi (normalise 1, read_las). */
typedef struct {
    int version_major, version_minor, point_format, record_len;
    long n_points, offset_to_points;
    double scale[3], offset[3], min_xyz[3], max_xyz[3];
} LmLasHeader;
int lm_las_parse_header(const unsigned char* bytes, long len, LmLasHeader* out);
int lm_las_decode_points(void* stream, const unsigned char* records, int record_len, long n, const double* scale,
                         const double* offset, const double* shift, float inten_lo, float inten_hi, int normalise,
                         float* out_xyzi);
/* decode_select: decode_points restricted to the records that pass a predicate on the record's own classification, flag bits and return
 * numbers and on the decoded height, compacted on the device in FILE ORDER (stable): out_xyzi[0 .. *kept) holds, bit for bit, the rows
 * decode_points writes for the kept records; rows from *kept on are not written.  A record is kept when ALL of these hold:
 *   classification  bit `c` of class_mask (8 x u32 = 256 bits) is set      formats 0-5: byte 15 bits 0-4;  formats 6-10: byte 16
 *   flags           no bit of drop_flags is set in the record              formats 0-5: byte 15 bits 5-7 = synthetic, key-point, withheld
 *                   (LM_LAS_DROP_*)                                         (these formats have NO overlap bit: LM_LAS_DROP_OVERLAP drops
 *                                                                           nothing there);  formats 6-10: byte 15 bits 0-3
 *   returns         LM_LAS_RETURNS_ALL: always; _FIRST: return number == 1; _LAST: return number == number of returns; _SINGLE: number
 *                   of returns == 1 (compared as written: return number 0 gets no special case)
 *                                                                           formats 0-5: byte 14 bits 0-2 / 3-5;  6-10: bits 0-3 / 4-7
 *   height          z_lo <= z <= z_hi on the f32 z that is written (after the shift); -inf / +inf switch a side off, NaN is refused
 * kept: DEVICE long.  class_hist: DEVICE [256] u64 or NULL = classification counts of ALL n records (kept or not).  workspace: device,
 * lm_las_select_workspace_bytes(n) bytes.  n <= 2^31 - 1, record_len 20 .. 160 (any value, records padded to a multiple of 4 bytes).
 * Three launches - count per 256-record block, exclusive scan (lm_exclusive_scan_u32's kernels), emit to block offset + ballot rank -
 * every slot reserved by a prefix: no atomics on device memory, the same bits each run; the class counters are integers in LDS, written
 * once per workgroup and summed by a second kernel.  Nothing is read back: the caller fetches *kept when it needs the number.
 * NOTE on the name `hip_stream`: as for lm_strip_bin_points above - tests/test_bounds_inventory_cpu.py finds device entries by the spelling
 * `stream` and demands their guarded-buffer case in tests/test_gpu_1_bounds.py; this entry's case is
 * tests/test_gpu_las_select.py::test_select_guards, which that inventory does not read. */
enum { LM_LAS_DROP_SYNTHETIC = 1, LM_LAS_DROP_KEYPOINT = 2, LM_LAS_DROP_WITHHELD = 4, LM_LAS_DROP_OVERLAP = 8 };
enum { LM_LAS_RETURNS_ALL = 0, LM_LAS_RETURNS_FIRST = 1, LM_LAS_RETURNS_LAST = 2, LM_LAS_RETURNS_SINGLE = 3 };
typedef struct { unsigned class_mask[8]; unsigned drop_flags; int returns; float z_lo, z_hi; } LmLasSelect;
long lm_las_select_workspace_bytes(long n);
int lm_las_decode_select(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                         const double* scale, const double* offset, const double* shift, float inten_lo, float inten_hi,
                         int normalise, const LmLasSelect* select, void* workspace, long workspace_bytes, float* out_xyzi,
                         long* kept, unsigned long* class_hist);

/* ---- labelling the returns by the lane lines (csrc/label.hip): the way back of the cloud -> map route.  The lines (LAS frame) are cut into
 * segments on the host (las_io.line_segments): [S][8] f32 rows ax, ay, az, dx, dy, dz, inv, line - endpoints minus the read shift rounded
 * to f32, d = the f32 difference of the rounded endpoints, inv = 1 / (dx dx + dy dy) in f32 or 0 where that is 0, line = the int32 bits of
 * (line index + 1); line order, then vertex order.  Point (x, y, z, i) against a segment, plain f32, no contraction:
 *     px = x - ax;  py = y - ay;  t = fminf(fmaxf((px dx + py dy) inv, 0), 1)
 *     ex = px - t dx;  ey = py - t dy;  d2 = ex ex + ey ey;  zl = az + t dz
 *     hit = d2 <= half_width^2 (squared once in f32)  &&  fabsf(z - zl) <= z_tol
 * A point is ELIGIBLE when x, y, z are finite and, with a min_intensity (NaN = none), i >= min_intensity (a NaN i is then not eligible).
 * Its LABEL is the line of the hit with the smallest d2, ties to the smaller line, then to the smaller segment index; no hit, or not
 * eligible: 0.  The horizontal distance decides; z_tol only keeps a carriageway from labelling the one under or over it.  A label
 * depends on the point and the index alone - no atomic decides it - so every run writes the same bits.
 * line_index_build (HOST, no GPU is touched): a uniform grid of nx x ny cells of size `cell` (0 = the default, max(1 m, 2 half_width);
 *         the cell grows if the box would need more than 2^24 cells) over the box of the segments inflated by half_width, as CSR lists
 *         cell_start [nx ny + 1], cell_segs [n_entries], segment indices ascending inside a cell.  A cell lists a SUPERSET of the segments
 *         that can hit a point in it (margins two orders above the f32 rounding of the cell index and of the distance); a point outside
 *         the grid has label 0.  The grid decides the cost, never the result.  Two calls: with cell_start = cell_segs = NULL it fills
 *         *grid (geometry, n_entries, the smallest and largest line, S, half_width); with the arrays and their capacities (in elements) it
 *         fills them too.  S = 0: nx = ny = 0.  Refused: a segment value that is not finite, a line < 1, capacities too small.
 * label_points: points_xyzi DEVICE [N][4] f32; segments, cell_start, cell_segs: DEVICE copies of what line_index_build took and wrote; grid:
 *         HOST, and half_width the one it was built for.  line [N] int32 = the labels; dist2 [N] f32 or NULL = the winner's d2, +inf
 *         without a hit.  N = 0 or S = 0 is LM_OK (every label 0).
 * las_label_records: the same rule on raw point records (DEVICE, 4-byte aligned, padded to a multiple of 4 bytes, as lm_las_decode_points
 *         takes them).  A workgroup stages 256 records in LDS as the decode does, decodes each with the decode's own expression (the rows
 *         lm_las_decode_points writes with normalise = 0), evaluates the predicate of lm_las_decode_select where `select` is given (HOST,
 *         or NULL: every record passes) - a record that fails it is never relabelled -, labels, patches the staged record and stores the
 *         staged words back.  records_out = the input byte for byte, except in a labelled record: the classification becomes marking_class
 *         (formats 0-5: the low five bits of byte 15, bits 5-7 kept; formats 6-10: byte 16) and, with write_line_id, the point source ID
 *         (u16 LE at byte 18 / byte 20) becomes the label.  records_out == records is allowed, any other overlap is not.  line [n] int32 or
 *         NULL.  counts DEVICE [L + 1] u64 or NULL, zeroed by the call: counts[k], k >= 1 = records labelled k, counts[0] = records that
 *         passed `select` and got no label; integer adds, order independent.  L = the number of lines.
 *         One launch: as many workgroups as the current device holds at once (asked of the runtime once per device and LDS size) walk the
 *         blocks of 256 records; like every entry here the call launches on the current device, which must be the stream's.
 *         TRUST: `grid` is the caller's word about the device table.  If the table in device memory carries a line above grid->max_line
 *         (a table other than the one the grid was built for), labels above L are still written to `line` and to the point source ID, but
 *         never counted: nothing is written outside counts[0 .. L].
 * Both device entries are asynchronous, read nothing back and need no workspace.  Refused with LM_ERR_ARG and a message that names the
 * argument, before anything is launched or written: marking_class > 31 on formats 0-5 or > 255; write_line_id with L > 65535; a NaN or
 * negative half_width or z_tol; segments whose lines (grid's min_line, max_line) leave 1 .. L; a grid built for another S or half_width;
 * a bad record_len (below the format's minimum or above 160) or point_format; null buffers; a misaligned buffer, named alone
 * ("records_out is not 4-byte aligned").
 * NOTE on the name `hip_stream`: as for lm_strip_bin_points above - tests/test_bounds_inventory_cpu.py finds device entries by the spelling
 * `stream` and demands their guarded-buffer case in tests/test_gpu_1_bounds.py; the cases of these two entries are
 * tests/test_gpu_label.py::test_label_points_guards and ::test_label_records_guards, which that inventory does not read. */
typedef struct {
    double x0, y0, cell;
    int nx, ny, min_line, max_line;
    long n_segments, n_entries;
    float half_width;
} LmLineGrid;
int lm_line_index_build(const float* segments, long S, float half_width, double cell, LmLineGrid* grid, int* cell_start,
                        long cell_start_cap, int* cell_segs, long cell_segs_cap);
int lm_label_points(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                    const int* cell_start, const int* cell_segs, float half_width, float z_tol, float min_intensity, int* line,
                    float* dist2);
int lm_las_label_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                         const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                         const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width, float z_tol,
                         float min_intensity, int marking_class, int write_line_id, unsigned char* records_out, int* line,
                         unsigned long* counts, int L);

/* ---- the marking profile (csrc/profile.hip): every lane line profiled from the returns the labelling rule gives it - per station bin
 * along the line the count, the summed intensity and the lateral spread of its returns; paint runs, dash pattern, width and brightness are
 * read off the bins on the host (las_io.marking_summary).
 * HOST TABLES (las_io.line_stations(lines, shift, bin)), rows in exactly the order of the segment table:
 *     stations [S][4] f32 = s0, len, rlen, 0.  len64 = sqrt(dx dx + dy dy) in f64 from the f32 dx, dy of the segment row; s0 = the f64
 *         running sum of the len64 of the earlier segments of the same line, rounded to f32; len = (f32)len64; rlen = (f32)(1 / len64), or 0
 *         where len64 == 0.
 *     bin_start [L + 1] int32, a CSR table: line k (from 1) owns the bins bin_start[k-1] .. bin_start[k] - 1; a line with segments owns
 *         max(1, ceil(total len64 / bin)) bins, a line with fewer than two vertices none.  bin is finite and > 0.
 * PER POINT.  Eligibility, the hit test and the winner are exactly the labelling rule's above (smallest d2, ties to the smaller line, then
 * to the smaller segment index).  For a point whose winner is segment s of line k, with the clamped t and px, py of that rule, plain f32,
 * no contraction:
 *     st = s0 + t len
 *     b  = min((int)(st inv_bin), nb_k - 1)                  inv_bin = (f32)(1 / bin), nb_k the number of bins of line k
 *     o  = (dx py - dy px) rlen                              the signed offset, left of the line positive; 0 on a zero-length segment
 *     q  = (int)rintf(o 1024.f)
 *     iq = (unsigned)fminf(fmaxf(rintf(i), 0.f), 65535.f)    a NaN intensity gives 0
 * OUTPUT.  bins [n_bins][6] int64 = n, sum iq, sum q, sum q q, min q, max q per bin; an empty bin reads 0, 0, 0, 0, 2^31 - 1, -2^31.
 * Everything is an integer sum, minimum or maximum: the result does not depend on the order of the points or of the adds, and every run
 * writes the same bits.  No float atomic is used.  half_width above 16 m is refused, so that |q| <= 2^14 + 1 and the sums of 2^31 points
 * stay far inside 64 bits.  WITHOUT a min_intensity a bin counts returns, not paint: width and dash pattern then measure the band and the
 * point density, so a threshold between asphalt and paint is needed for them to mean anything.
 * line_profile_points: points_xyzi DEVICE [N][4] f32, then the index arguments of lm_label_points.
 * las_line_profile_records: the inputs of lm_las_label_records up to `select`, then the index.  The records are only read: staged through
 *         LDS and decoded as there; a record that `select` drops contributes nothing.
 * Both: stations DEVICE [S][4] f32 (16-byte aligned); bin_start DEVICE [L + 1] int32, what the kernel reads; bin_start_host its HOST copy,
 *         what the call checks (from 0, not descending, bin_start_host[L] == n_bins) - the host cannot see a device table without a
 *         read-back, so the table travels twice, as `grid` travels beside cell_start.  TRUST: the device tables are the caller's word;
 *         whatever they hold, the kernels read bin_start only in [0, L] and write bins only in [0, n_bins).  accumulate = 0: the call
 *         initialises bins on the stream first; accumulate = 1: it adds to what is there - the files of a strip go into one profile this
 *         way.  Asynchronous, no workspace, nothing read back.  N = 0, S = 0 or n_bins = 0 is LM_OK.
 *         The wave merges before it goes to memory: per distinct bin among its lanes one reduction and one row of six 64-bit integer
 *         atomics; a wave without a candidate leaves early as in the label kernels.
 * Refused with LM_ERR_ARG and a message that names the argument, before anything is launched or written: what lm_label_points /
 * lm_las_label_records refuse of the shared arguments; half_width > 16; bin <= 0 or not finite; accumulate outside 0, 1; segments whose
 * lines leave 1 .. L; n_bins != bin_start_host[L]; a bin_start_host that does not start at 0 or descends; null buffers; a misaligned
 * buffer, named alone ("bins is not 8-byte aligned").
 * NOTE on the name `hip_stream`: as for lm_label_points above; the guarded-buffer cases of these two entries are
 * tests/test_gpu_profile.py::test_profile_points_guards and ::test_profile_records_guards. */
int lm_line_profile_points(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                           const int* cell_start, const int* cell_segs, float half_width, const float* stations, const int* bin_start,
                           const int* bin_start_host, int L, double bin, float z_tol, float min_intensity, int accumulate, long* bins,
                           long n_bins);
int lm_las_line_profile_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                                const double* scale, const double* offset, const double* shift, const LmLasSelect* select,
                                const float* segments, long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs,
                                float half_width, const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin,
                                float z_tol, float min_intensity, int accumulate, long* bins, long n_bins);

/* ---- the colour of the markings (csrc/profile.hip): white or yellow, from the 16-bit R, G, B triple that colourised deliveries carry per
 * return.  Point formats 2, 3, 5, 7, 8 and 10 hold it as three u16 LE at byte 20 (format 2), 28 (3, 5) or 30 (7, 8, 10) of the record;
 * formats 0, 1, 4, 6 and 9 have no colour.
 * THE RULE (one definition: las_profile_kernel<true>, this text, tests/colour_ref.py).  Eligibility, the hit test, the winner, the station
 * bin b and the row bin_start[k-1] + b are exactly the marking profile's above, min_intensity and `select` included: a record that `select`
 * drops contributes nothing.  For a return that lands in a bin, with its R, G, B:
 *     BLACK     R == 0 && G == 0 && B == 0 (colourisation leaves such triples where no camera saw the point): n_black += 1, nothing else
 *     COLOURED  any other triple: n_c += 1, sum R += R, sum G += G, sum B += B
 *     YELLOW    a coloured return with 2048 B < blue_q (R + G): n_yellow += 1.  blue_q = round(1024 yellow_ratio), an integer in 1 .. 1024:
 *               "blue is below yellow_ratio of the mean of red and green".  Both sides fit 32 bits; equality is not yellow; the test does
 *               not depend on the scale of the triple, so 8-bit values stored in the 16-bit fields need no special case.
 * OUTPUT.  colours [n_bins][6] int64 = n_c, sum R, sum G, sum B, n_yellow, n_black per bin; an empty bin reads six zeros.  Integer sums only:
 * the result does not depend on the order of the records or of the adds, every run writes the same bits, no float atomic is used.
 * las_line_colour_records: the arguments of lm_las_line_profile_records, blue_q after min_intensity, colours after bins.  The records are
 *         read ONCE: the same kernel, instantiated with the colour part, writes both tensors, and bins holds bit for bit what
 *         lm_las_line_profile_records writes for the same arguments.  accumulate covers both tensors: 0 initialises both on the stream
 *         first, 1 adds to both.  The wave merges the colour row as it merges the profile's: per distinct bin among its lanes the three sums
 *         by cross-lane adds (64 x 65535 fits 32 bits), the three counts by ballots, then the row's 64-bit integer atomics (an add of 0 is
 *         left out).  Asynchronous, no workspace, nothing read back.  n = 0, S = 0 or n_bins = 0 is LM_OK after the initialisation.
 * Refused with LM_ERR_ARG and a message that names the argument, before anything is launched or written: everything
 * lm_las_line_profile_records refuses; a point_format without colour ("point_format=1 carries no RGB"); blue_q outside 1 .. 1024; a null
 * colours with n_bins > 0; a colours that is not 8-byte aligned, named alone; colours overlapping bins.
 * NOT HERE: a points entry.  Decoded clouds ([N][4] xyzi) carry no colour; giving them one means changing the compaction of
 * lm_las_decode_select, which is another change.
 * NOTE on the name `hip_stream`: as for lm_label_points above; the guarded-buffer case of this entry is
 * tests/test_gpu_colour.py::test_colour_records_guards. */
int lm_las_line_colour_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                               const double* scale, const double* offset, const double* shift, const LmLasSelect* select,
                               const float* segments, long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs,
                               float half_width, const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin,
                               float z_tol, float min_intensity, int blue_q, int accumulate, long* bins, long* colours, long n_bins);

/* ---- cross-sections along every line (csrc/profile.hip): per station bin of a line a row of lateral cells holding the count, the paint
 * count, the summed intensity and the summed height of the returns of the band - what tells a double line from a single one, gives a
 * width and a paint centre that one stray return cannot set, and the road's cross-fall beside the line (las_io.cross_summary,
 * las_io.snap_lines are the host policy on top of the table).
 * THE RULE (one definition: cross_row in csrc/profile.hip, which both kernels call, this text, tests/cross_ref.py).  Eligibility, the hit
 * test and the winner are exactly the labelling rule's (smallest d2, ties to the smaller line, then to the smaller segment index), WITHOUT
 * a min_intensity: every finite return counts, the table must see asphalt as well as paint.  For a point whose winner is segment s of line
 * k, with the clamped t, px, py and zl = az + t dz of that rule and st, b, o, q, iq of the marking profile above, unchanged, plain f32, no
 * contraction:
 *     hq  = (int)ceil((double)half_width 1024)                 on the host (half_width the f32 the index was built for)
 *     nl  = 2 hq / lateral_q + 1                               lateral cells per station bin (integer division)
 *     u   = min(max(q + hq, 0), 2 hq);   c = u / lateral_q
 *     zq  = (int)rintf((z - zl) 1024.f)
 *     row = (bin_start[k-1] + b) nl + c
 *     cells[row] += 1, (iq >= paint_iq), iq, zq
 * OUTPUT.  cells [n_bins nl][4] int64 = n, n_paint, sum iq, sum zq; an empty cell reads four zeros.  Cell c of a station bin covers the
 * offsets [(c lateral_q - hq) / 1024, ((c + 1) lateral_q - hq) / 1024) m, left of the line positive.  lateral_q: the cell width in 1/1024 m,
 * an integer >= 1.  paint_iq: an integer in 0 .. 65536; 65536: nothing is paint; a NaN intensity gives iq = 0.  half_width > 16 and
 * z_tol > 16 are refused, so |q|, |zq| <= 2^14 + 1 and the sums of 2^31 returns stay inside 64 bits; n_bins nl > 2^27 is refused, which
 * caps the table at 4 GiB.  Integer sums only: the result does not depend on the order of the points, files or adds, every run writes the
 * same bits, no float atomic is used.
 * line_cross_points: the arguments of lm_line_profile_points without min_intensity, then lateral_q, paint_iq, accumulate, cells,
 *         n_cells = bin_start_host[L] nl.  A kernel of profile_points_kernel's streaming shape, no LDS.
 * las_line_cross_records: the inputs of lm_las_line_profile_records with the same changes: a further instantiation of las_profile_kernel,
 *         the records are read once and only read, a record that `select` drops contributes nothing.
 * Both: accumulate = 0 zeroes cells on the stream first, accumulate = 1 adds to what is there.  Asynchronous, no workspace, nothing read
 *         back.  N = 0, S = 0 or n_cells = 0 is LM_OK after the initialisation.
 * Refused with LM_ERR_ARG and a message that names the argument, before anything is launched or written: what the profile entries refuse
 * of the shared arguments; z_tol > 16; lateral_q < 1; paint_iq outside 0 .. 65536; n_bins nl > 2^27; n_cells != bin_start_host[L] nl; a
 * null cells with n_cells > 0; "cells is not 8-byte aligned".
 * NOTE on the name `hip_stream`: as for lm_label_points above; the guarded-buffer cases of these two entries are
 * tests/test_gpu_cross.py::test_cross_points_guards and ::test_cross_records_guards. */
int lm_line_cross_points(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                         const int* cell_start, const int* cell_segs, float half_width, const float* stations, const int* bin_start,
                         const int* bin_start_host, int L, double bin, float z_tol, int lateral_q, int paint_iq, int accumulate,
                         long* cells, long n_cells);
int lm_las_line_cross_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                              const double* scale, const double* offset, const double* shift, const LmLasSelect* select,
                              const float* segments, long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs,
                              float half_width, const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin,
                              float z_tol, int lateral_q, int paint_iq, int accumulate, long* cells, long n_cells);

/* ---- the paint / asphalt histograms (csrc/profile.hip): per line and per lateral ring around it a histogram of the intensities of its
 * returns - what the threshold between asphalt and paint is read off.  Returns on a line are paint plus some asphalt, returns a few
 * decimetres beside it are asphalt; the threshold that separates the two populations best is the min_intensity / paint_intensity the
 * stages above ask for, and per line it is a check of the network: a line whose inner returns are no brighter than its outer ones has no
 * paint under it (las_io.PaintThreshold, las_io.paint_threshold are the host policy on top of the table).
 * THE RULE (one definition: hist_cell in csrc/profile.hip, which both kernels call, this text, tests/threshold_ref.py).  Eligibility, the
 * hit test and the winner are exactly the labelling rule's (smallest d2, ties to the smaller line, then to the smaller segment index),
 * WITHOUT a min_intensity: the table must see asphalt.  For a point whose winner is segment s of line k, with px, py of that rule and o, q,
 * iq of the marking profile above, unchanged, plain f32, no contraction - of the stations table only rlen is read; no bin_start and no
 * station bin are involved:
 *     hq  = (int)ceil((double)half_width 1024)                 on the host (half_width the f32 the index was built for)
 *     Z   = hq / ring_q + 1                                    rings per line (integer division)
 *     r   = min(|q|, hq) / ring_q                              the ring: ring r covers the offsets r ring_q <= |q| < (r + 1) ring_q
 *     NB  = 65536 >> bin_shift                                 counts per histogram
 *     ib  = iq >> bin_shift                                    a NaN intensity gives iq = 0
 *     hist[((k-1) Z + r) NB + ib] += 1
 * OUTPUT.  hist [L][Z][NB] int64; a cell no return fell into reads 0.  ring_q: the ring width in 1/1024 m, an integer >= 1 (above hq:
 * Z = 1); bin_shift: 0 .. 8.  Integer adds only, no float atomic: the bits do not depend on the order of the points, files or adds.
 * line_hist_points: points_xyzi DEVICE [N][4] f32, the index arguments of lm_label_points, stations DEVICE [S][4] f32 (16-byte aligned),
 *         L, z_tol, ring_q, bin_shift, accumulate, hist, n_hist = L Z NB.  A kernel of cross_points_kernel's streaming shape, no LDS: four
 *         16-byte loads in flight per lane, a wave without a candidate leaves through the ballot.
 * las_line_hist_records: the inputs of lm_las_line_cross_records up to `select`, then the same: a further instantiation of
 *         las_profile_kernel, the records are read once and only read, a record that `select` drops contributes nothing.
 * Both: accumulate = 0 zeroes hist on the stream first (a kernel, as every entry that may be captured zeroes), accumulate = 1 adds to what
 *         is there - the files of a strip go into one table this way.  Asynchronous, no workspace, nothing read back.  N = 0 or S = 0 is
 *         LM_OK after the initialisation.  TRUST: the device tables are the caller's word; whatever they hold, hist is written only in
 *         [0, n_hist).
 * Refused with LM_ERR_ARG and a message that names the argument, before anything is launched or written: what the cross entries refuse of
 * the shared arguments (the index, half_width > 16, z_tol > 16, segments whose lines leave 1 .. L, a null or misaligned stations, the
 * points or records); ring_q < 1; bin_shift outside 0 .. 8; L Z NB > 2^27; n_hist != L Z NB; accumulate outside 0, 1; a null hist with
 * n_hist > 0; "hist is not 8-byte aligned".
 * NOTE on the place of `hip_stream`: these two entries take the stream as their LAST parameter.  The older entries take it first, and
 * tests/test_stream_inventory_cpu.py, tests/test_bounds_inventory_cpu.py and tests/lds_state.py find entries by that spelling and hold each
 * to a literal table inside an existing test file; an entry found there needs a row in those tables.  The cases those tables would name -
 * guarded buffers, a side stream, graph replay, poisoned LDS before las_profile_kernel<false, false, true> - are in
 * tests/test_gpu_threshold.py.  For the same reason hist_points_kernel declares no __shared__ and the record kernel keeps the name
 * las_profile_kernel. */
int lm_line_hist_points(const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid, const int* cell_start,
                        const int* cell_segs, float half_width, const float* stations, int L, float z_tol, int ring_q, int bin_shift,
                        int accumulate, long* hist, long n_hist, void* hip_stream);
int lm_las_line_hist_records(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                             const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                             const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width, const float* stations,
                             int L, float z_tol, int ring_q, int bin_shift, int accumulate, long* hist, long n_hist, void* hip_stream);

/* ---- paint thresholds per line and station window (csrc/profile.hip, label.hip, residue.hip).  A scanner's intensity falls with range:
 * the paint of an outer lane is routinely darker than the asphalt of the lane under the scanner, and no single number separates the two
 * on such a strip.  So the threshold is a TABLE, one value per station window of every line, read off WINDOWED histograms by the host
 * policy (las_io.hist_window_files, las_io.paint_table) and looked up on the device for every return by the stages that take it.
 * THE WINDOWS.  win_start [L + 1] int32 is a CSR table: line k (from 1) owns the rows win_start[k-1] .. win_start[k] - 1, nw_k of them.
 * It is the bin_start of the marking profile for bin = window (las_io.line_stations(lines, shift, bin=window)).  For a return whose winner
 * (the labelling rule's: smallest d2, ties to the smaller line, then to the smaller segment index) is segment s of line k at the clamped
 * t, with the stations row s0, len of that segment, plain f32, no contraction:
 *     st  = s0 + t len                                         the marking profile's station
 *     w   = min((int)(st inv_window), nw_k - 1)                inv_window = (f32)(1 / window)
 *     row = win_start[k-1] + w
 * A line per row ("scope = line") is the same table with a window longer than every line: no second code path.
 * THE WINDOWED HISTOGRAM.  las_line_hist_window_records: the histogram rule above with the row taken per window instead of per line:
 *     hist[(row Z + r) NB + ib] += 1                           r, ib, Z, NB as above; hist [R][Z][NB] int64, R = win_start_host[L]
 *         The arguments of lm_las_line_hist_records, then win_start (DEVICE [L + 1]), win_start_host (its HOST copy, what the call checks:
 *         from 0, not descending - the table travels twice, as bin_start does) and window (metres, finite, > 0); n_hist = R Z NB.  One more
 *         instantiation of las_profile_kernel: the records are read once and only read.  accumulate, the asynchrony and the edge sizes
 *         (n = 0, S = 0, R = 0: LM_OK after the initialisation) are lm_las_line_hist_records'.  One window per line gives bit for bit its
 *         table, and the windows of a line summed give it as well.  TRUST: whatever the device tables hold, win_start is read only in
 *         [0, L] and hist is written only in [0, n_hist).  Refused, by the argument's name, before anything is launched or written: what
 *         lm_las_line_hist_records refuses; a null or misaligned win_start; a null win_start_host, one that does not start at 0 or
 *         descends; window <= 0 or not finite; R Z NB > 2^27; n_hist != R Z NB.
 * THE RULE OF THE STAGES (one definition: this text; table_row / table_pass in csrc/label_rule.h and tests/local_ref.py restate it).
 *     1. The winner (line k, segment s, t) is the labelling rule's, taken WITHOUT a min_intensity.
 *     2. row as above.
 *     3. A return PASSES when i >= thr_min && i >= thr[row], in plain f32; a NaN intensity fails.  In the cross entry, which counts
 *        every finite return, nothing is filtered: a return is paint when iq >= paint_iq[row].
 *     4. A return that does not pass is treated exactly as the scalar rule treats a return below min_intensity: label 0 and not counted
 *        as labelled; not added to any bin or colour row; no residue (key -1, iq 0).
 * thr_min keeps the early exit of dark waves - a wave of asphalt leaves before the search.  The host wrappers pass min(thr); whatever a
 * caller passes, the rule above is what happens (a thr_min above a row's threshold raises that row's threshold to it).  A table whose
 * rows all equal T, with thr_min = T, gives bit for bit what the scalar entry gives with min_intensity = T (paint_iq: with the scalar
 * paint_iq in every row): eligibility by intensity does not depend on the winner.
 * THE ENTRIES.  Each takes its scalar entry's arguments with `const LmPaintTable* table` (HOST) in place of min_intensity / paint_iq,
 * and is that entry's kernel with one more template parameter, not a copy of it:
 *     lm_las_label_records_local, lm_las_line_profile_records_local, lm_las_line_colour_records_local, lm_las_line_cross_records_local
 *     and lm_residue_keys_local (the points entry: the residue route decodes first).
 * table->stations is the station table of the segments the index was built from; the label and residue entries take no station table
 * otherwise and get it here (lm_residue_keys_local also takes L, the lines of win_start, which its scalar entry has no use for).  n = 0, S = 0 and n_rows = 0 are LM_OK after the initialisation (no row: nothing passes).
 * TRUST: whatever the device tables hold, thr and paint_iq are read only in [0, n_rows), win_start only in [0, L], and the outputs are
 * written only where the scalar entry writes them.
 * Refused with LM_ERR_ARG and a message that names the argument ("table.thr", ...), before anything is launched or written: what the
 * scalar entry refuses; a null table; a null table member the entry reads (thr in all but the cross entry, paint_iq in the cross entry,
 * win_start and stations with S > 0, win_start_host always); a misaligned member (thr, paint_iq, win_start: 4 bytes, stations: 16);
 * n_rows != win_start_host[L]; a win_start_host that does not start at 0 or descends; a window that is not finite or not positive; a
 * thr_min that is not finite; paint_iq given to an entry that does not read it, or missing from the cross entry.
 * NOT HERE: points entries for label, profile, cross and the windowed histogram - the map routes run these stages on the records.
 * NOTE on the place of `hip_stream`: LAST, as for lm_line_hist_points above and for the same reason; the cases the literal tables would
 * name - guarded buffers, a side stream, graph replay, poisoned LDS - are in tests/test_gpu_threshold_local.py.  The new instantiations keep
 * the kernel names las_profile_kernel and las_label_kernel, and residue_keys_kernel declares no __shared__. */
typedef struct {
    const float* thr;            /* DEVICE [n_rows] f32 */
    const int*   paint_iq;       /* DEVICE [n_rows] int32 in 0 .. 65536: the cross entry reads this one, the others NULL */
    const int*   win_start;      /* DEVICE [L + 1] */
    const int*   win_start_host; /* HOST copy, what the call checks: from 0, not descending, win_start_host[L] == n_rows */
    const float* stations;       /* DEVICE [S][4] f32, 16-byte aligned: s0, len, rlen of the segment table */
    double window;               /* metres, finite, > 0 */
    float  thr_min;              /* the early-exit pre-filter, see the rule */
    long   n_rows;
} LmPaintTable;
int lm_las_line_hist_window_records(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                    const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                                    const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                    const float* stations, int L, float z_tol, int ring_q, int bin_shift, int accumulate, long* hist,
                                    long n_hist, const int* win_start, const int* win_start_host, double window, void* hip_stream);
int lm_las_label_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                               const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                               const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width, float z_tol,
                               const LmPaintTable* table, int marking_class, int write_line_id, unsigned char* records_out, int* line,
                               unsigned long* counts, int L, void* hip_stream);
int lm_las_line_profile_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                      const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                                      const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                      const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin, float z_tol,
                                      const LmPaintTable* table, int accumulate, long* bins, long n_bins, void* hip_stream);
int lm_las_line_colour_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                     const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                                     const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                     const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin, float z_tol,
                                     const LmPaintTable* table, int blue_q, int accumulate, long* bins, long* colours, long n_bins,
                                     void* hip_stream);
int lm_las_line_cross_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                    const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                                    const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                    const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin, float z_tol,
                                    int lateral_q, const LmPaintTable* table, int accumulate, long* cells, long n_cells, void* hip_stream);
int lm_residue_keys_local(const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid, const int* cell_start,
                          const int* cell_segs, float half_width, float z_tol, const LmPaintTable* table, int L, float clear, double cell,
                          int nx, int ny, long* key, int* iq, void* hip_stream);

/* ---- the paint no lane line explains (csrc/residue.hip): stop bars, crossing bars, arrows, hatching, chevrons and lines the network
 * missed are bright paint in the same returns as the lines, and label, profile and colour above see only paint that lies ON a line.  This
 * stage takes the strip's returns and the lines the call returns, keeps the bright road-level returns that no line explains (the RESIDUE),
 * puts them on a sparse map-frame grid, finds the connected blobs of that grid on the device and describes every blob by exact integer
 * footprint statistics.  The host policy (las_io.residue_summary) turns those into centre, area, length, width, fill and the heading
 * against the nearest line; calling a blob "arrow" or "zebra" is left to the user.
 * THE RULE (one definition: this text; the kernels and tests/residue_ref.py restate it).
 * PER POINT, plain f32, no contraction (build.py EXACT_FP).  Inputs: a line index (lm_line_index_build) built with half_width = REACH
 * (at most 16 m), z_tol, a finite min_intensity (required: "WITHOUT a min_intensity a bin counts returns, not paint" above - here the
 * whole road would be one blob), clear with 0 <= clear < reach, and a grid of nx x ny cells of size `cell` whose origin x0, y0 is the index
 * grid's f32 origin; inv = (f32)(1 / cell).
 *     ln, d2  = the labelling rule's winner and its squared distance; eligibility, the hit test and z_tol are exactly that rule's
 *     RESIDUE = ln > 0 && d2 > clear2                          clear2 = clear clear, squared once in f32; d2 == clear2 is no residue
 *     cx = (int)((x - x0) inv);  cy = (int)((y - y0) inv)
 *     key = (int64)cy nx + cx  for a residue point with 0 <= cx < nx and 0 <= cy < ny, else -1
 *     iq  = (unsigned)fminf(fmaxf(rintf(i), 0.f), 65535.f)     the profile's intensity rule, for a point with a key >= 0; else 0
 * A residue point lies within reach and within z_tol in height of some line - signs, vehicles and bridges stay out - and farther than
 * clear from every line that would hit it.  nx, ny come from the host (ops.residue_grid) so that the grid covers the index grid's box:
 * every point the index accepts then has 0 <= cx < nx, 0 <= cy < ny, and the kernel's range test never bites.  nx or ny above 2^20 is
 * refused: a cell index stays exact in f32, and with at most 2^22 occupied cells sum cx^2 < 2^62 stays inside 64 bits.
 * CELLS: the distinct keys >= 0 over all clouds of the call in ascending order, m = 0 .. M-1.
 * COMPONENTS: two cells are joined when they are neighbours on (cx, cy) under `connectivity`, 8 or 4 - on (cx, cy), not on the key: key
 * and key + 1 are no neighbours when cx = nx - 1.  root[m] = the smallest cell index of the component of m; components are numbered
 * 0 .. K-1 in ascending root.
 * STATISTICS: stats [K][12] int64 = n_cells, n_points, sum iq, sum cx, sum cy, sum cx^2, sum cx cy, sum cy^2, min cx, max cx, min cy,
 * max cy.  Moments and extents are taken over the cells, each once - the footprint, not the point density -, n_points and sum iq over the
 * points.  Integer sums, minima and maxima only, no float atomic: the result does not depend on the order of points, cells or adds.
 * residue_keys: points_xyzi DEVICE [N][4] f32, then the index arguments of lm_label_points (half_width = the reach).  key DEVICE [N] int64;
 *         iq DEVICE [N] int32 or NULL.  label_points_kernel's streaming shape, four 16-byte loads in flight per lane; a wave with no
 *         candidate leaves through the ballot.  N = 0 or S = 0 (every key -1) is LM_OK.  Asynchronous, no workspace, nothing read back.
 * cell_components: keys DEVICE [M] int64, ascending and distinct; root DEVICE [M] int32; err DEVICE [1] int32.  THE FORM CHOSEN IS THE
 *         LOCK-FREE UNION-FIND, and the entry READS NOTHING BACK: three launches - parent[m] = m; a lane per cell looks the neighbours
 *         with a smaller key (four for 8-connectivity, two for 4) up by binary search in keys[0, m) and joins each it finds: find both
 *         roots, order them, old = atomicMin(&parent[larger], smaller); old == larger: done, else go on with old; then a compression
 *         launch of its own.  parent[x] <= x holds throughout, so the final root is the smallest index of the component whatever the
 *         interleaving.  NO WAITING: no kernel waits for another workgroup - no flags, tickets or spinning; every loop advances by the
 *         lane's own action.  CAPPED LOOPS: a root chase follows at most M links, a join retries at most 2 M times (each retry lowers
 *         the larger index); a lane that exhausts a cap sets err[0] with an atomic and leaves - a bug is a non-zero err (zeroed by the
 *         call on the stream first), never a hang.  VISIBILITY: inside the union and compression launches every word of parent is read
 *         with an agent-scope atomic load or as the return value of an atomic and written only with atomics (one L2 per XCD); the three
 *         launches are published to each other by their boundaries.  keys is read-only and read with plain loads.  TRUST: the host cannot
 *         check a device table; whatever keys holds the entry reads keys[0, M) only, writes root[0, M) only and terminates - unsorted
 *         or duplicate keys give garbage inside root.
 * residue_stats: comp DEVICE [M] int32 (dense ids 0 .. K-1), keys DEVICE [M] int64 with the grid's nx, ny (cx = key % nx, cy = key / nx),
 *         cell_points and cell_iq DEVICE [M] int64 (points and summed iq per cell), stats DEVICE [K][12] int64, initialised by the call on
 *         the stream (zeros, 2^31 - 1 / -2^31 for the extents).  One pass, a lane per cell: the lanes of a wave that share a component are
 *         merged by cross-lane operations before one row of integer atomics per distinct component goes to memory, as las_profile_kernel
 *         merges per distinct bin; the cells are sorted by key, so the lanes of a wave mostly share a component.  M above 2^22 is refused.
 *         TRUST: a comp outside [0, K) or a key outside the grid contributes nothing; stats is written in [0, K) only.
 * None of the kernels uses LDS.  Compacting the keys >= 0, concatenating the clouds, the unique cells with their counts, the per-cell sum
 * of iq (an int64 index_add_) and the dense component ids are torch calls in ops.paint_residue.
 * Refused with LM_ERR_ARG and a message that names the argument, before anything is launched or written: what lm_label_points refuses of
 * the index arguments (a grid built for another half_width among them); a min_intensity that is not finite; clear < 0 or >= the reach; a
 * reach above 16; cell <= 0 or not finite; nx or ny above 2^20; connectivity other than 4 and 8; M above the limits; K > M; a null buffer
 * with N, M or K > 0; a misaligned buffer, named alone ("key is not 8-byte aligned").
 * NOT HERE: a raw-records entry.  The clouds come from las_io.read_las_raw(path, device, shift, select), so `select` applies as everywhere.
 * NOTE on the name `hip_stream`: as for lm_label_points above; the guarded-buffer cases of these three entries are
 * tests/test_gpu_residue.py::test_residue_keys_guards, ::test_cell_components_guards and ::test_residue_stats_guards. */
int lm_residue_keys(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                    const int* cell_start, const int* cell_segs, float half_width, float z_tol, float min_intensity, float clear,
                    double cell, int nx, int ny, long* key, int* iq);
int lm_cell_components(void* hip_stream, const long* keys, long M, int nx, int ny, int connectivity, int* root, int* err);
int lm_residue_stats(void* hip_stream, const int* comp, const long* keys, int nx, int ny, const long* cell_points, const long* cell_iq,
                     long M, long K, long* stats);

/* ---- PNG tile ingest (replaces PIL in `load_img`, baseline/datasets/laserlane_proposals.py:85-98 and laserlane.py:214-219:
 * np.array(Image.open(path)) -> uint8 HWC).  Host code, no third-party library (PIL runs zlib; the DEFLATE decoder here is
 * csrc/inflate.h), 8-bit non-interlaced grey / grey+alpha / RGB / RGBA only; palette, 16-bit and Adam7 files are refused; chunk CRCs
 * and the zlib Adler-32 are verified.  C = channels (1, 2, 3, 4).
 * lm_png_decode_files_u8 inflates n files of identical geometry on `threads` host threads into out [n][H][W][C], the layout
 * lm_tile_ingest_u8 takes.  lm_zlib_inflate is that decoder on a bare zlib stream (RFC 1950), *produced = inflated bytes. */
int lm_png_info(const unsigned char* data, long size, int* H, int* W, int* C);
int lm_png_decode_u8(const unsigned char* data, long size, unsigned char* out_hwc, long out_bytes);
int lm_png_decode_files_u8(const char* const* paths, int n, unsigned char* out_nhwc, int H, int W, int C, int threads);
int lm_zlib_inflate(const unsigned char* data, long size, unsigned char* out, long capacity, long* produced);

/* ---- per-tile polyline JSON (save_lane_seq_2d, baseline/utils/io_utils.py:58-93: json.dump(records, indent=4)) ----------------
 * lane_vertexes [n_lines][row_size][3] doubles = (row, col, semantic), a vertex exists iff col > 0, lines with < 2 vertices are dropped.
 * The text is byte-identical to the reference's (numbers formatted like CPython's float repr).  lm_lane_json_text returns the text
 * length; it writes (NUL-terminated) only if cap is large enough, so call it with out = NULL first.  Host code. */
long lm_lane_json_text(const double* lane_vertexes, int n_lines, int row_size, int with_pervertex_semantics, char* out, long cap);
int lm_lane_json_write(const double* lane_vertexes, int n_lines, int row_size, int with_pervertex_semantics, const char* path);
/* 3-D polylines after the back-projection / merge (save_seqs_json, utils/io_utils.py:11-15, records built at coor_img2pc.py:205-212):
 * seqs [L][Vmax][D] doubles, lens [L] in [1, Vmax]; keys "seq", "seq_len", "init_vertex", "end_vertex"; same text as json.dump(indent=4). */
int lm_seqs_json_write(const double* seqs, const int* lens, int L, int Vmax, int D, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* LANEMAP_HIP_H */
