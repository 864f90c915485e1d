"""ctypes binding of liblanemap_hip.so — the C-ABI declared in include/lanemap_hip.h.

The library is the product: there is no CPU/ATen fallback.  If it is missing, import of any op
fails loudly with a build hint (run ``python -m lanemapping_amd.build``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('LANEMAP_HIP_LIB') or os.path.join(_HERE, 'liblanemap_hip.so')   # override: another build (tests/asan)

c_f32p = C.POINTER(C.c_float)
vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_long, C.c_float


class LmRasterParams(C.Structure):
    """Per-tile BEV<->LAS parameters (reference utils/io_utils.py:125-150)."""
    _fields_ = [('quat', C.c_float * 4), ('trans', C.c_float * 3), ('bev_img_offset', C.c_float * 2),
                ('img_reso', C.c_float * 2), ('local_min_ele', C.c_float), ('ele_reso', C.c_float),
                ('inten_lo', C.c_float), ('inten_hi', C.c_float)]


class LmLasHeader(C.Structure):
    """Fields of the LAS public header block the ingest needs (include/lanemap_hip.h)."""
    _fields_ = [('version_major', C.c_int), ('version_minor', C.c_int), ('point_format', C.c_int), ('record_len', C.c_int),
                ('n_points', C.c_long), ('offset_to_points', C.c_long), ('scale', C.c_double * 3), ('offset', C.c_double * 3),
                ('min_xyz', C.c_double * 3), ('max_xyz', C.c_double * 3)]


class LmStripGrid(C.Structure):
    """Point-to-tile lookup grid of the strip binning (include/lanemap_hip.h)."""
    _fields_ = [('x0', C.c_double), ('y0', C.c_double), ('cell', C.c_double), ('nx', C.c_int), ('ny', C.c_int)]


class LmLasSelect(C.Structure):
    """Point selection of lm_las_decode_select (include/lanemap_hip.h)."""
    _fields_ = [('class_mask', C.c_uint * 8), ('drop_flags', C.c_uint), ('returns', C.c_int), ('z_lo', C.c_float), ('z_hi', C.c_float)]


class LmLineGrid(C.Structure):
    """Point-to-segment lookup grid of the labelling (include/lanemap_hip.h)."""
    _fields_ = [('x0', C.c_double), ('y0', C.c_double), ('cell', C.c_double), ('nx', C.c_int), ('ny', C.c_int), ('min_line', C.c_int),
                ('max_line', C.c_int), ('n_segments', C.c_long), ('n_entries', C.c_long), ('half_width', C.c_float)]


class LmPaintTable(C.Structure):
    """A paint threshold per station window of every line, as the _local entries take it (include/lanemap_hip.h)."""
    _fields_ = [('thr', C.c_void_p), ('paint_iq', C.c_void_p), ('win_start', C.c_void_p), ('win_start_host', C.c_void_p),
                ('stations', C.c_void_p), ('window', C.c_double), ('thr_min', C.c_float), ('n_rows', C.c_long)]


# name -> (restype, argtypes); every entry must be declared in include/lanemap_hip.h
SIGNATURES = {
    'lm_abi_version': (i32, []),
    'lm_last_error': (C.c_char_p, []),
    'lm_device_count': (i32, []),
    'lm_conv2d_nhwc_mfma_f32': (i32, [vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, i32,
                                      i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32]),
    'lm_conv2d_nhwc_mfma_resup_f32': (i32, [vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, vp, i32,
                                            i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32]),
    'lm_winograd44_supported': (i32, [i32, i32, i32, i32]),
    'lm_winograd44_supported_ld': (i32, [i32, i32, i32, i32, i32]),
    'lm_winograd44_gn_chunks': (i32, [i32, i32, i32]),
    'lm_winograd44_tiles': (i64, [i32, i32, i32, i32]),
    'lm_winograd44_twin_workspace_bytes': (i64, [i32, i32, i32, i32, i32, i32]),
    'lm_conv3x3_winograd44_f32': (i32, [vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    'lm_conv3x3_winograd44_twin_f32': (i32, [vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i64]),
    'lm_wino44_split_fragments': (i32, [vp, vp, vp, i64]),
    'lm_conv3x3_winograd44_split_f32': (i32, [vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, f32]),
    'lm_conv3x3_winograd44_split_twin_f32': (i32, [vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i64, f32]),
    'lm_conv2d_nhwc_mfma_f32_gnstats': (i32, [vp, vp, i32, vp, i32, vp, vp, i32, vp] + [i32] * 11),
    'lm_gn_finalize': (i32, [vp, vp, vp, i32, i32, i32, i32, f32]),
    'lm_gn_finalize_split': (i32, [vp, vp, vp, i32, i32, i32, i32, f32, i32]),
    'lm_stem_conv7x7_bn_relu': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32]),
    'lm_stem_conv7x7_bn_relu_u8': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32]),
    'lm_maxpool3x3s2_nhwc': (i32, [vp, vp, vp, i32, i32, i32, i32]),
    'lm_conv2d_nhwc_small': (i32, [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32]),
    'lm_gn_stats': (i32, [vp, vp, vp, vp, i32, i32, i32, f32]),
    'lm_gn_stats_workspace_bytes': (i64, [i32, i32, i32]),
    'lm_gn_relu_upsample': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32]),
    'lm_gn_relu_upsample_sum': (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    'lm_gn_relu_upsample_sum_conv1x1': (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, i32]),
    'lm_upsample_bilinear_nhwc': (i32, [vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32]),
    'lm_upsample_bilinear_to_chw': (i32, [vp, vp, i32, vp, i32, i32, i32, i32, i32, i32]),
    'lm_layernorm_rows': (i32, [vp, vp, vp, vp, vp, i64, i32, f32]),
    'lm_token_mix_mfma_f32': (i32, [vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32]),
    'lm_unpatchify': (i32, [vp, vp, vp, i32, i32, i32, i32]),
    'lm_attention_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, f32]),
    'lm_attention_masked_f32': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32]),
    'lm_head_tokens': (i32, [vp, vp, vp, vp, f32, i32, i32, i32, i32, i32, i32]),
    'lm_head_tokens_window': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32]),
    'lm_head_stage2': (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, i64]),
    'lm_head_proposal_conf': (i32, [vp, vp, vp, vp, vp, i32, i32]),
    'lm_head_endpoint_tile': (i32, []),
    'lm_head_endpoint': (i32, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    'lm_decode_proposals': (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32]),
    'lm_decode_orient': (i32, [vp, vp, i32, i32, vp, i64]),
    'lm_decode_semantic': (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32]),
    'lm_endp_topk_workspace_bytes': (i64, [i32]),
    'lm_endp_topk': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    'lm_pack_segments': (i32, [vp, i32, vp, vp, vp, vp]),
    'lm_bev_raster_workspace_bytes': (i64, [i32, i64, i32, i32]),
    'lm_bev_raster_batch': (i32, [vp, vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, vp, i64, vp, vp, i32, i32]),
    'lm_bev_raster_batch_scaled': (i32, [vp, vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, vp, i64, vp, vp, i32, i32, c_f32p]),
    'lm_tile_ingest_u8': (i32, [vp, vp, vp, i32, i32, i32, i32]),
    'lm_strip_build_grid': (i32, [C.POINTER(LmRasterParams), i32, i32, i32, C.c_double, C.c_double, C.POINTER(LmStripGrid), vp, i64]),
    'lm_strip_bin_workspace_bytes': (i64, [i64, i32]),
    'lm_strip_bin_points': (i32, [vp, vp, i64, C.POINTER(LmRasterParams), i32, i32, i32, C.c_double, C.c_double, vp, i64, vp, vp,
                                  C.POINTER(i64), vp, i64]),
    'lm_strip_plan_consts_bytes': (i64, [i32, i64]),
    'lm_strip_plan_create': (i32, [C.POINTER(LmRasterParams), i32, i32, i32, C.c_double, C.c_double, vp, i64, C.POINTER(vp), vp]),
    'lm_strip_plan_destroy': (i32, [vp]),
    'lm_strip_chunk_workspace_bytes': (i64, [i64, i32]),
    'lm_strip_bin_count': (i32, [vp, vp, i64, vp, i64, vp, vp]),
    'lm_strip_bin_scatter': (i32, [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp]),
    'lm_tile_ground_workspace_bytes': (i64, [i32, i32, i32, i32]),
    'lm_tile_ground': (i32, [vp, vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, i32, i32, i32, vp, i64, vp, vp, vp]),
    'lm_ground_select_workspace_bytes': (i64, [i64, i32]),
    'lm_ground_select': (i32, [vp, vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, i32, i32, i32, vp, f32, f32, vp, i64, vp, vp,
                               C.POINTER(i64)]),
    'lm_tile_intensity_workspace_bytes': (i64, [i32, i32]),
    'lm_tile_intensity_window': (i32, [vp, vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, i32, i32, C.POINTER(i32), i32, i32, i32, vp, i64,
                                       vp, vp, vp]),
    'lm_tile_intensity_cells_workspace_bytes': (i64, [i32, i32, i32, i32]),
    'lm_tile_intensity_cells': (i32, [vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp]),
    'lm_tile_intensity_apply_workspace_bytes': (i64, [i32]),
    'lm_tile_intensity_apply': (i32, [vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, i32, i32, i32, vp, vp, i64, vp, vp]),
    'lm_drape_workspace_bytes': (i64, [i64, i32, i32]),
    'lm_drape_vertices': (i32, [vp, vp, C.POINTER(i64), C.POINTER(LmRasterParams), i32, i32, i32, vp, C.POINTER(i64), i32, vp, i64, vp, vp, vp]),
    'lm_tile_gap_hist': (i32, [vp, vp, i32, i32, i32, i32, vp]),
    'lm_tile_gap_fill': (i32, [vp, vp, i32, i32, i32, C.POINTER(i32), vp]),
    'lm_endp_cluster': (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp]),
    'lm_polyline_assemble': (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, vp]),
    'lm_raster_polylines': (i32, [vp, i32, i32, vp]),
    'lm_line8': (i32, [vp, i32, i32, i32, i32, i32]),
    'lm_trace_lines': (i32, [vp, i32, i32, vp, vp]),
    'lm_polyline_backproject': (i32, [vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp]),
    'lm_polyline_backproject_z': (i32, [vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, i32]),
    'lm_skeletonize_lee_2d': (i64, [vp, i32, i32]),
    'lm_merge_create': (vp, []),
    'lm_merge_destroy': (None, [vp]),
    'lm_merge_add_tile': (i32, [vp, vp, vp, i32]),
    'lm_merge_finish': (i64, [vp, C.POINTER(i64)]),
    'lm_merge_result': (i32, [vp, vp, vp]),
    'lm_downsample_seq': (i32, [vp, i32, C.c_double, vp]),
    'lm_softmax_rows': (i32, [vp, vp, i64, i32]),
    'lm_rowref_select': (i32, [vp, vp, vp, vp, vp, f32, vp, i32, i32, i32, i32]),
    'lm_rowref_gather': (i32, [vp, vp, vp, vp, i32, i32, i32, i32]),
    'lm_rowref_scatter': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    'lm_rowref_gather_win': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    'lm_rowref_scatter_win': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    'lm_rowref_decode': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    'lm_voxelize_workspace_bytes': (i64, [i64]),
    'lm_scan_workspace_bytes': (i64, [i64]),
    'lm_exclusive_scan_u32': (i32, [vp, vp, vp, i64, vp, i64]),
    'lm_sort_pairs_workspace_bytes': (i64, [i64]),
    'lm_sort_pairs_u32': (i32, [vp, vp, vp, i64, i32, vp, i64]),
    'lm_voxelize_hard': (i32, [vp, vp, i64, c_f32p, c_f32p, C.POINTER(i32), i32, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp, i64]),
    'lm_sparse_grid_build': (i32, [vp, vp, i64, vp, i32, i32, i32, i32]),
    'lm_sparse_conv_outputs_workspace_bytes': (i64, [i64]),
    'lm_sparse_conv_outputs': (i32, [vp, vp, i64, i32, C.POINTER(i32), i32, i32, i32, vp, vp, i32, vp, vp, i64]),
    'lm_sparse_rulebook': (i32, [vp, vp, i64, vp, i32, i32, i32, i32, C.POINTER(i32), vp]),
    'lm_conv_gather_mfma_f32': (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i64, i32, i32, i32]),
    'lm_sparse_to_dense_nhwc': (i32, [vp, vp, i32, vp, i64, vp, i32, i32, i32, i32, i32, i32]),
    'lm_upsample_bicubic_nhwc': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32]),
    'lm_las_parse_header': (i32, [vp, i64, C.POINTER(LmLasHeader)]),
    'lm_las_decode_points': (i32, [vp, vp, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), f32, f32,
                                   i32, vp]),
    'lm_las_select_workspace_bytes': (i64, [i64]),
    'lm_las_decode_select': (i32, [vp, vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), f32, f32,
                                   i32, C.POINTER(LmLasSelect), vp, i64, vp, vp, vp]),
    'lm_line_index_build': (i32, [vp, i64, f32, C.c_double, C.POINTER(LmLineGrid), vp, i64, vp, i64]),
    'lm_label_points': (i32, [vp, vp, i64, vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, f32, f32, vp, vp]),
    'lm_las_label_records': (i32, [vp, vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, f32, f32, i32, i32, vp, vp, vp, i32]),
    'lm_line_profile_points': (i32, [vp, vp, i64, vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double, f32, f32, i32, vp, i64]),
    'lm_las_line_profile_records': (i32, [vp, vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double, f32, f32,
                                          i32, vp, i64]),
    'lm_las_line_colour_records': (i32, [vp, vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double, f32, f32,
                                         i32, i32, vp, vp, i64]),
    'lm_line_cross_points': (i32, [vp, vp, i64, vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double, f32, i32, i32, i32, vp, i64]),
    'lm_las_line_cross_records': (i32, [vp, vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double, f32, i32,
                                        i32, i32, vp, i64]),
    'lm_line_hist_points': (i32, [vp, i64, vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, i32, f32, i32, i32, i32, vp, i64, vp]),
    'lm_las_line_hist_records': (i32, [vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, i32, f32, i32, i32, i32, vp,
                                       i64, vp]),
    'lm_las_line_hist_window_records': (i32, [vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, i32, f32, i32, i32, i32,
                                              vp, i64, vp, vp, C.c_double, vp]),
    'lm_las_label_records_local': (i32, [vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, f32, C.POINTER(LmPaintTable), i32, i32,
                                         vp, vp, vp, i32, vp]),
    'lm_las_line_profile_records_local': (i32, [vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double,
                                                f32, C.POINTER(LmPaintTable), i32, vp, i64, vp]),
    'lm_las_line_colour_records_local': (i32, [vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double,
                                               f32, C.POINTER(LmPaintTable), i32, i32, vp, vp, i64, vp]),
    'lm_las_line_cross_records_local': (i32, [vp, i32, i32, i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.POINTER(LmLasSelect), vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, vp, vp, vp, i32, C.c_double,
                                              f32, i32, C.POINTER(LmPaintTable), i32, vp, i64, vp]),
    'lm_residue_keys_local': (i32, [vp, i64, vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, f32, C.POINTER(LmPaintTable), i32, f32, C.c_double, i32,
                                    i32, vp, vp, vp]),
    'lm_residue_keys': (i32, [vp, vp, i64, vp, i64, C.POINTER(LmLineGrid), vp, vp, f32, f32, f32, f32, C.c_double, i32, i32, vp, vp]),
    'lm_cell_components': (i32, [vp, vp, i64, i32, i32, i32, vp, vp]),
    'lm_residue_stats': (i32, [vp, vp, vp, i32, i32, vp, vp, i64, i64, vp]),
    'lm_png_info': (i32, [vp, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    'lm_png_decode_u8': (i32, [vp, i64, vp, i64]),
    'lm_png_decode_files_u8': (i32, [C.POINTER(C.c_char_p), i32, vp, i32, i32, i32, i32]),
    'lm_zlib_inflate': (i32, [vp, i64, vp, i64, C.POINTER(i64)]),
    'lm_lane_json_text': (i64, [vp, i32, i32, i32, vp, i64]),
    'lm_lane_json_write': (i32, [vp, i32, i32, i32, C.c_char_p]),
    'lm_seqs_json_write': (i32, [vp, vp, i32, i32, i32, C.c_char_p]),
}

_lib = None


class LanemapHipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LanemapHipError(
                f'{LIB_PATH} is missing: the HIP library is the only implementation of this package '
                '(no CPU fallback). Build it with `python -m lanemapping_amd.build`.')
        import torch  # noqa: F401  first: the process must hold ONE HIP runtime, the one torch loads (loading ours before
        #                     torch's made every later launch fail with "no ROCm-capable device is detected")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)           # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != 0:
        raise LanemapHipError(f'lanemap_hip error {code}: {lib().lm_last_error().decode()}')
