"""ctypes binding of libpgdvs_hip.so (C ABI declared in include/pgdvs_hip.h).

There is no CPU fallback: if the shared library is missing or an op is handed a
non-GPU tensor the call raises.  Build with ``python __graft_entry__.py`` (or
``make -C ml-pgdvs_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import pathlib

_PKG = pathlib.Path(__file__).resolve().parent
LIB_PATH = _PKG.parent / "lib" / "libpgdvs_hip.so"

CAM_BLOCK = 80

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float

# name -> (restype, argtypes); mirrors include/pgdvs_hip.h one-to-one
SIGNATURES = {
    "pgdvs_last_error": (C.c_char_p, []),
    "pgdvs_option_set": (_i, [C.c_char_p, C.c_double]),
    "pgdvs_option_get": (C.c_double, [C.c_char_p]),
    "pgdvs_abi_version": (_i, []),
    "pgdvs_build_arch": (C.c_char_p, []),
    "pgdvs_prof_enable": (None, [_i]),
    "pgdvs_prof_report": (_i, [C.c_char_p, _i]),
    "pgdvs_prof_overhead_ms": (C.c_double, []),
    "pgdvs_cam_prep": (_i, [_vp, _i, _vp, _vp]),
    "pgdvs_get_rays": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pgdvs_dyn_warp": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pgdvs_compact_workspace_bytes": (_i64, [_i64]),
    "pgdvs_compact_u8": (_i, [_vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_gather_rows": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp]),
    "pgdvs_knn_workspace_bytes": (_i64, [_i64]),
    "pgdvs_knn_mean_dist": (_i, [_vp, _vp, _i64, _i, _vp, _i, _vp, _i64, _vp]),
    "pgdvs_outlier_workspace_bytes": (_i64, [_i64]),
    "pgdvs_outlier_flags": (_i, [_vp, _vp, _i64, _f, _i, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_scatter_keep": (_i, [_vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "pgdvs_project_flow_dense": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pgdvs_project_points": (_i, [_vp, _vp, _i64, _vp, _vp]),
    "pgdvs_backwarp_l1": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "pgdvs_softsplat_workspace_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "pgdvs_softsplat_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    "pgdvs_softsplat_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pgdvs_dyn_splat_workspace_bytes": (_i64, [_i, _i]),
    "pgdvs_dyn_splat_composite": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_dyn_splat_composite_rng": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_splat_noise_field": (_i, [_i, _i, _vp, _vp, _vp]),
    "pgdvs_points_raster_workspace_bytes": (_i64, [_i64, _i, _i, _f]),
    "pgdvs_points_raster": (_i, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i64, _vp]),
    "pgdvs_points_raster_bounded": (_i, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp,
                                         _vp, _i64, _vp]),
    "pgdvs_static_aggregate_workspace_bytes": (_i64, [_i, _i, _i, _i64]),
    "pgdvs_static_aggregate": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _vp, _i64, _vp]),
    "pgdvs_static_aggregate_packed": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "pgdvs_gnt_gather": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _vp,
                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pgdvs_gnt_embed_weight_floats": (_i64, [_i]),
    "pgdvs_gnt_embed": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp]),
    "pgdvs_gnt_posfc": (_i, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i, _vp, _vp]),
    "pgdvs_gnt_head": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pgdvs_gnt_view_weight_floats": (_i64, []),
    "pgdvs_gnt_view_layer": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "pgdvs_gnt_ray_layer": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "pgdvs_mesh_render_workspace_bytes": (_i64, [_i, _i]),
    "pgdvs_mesh_render": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_track_points": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pgdvs_knn_cross_workspace_bytes": (_i64, [_i64, _i64]),
    "pgdvs_knn_cross_mean_dist": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _i, _vp, _vp, _i64, _vp]),
    "pgdvs_threshold_flags": (_i, [_vp, _vp, _i64, _vp, _f, _vp, _vp, _vp, _vp]),
    "pgdvs_concat_rows": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "pgdvs_combine": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
}


class ViewGeoDesc(C.Structure):
    """``pgdvs_view_geo_desc`` (include/pgdvs_hip.h), field for field."""
    _fields_ = [
        ("H", C.c_int32), ("W", C.c_int32),
        ("flat_cam_tgt", _vp), ("flat_cam_src", _vp), ("time_src", _vp), ("time_tgt", _vp),
        ("rgb1", _vp), ("rgb2", _vp), ("depth1", _vp), ("depth2", _vp), ("dyn_mask1", _vp), ("flow12", _vp), ("flow_occ", _vp),
        ("use_flow_consistency", C.c_int32), ("remove_outlier", C.c_int32), ("outlier_knn", C.c_int32),
        ("outlier_std_thres", _f), ("alpha", _f),
        ("noise", _vp), ("rng_state", _vp),
        ("st_pcl_rgb", _vp), ("st_pcl_xyz", _vp), ("st_rows", _i64), ("st_count_dev", _vp),
        ("agg_S", C.c_int32), ("agg_rgbs", _vp), ("agg_depths", _vp), ("agg_masks", _vp), ("agg_K3s_host", _vp),
        ("agg_c2ws_host", _vp), ("agg_cloud_out", _vp), ("agg_xyz_out", _vp), ("agg_capacity", _i64), ("agg_count_out", _vp),
        ("row_bound", _i64), ("radius", _f), ("K", C.c_int32),
        ("static_rgb", _vp), ("static_mask", _vp), ("raster_status", _vp), ("render_dyn_rgb", _vp), ("render_dyn_mask", _vp),
        ("combined", _vp), ("combined_static", _vp), ("combined_dyn", _vp),
        ("side_stream", _vp), ("agg_params_cached", C.c_int32),
    ]


class JpegInfo(C.Structure):
    """``pgdvs_jpeg_info`` (include/pgdvs_hip.h), field for field."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("sampling", C.c_int32), ("restart_interval", C.c_int32),
        ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3), ("coef_bytes", _i64), ("quant", (C.c_uint16 * 64) * 3),
    ]


class PngImage(C.Structure):
    """``pgdvs_png_image`` (include/pgdvs_hip.h), field for field: one entry of the table at the front of a batch buffer."""
    _fields_ = [
        ("offset", _i64), ("size", _i64), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("out_channels", C.c_int32),
        ("row_stride", _i64), ("out", _vp), ("bit_depth", C.c_int32), ("scale", C.c_int32),
    ]


class DepthEntry(C.Structure):
    """``pgdvs_depth_entry`` (include/pgdvs_hip.h), field for field: one entry of the table at the front of a depth batch buffer."""
    _fields_ = [
        ("offset", _i64), ("h", C.c_int32), ("w", C.c_int32), ("op", C.c_int32), ("scale", C.c_float), ("map", _vp), ("out", _vp),
        ("out_row_stride", _i64), ("H", C.c_int32), ("W", C.c_int32),
    ]


class JpegScanHeader(C.Structure):
    """The front of the buffer ``pgdvs_jpeg_scan_prepare`` fills (csrc/jpeg_scan_core.h ``jscan::Header``), field for field:
    the offsets are bytes from the buffer's start."""
    _fields_ = [
        ("magic", C.c_uint32), ("sub_bytes", C.c_int32), ("nseg", C.c_int32), ("nsub", C.c_int32), ("h", C.c_int32), ("v", C.c_int32),
        ("mcus_w", C.c_int32), ("mcus_h", C.c_int32), ("restart_mcus", C.c_int32), ("reserved0", C.c_int32), ("coef_bytes", _i64),
        ("stream_bytes", _i64), ("off_quant", _i64), ("off_tables", _i64), ("off_segments", _i64), ("off_sub_segment", _i64),
        ("off_stream", _i64), ("total_bytes", _i64), ("reserved", _i64 * 4),
    ]


SIGNATURES.update({
    "pgdvs_eval_psnr_workspace_bytes": (_i64, []),
    "pgdvs_eval_psnr_sums": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_eval_ssim_workspace_bytes": (_i64, [_i, _i]),
    "pgdvs_eval_ssim_sums": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_lpips_workspace_bytes": (_i64, [_i, _i]),
    "pgdvs_lpips_sums": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_dycheck_psnr_ssim_workspace_bytes": (_i64, [_i, _i]),
    "pgdvs_dycheck_psnr_ssim_sums": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_dycheck_lpips_workspace_bytes": (_i64, [_i, _i]),
    "pgdvs_dycheck_lpips": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_dycheck_depth_range_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "pgdvs_dycheck_depth_range": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _i64,
                                       _vp]),
    "pgdvs_nvidia_depth_range_workspace_bytes": (_i64, [_i, _i, _i]),
    "pgdvs_nvidia_depth_range": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_nvidia_zoe_depth_range_workspace_bytes": (_i64, [_i, _i, _i]),
    "pgdvs_nvidia_zoe_depth_range": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_png_scanlines": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pgdvs_eval_export_scanlines": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "pgdvs_jpeg_coefficients": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pgdvs_jpeg_scan_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "pgdvs_jpeg_scan": (_i, [_vp, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _i64, _vp]),
    "pgdvs_jpeg_coefficients_420": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pgdvs_jpeg_scan_420_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "pgdvs_jpeg_scan_420": (_i, [_vp, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _i64, _vp]),
    "pgdvs_png_deflate_workspace_bytes": (_i64, [_i, _i64, _i]),
    "pgdvs_png_deflate": (_i, [_vp, _i, _i64, _i, _vp, _i64, _vp, _vp, _i64, _vp]),
    "pgdvs_flow_consistency": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "pgdvs_epipolar_mask": (_i, [_vp, _vp, _i, _i, _vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    "pgdvs_flow_tile_blend": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "pgdvs_flow_pair_export_workspace_bytes": (_i64, [_i, _i]),
    "pgdvs_flow_pair_export": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_zoe_sample_workspace_bytes": (_i64, [_i, _i, _i64]),
    "pgdvs_zoe_sample": (_i, [_vp, _vp, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_zoe_fit_workspace_bytes": (_i64, [_i64]),
    "pgdvs_zoe_fit": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_zoe_errors": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "pgdvs_mask_combine_workspace_bytes": (_i64, [_i, _i, _i]),
    "pgdvs_mask_combine": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_semantic_mask": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "pgdvs_cotracker_pyramid_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "pgdvs_cotracker_pyramid": (_i, [_vp, _i, _i, _i, _i, _vp, _i64, _vp]),
    "pgdvs_cotracker_corr_lookup": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _i64, _i64, _vp]),
    "pgdvs_item_views": (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _i64, _i64, _vp, _i, _vp, _i, _vp, _vp]),
    "pgdvs_flow_occ": (_i, [_vp, _i, _i, _f, _vp, _vp]),
    "pgdvs_item_target": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "pgdvs_item_zoe_depths_workspace_bytes": (_i64, [_i, _i, _i]),
    "pgdvs_item_zoe_depths": (_i, [_vp, _i, _i, _i, _i64, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_resample_table": (_i, [_i, _i, _i, _vp, _vp]),
    "pgdvs_resample_u8_workspace_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "pgdvs_resample_u8": (_i, [_vp, _i64, _i, _i, _i, _i, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pgdvs_jpeg_info_size": (_i64, []),
    "pgdvs_jpeg_parse": (_i, [_vp, _i64, C.POINTER(JpegInfo)]),
    "pgdvs_jpeg_entropy_decode": (_i, [_vp, _i64, _vp, _i64]),
    "pgdvs_jpeg_reconstruct_workspace_bytes": (_i64, [C.POINTER(JpegInfo)]),
    "pgdvs_jpeg_reconstruct": (_i, [_vp, _vp, C.POINTER(JpegInfo), _vp, _i64, _vp, _i64, _vp]),
    "pgdvs_jpeg_scan_prepare_bytes": (_i64, [_vp, _i64, C.c_int32]),
    "pgdvs_jpeg_scan_prepare": (_i, [_vp, _i64, C.c_int32, _vp, _i64, C.POINTER(JpegInfo)]),
    "pgdvs_jpeg_scan_decode_workspace_bytes": (_i64, [_vp, _i64]),
    "pgdvs_jpeg_scan_decode": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "pgdvs_jpeg_scan_decode_host": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64]),
    "pgdvs_png_inflate_workspace_bytes": (_i64, [_vp, C.c_int32]),
    "pgdvs_png_decode": (_i, [_vp, _vp, _i64, C.c_int32, C.c_int32, _vp, _vp, _i64, _vp]),
    "pgdvs_png_decode_host": (_i, [_vp, _vp, _i64, C.c_int32, C.c_int32, _vp, _vp, _i64]),
    "pgdvs_mask_place": (_i, [_vp, C.c_int32, C.c_int32, C.c_int32, _i64, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _i64, _vp]),
    "pgdvs_depth_place": (_i, [_vp, _vp, _i64, C.c_int32, _vp]),
    "pgdvs_percentile_f32_workspace_bytes": (_i64, [_vp, C.c_int32]),
    "pgdvs_percentile_f32": (_i, [_vp, _vp, C.c_int32, C.c_double, _vp, _vp, _i64, _vp]),
    "pgdvs_view_geo_desc_size": (_i64, []),
    "pgdvs_view_geo_workspace_bytes": (_i64, [C.POINTER(ViewGeoDesc)]),
    "pgdvs_view_geo_forward": (_i, [C.POINTER(ViewGeoDesc), _vp, _i64, _vp]),
    "pgdvs_view_geo_counters": (_i, [C.POINTER(ViewGeoDesc), _vp, _i64, _vp, _vp]),
    "pgdvs_view_geo_host_stats": (None, [C.POINTER(_i64), C.POINTER(C.c_double)]),
})

_lib = None


class PgdvsHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load libpgdvs_hip.so; raises (never falls back) when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise PgdvsHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` from the repo root "
            "(needs hipcc). There is no CPU fallback for the product path."
        )
    # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so).  It must be the ONE runtime of the
    # process: loaded first, the dynamic loader binds this library's libamdhip64 references to it.  Loaded
    # second (after /opt/rocm's copy came in through this library), torch's streams and allocations live in a
    # different runtime instance than our launches ("no ROCm-capable device is detected").
    import torch  # noqa: F401

    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.pgdvs_view_geo_desc_size() != C.sizeof(ViewGeoDesc):
        raise PgdvsHipError(f"pgdvs_view_geo_desc: the library's struct has {lib.pgdvs_view_geo_desc_size()} bytes, this binding's "
                            f"{C.sizeof(ViewGeoDesc)} -- rebuild the extension (stale {LIB_PATH.name})")
    if lib.pgdvs_jpeg_info_size() != C.sizeof(JpegInfo):
        raise PgdvsHipError(f"pgdvs_jpeg_info: the library's struct has {lib.pgdvs_jpeg_info_size()} bytes, this binding's "
                            f"{C.sizeof(JpegInfo)} -- rebuild the extension (stale {LIB_PATH.name})")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().pgdvs_last_error().decode("utf-8", "replace")
        raise PgdvsHipError(f"{what} failed (rc={rc}): {msg}")
