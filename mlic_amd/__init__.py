"""mlic_amd: MI355X-native (gfx950) MLIC++ encode/decode behind the CompressAI-style API.

    from mlic_amd import get_model
    net = get_model("MLICPP_L").cuda().eval()
"""
from .models import MLICPlusPlus, MLICPlusPlusSD, MLICPlusPlusSDVbr, MLICPlusPlusVbr, get_model, model_config  # noqa: F401
from .metrics import DISTS, LPIPS, dists_synthetic_weights, lpips_synthetic_weights, ms_ssim_db, ms_ssim_u8  # noqa: F401
from .codec import blur3_pad, decode_images, egress_u8, encode_images, ingest_u8, peek, rate_loop  # noqa: F401
from .codec import (coded_size, egress_u8_scaled, ingest_u8_scaled, is_scaled_file, parse_container_scaled,  # noqa: F401
                    resample_table, write_container_scaled)
from .codec import (is_residual_file, parse_container_residual, residual_apply, residual_front,  # noqa: F401
                    residual_tables, strip_residual, write_container_residual)
from .codec import (is_residual_seg_file, parse_container_residual_seg, residual_decode_segments,  # noqa: F401
                    residual_encode_segments, write_container_residual_seg)
from .codec import (encode_residual16, is_residual_deep_file, parse_container_residual_deep,  # noqa: F401
                    residual_apply16, residual_front16, residual_shift, residual_stats16,
                    write_container_residual_deep)
from .codec import (encode_residual_yuv, is_residual_yuv_file, parse_container_residual_yuv,  # noqa: F401
                    residual_apply_yuv, residual_front_yuv, residual_stats_yuv, residual_yuv_format,
                    write_container_residual_yuv)
from .codec import blend_tiles, decode_tiled, encode_tiled, tile_grid  # noqa: F401
from .codec import YuvFormat, decode_yuv, egress_yuv, encode_yuv, ingest_yuv, split_yuv  # noqa: F401
from .codec import egress_u16, ingest_u16  # noqa: F401
from .codec import heat_u8, rate_map, rate_maps, sq_err_blocks  # noqa: F401
from .spec import CONFIGS  # noqa: F401

__all__ = ["MLICPlusPlus", "MLICPlusPlusSD", "MLICPlusPlusSDVbr", "MLICPlusPlusVbr", "get_model", "model_config", "CONFIGS",
           "ms_ssim_u8", "ms_ssim_db", "LPIPS", "lpips_synthetic_weights", "DISTS", "dists_synthetic_weights", "ingest_u8", "egress_u8", "encode_images", "decode_images", "peek",
           "blur3_pad", "rate_loop", "tile_grid", "blend_tiles", "encode_tiled", "decode_tiled",
           "resample_table", "ingest_u8_scaled", "egress_u8_scaled", "write_container_scaled", "parse_container_scaled",
           "is_scaled_file", "coded_size", "rate_maps", "rate_map", "sq_err_blocks", "heat_u8",
           "residual_front", "residual_apply", "residual_tables", "write_container_residual", "parse_container_residual",
           "is_residual_file", "strip_residual", "is_residual_seg_file", "parse_container_residual_seg",
           "write_container_residual_seg", "residual_encode_segments", "residual_decode_segments",
           "encode_residual16", "is_residual_deep_file", "parse_container_residual_deep", "residual_apply16",
           "residual_front16", "residual_shift", "residual_stats16", "write_container_residual_deep",
           "encode_residual_yuv", "is_residual_yuv_file", "parse_container_residual_yuv", "residual_apply_yuv",
           "residual_front_yuv", "residual_stats_yuv", "residual_yuv_format", "write_container_residual_yuv"]
