"""videocof_amd -- MI355X-native Wan2.1-DiT video denoising path (VideoCoF-compatible).

Host side mirrors the reference's interface for this path only:

    videocof_amd.WanTransformer3DModel      <- videox_fun/models/wan_transformer3d.py
    videocof_amd.attention                  <- videox_fun/models/attention_utils.py
    videocof_amd.FlowUniPCMultistepScheduler<- videox_fun/utils/fm_solvers_unipc.py
    videocof_amd.FlowDPMSolverMultistepScheduler <- videox_fun/utils/fm_solvers.py (+ get_sampling_sigmas, retrieve_timesteps)
    videocof_amd.WanPipeline                <- videox_fun/pipeline/pipeline_wan.py
    videocof_amd.AutoencoderKLWan           <- videox_fun/models/wan_vae.py
    videocof_amd.WanT5EncoderModel          <- videox_fun/models/wan_text_encoder.py (umT5 encoder)
    videocof_amd.lora_utils                 <- videox_fun/utils/lora_utils.py (merge_lora on state dicts)
    videocof_amd.cache_utils                <- videox_fun/models/cache_utils.py (TeaCache, opt-in)
    videocof_amd.dist                       <- videox_fun/dist/{fuser,wan_xfuser}.py (Ulysses on RCCL)
    videocof_amd.video_io                   <- fast_infer.py load_video_frames + videox_fun/utils/utils.py save_videos_grid's byte conversion
    videocof_amd.windows                    (no counterpart) temporal and spatial context windows: clips longer / frames larger than trained, opt-in
    videocof_amd.edit_region                (no counterpart) edit region: the denoise loop only on the rectangle (and, on request, the frame range; on request a rectangle that follows the mask from frame to frame, or one box per separate object) the edit mask touches, opt-in and lossy
    videocof_amd.local_attention            (no counterpart) local self-attention: key tiles listed per query block, opt-in and lossy

Device arithmetic lives in ``libwan_hip.so`` (csrc/, C ABI in include/wan_hip.h).
"""
from .fm_solvers_unipc import FlowUniPCMultistepScheduler  # noqa: F401
from .fm_solvers import FlowDPMSolverMultistepScheduler, get_sampling_sigmas, retrieve_timesteps  # noqa: F401
from .pipeline_wan import WanPipeline, WanPipelineOutput  # noqa: F401
from .wan_transformer3d import WanTransformer3DModel  # noqa: F401
from .graph import GraphedForward, GraphedLoop  # noqa: F401
from .cache_utils import TeaCache, get_teacache_coefficients  # noqa: F401
from .attention_utils import attention, flash_attention  # noqa: F401
from .wan_vae import AutoencoderKLWan  # noqa: F401
from .wan_text_encoder import WanT5EncoderModel  # noqa: F401
from .video_io import frames_to_video, video_to_frames, load_video_frames  # noqa: F401
from .video_io import FitPlan, fit_size, fit_plan, fit_frames, restore_frames, reference_fit_frames  # noqa: F401
from .video_io import change_mask, composite_frames, keep_unedited, reference_change_mask, reference_composite_frames  # noqa: F401
from .video_io import (fit_mask, latent_edit_mask, reference_fit_mask, reference_latent_edit_mask,  # noqa: F401
                       reference_masked_prediction)
from .video_io import ClipStats, clip_stats, reference_clip_stats, vae_roundtrip_frames  # noqa: F401
from .video_io import (color_match, color_match_coefficients, reference_color_match, reference_color_stats,  # noqa: F401
                       reference_color_coefficients, reference_frames_affine)
from .video_io import grid_frames, compare_frames, reference_grid_frames, reference_compare_frames  # noqa: F401
from .video_io import yuv_matrix, yuv_to_frames, frames_to_yuv, reference_yuv_to_frames, reference_frames_to_yuv  # noqa: F401
from .video_io import YuvClip, read_y4m, load_y4m_frames, write_y4m  # noqa: F401
from .windows import WindowPlan, window_plan, window_latent_frames, reference_window_gather, reference_window_blend  # noqa: F401
from .windows import TilePlan, spatial_window_cells, reference_tile_gather, reference_tile_blend  # noqa: F401
from .edit_region import (RegionPlan, region_plan, region_margin_cells, reference_mask_bounds, reference_region_crop,  # noqa: F401
                          reference_region_restore)
from .edit_region import (TimeRegion, region_time_plan, region_time_margin_frames, reference_region_crop_frames,  # noqa: F401
                          reference_region_restore_frames)
from .edit_region import region_vae_box, reference_frames_box_to_video, reference_video_box_stitch  # noqa: F401
from .edit_region import (TrackPlan, region_track_plan, region_follow_frames, reference_region_crop_track,  # noqa: F401
                          reference_region_restore_track)
from .edit_region import (SplitPlan, region_split_plan, reference_mask_spans, reference_region_crop_split,  # noqa: F401
                          reference_region_restore_split)
from .local_attention import LocalAttentionPlan, local_attention_plan, reference_local_mask, reference_sparse_attention  # noqa: F401

__version__ = "0.1.0"
