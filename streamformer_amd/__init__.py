"""streamformer_amd — MI355X-native (gfx950) StreamFormer encoder hot path.

One hot path of Go2Heart/StreamFormer, rebuilt from scratch: the
``TimesformerMultiTaskingModelSigLIP`` forward (+ its KV-cached streaming variant and the
retrieval / localization loss heads), as hand-written HIP kernels behind a C ABI
(``include/streamformer_hip.h``), with this package as the Python mirror of the reference module.
Importing the package loads ``libstreamformer_hip.so``; there is no fallback if it is missing.
"""
from .configuration import StreamformerConfig, siglip_base  # noqa: F401
from .init_weights import make_state_dict, state_dict_sha256  # noqa: F401
from . import _native  # noqa: F401  (raises ImportError when the HIP library is not built)
from .modeling import (  # noqa: F401
    BaseModelOutputWithPast,
    BaseModelOutputWithPooling,
    StreamCache,
    StreamSnapshot,
    TimesformerMultiTaskingModelSigLIP,
    TimesformerVisionTower,
)
from . import heads  # noqa: F401
from .multitask import (  # noqa: F401
    StreamformerForMultiTaskingSigLIP,
    TimesformerUniversalLocalizationHead,
    TimesformerVideoRetrievalHead,
)
from .text import SiglipTextConfig, SiglipTextModel, encode_captions, encode_label_prompts  # noqa: F401
from .connector import StreamingVideoTokens, VideoTokenConnector  # noqa: F401
from .oad import OADConfig, OnlineActionDetector, StreamingActionDetector  # noqa: F401
from . import msda  # noqa: F401
from .msda import MSDeformAttn, MSDeformAttnFunction, as_compiled_op, ms_deform_attn  # noqa: F401
from .adapter import TimesformerMultiTaskingModelSigLIPViTAdapter  # noqa: F401
from .pixel_decoder import MSDeformAttnPixelDecoder, ShapeSpec  # noqa: F401
from .mask_decoder import CLMultiScaleMaskedTransformerDecoder, MultiScaleMaskedTransformerDecoder  # noqa: F401
from .vis import SimpleTracker, VideoInstanceSegmenter, postprocess_video_masks  # noqa: F401
from .segmentation import (  # noqa: F401
    ImageSegmenter,
    SegmentationInstances,
    instance_inference,
    panoptic_inference,
    panoptic_segments_host,
    semantic_inference,
)
from .criterion import HungarianMatcher, SetCriterion  # noqa: F401
from .cl_plugin import CTCLPlugin, ctvis_train_losses  # noqa: F401
from .masked_attention import (  # noqa: F401
    MaskedAttentionFunction,
    MaskedMultiheadAttention,
    PackedAttentionMask,
    masked_attention,
    pack_attention_mask,
    use_native_attention,
)
from .processing import TimesformerImageProcessor  # noqa: F401

__version__ = "0.1.0"
