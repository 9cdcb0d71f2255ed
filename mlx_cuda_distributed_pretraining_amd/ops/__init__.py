from .rmsnorm import RMSNorm, rms_norm, rms_norm_ref
from .rope import RopeTable, apply_rope, rope_ref
from .qk_norm import qk_norm_rope
from .swiglu import swiglu, swiglu_ref
from .cross_entropy import (
    cross_entropy_capped,
    cross_entropy_ref,
    cross_entropy_with_z,
    fused_cross_entropy,
)
from .softcap import softcap, softcap_
from .attention import (
    BlockMask,
    attention_ref,
    create_block_mask,
    document_bounds,
    flash_attention,
    flex_attention,
)
from .sampling import make_sampler, make_logits_processors, sample_token
from .gemv import FastLinear, linear_fast
from .fp8 import fp8_linear, quantize_e4m3
from . import fused_optim
from ._ext import get_ext, require_ext

__all__ = [
    "RMSNorm", "rms_norm", "rms_norm_ref",
    "RopeTable", "apply_rope", "rope_ref",
    "qk_norm_rope",
    "swiglu", "swiglu_ref",
    "fused_cross_entropy", "cross_entropy_ref", "cross_entropy_with_z",
    "cross_entropy_capped", "softcap", "softcap_",
    "BlockMask", "attention_ref", "create_block_mask", "document_bounds",
    "flash_attention", "flex_attention",
    "make_sampler", "make_logits_processors", "sample_token",
    "FastLinear", "linear_fast", "fp8_linear", "quantize_e4m3",
    "fused_optim", "get_ext", "require_ext",
]
