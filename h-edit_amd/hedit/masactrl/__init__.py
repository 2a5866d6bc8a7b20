from .masactrl import (MutualSelfAttentionControl, MutualSelfAttentionControlMask,  # noqa: F401
                       MutualSelfAttentionControlMaskAuto)
from .masactrl_utils import AttentionBase, regiter_attention_editor_diffusers  # noqa: F401
