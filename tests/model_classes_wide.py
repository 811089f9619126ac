"""A ColQwen3-style retrieval model owned by this test suite: transformers' Qwen3-VL backbone followed by the embedding tail with a
projection to 320 columns (the width of the ColQwen3 family), which colpali_amd/models.py replaces with the fused head when width 320
is admitted there.

Like tests/model_classes.py: the class carries a `colpali_engine.models.*` module name, which is how patch_colpali_engine recognises
model classes; nothing of `colpali_engine` is needed.  Random init, tiny config; no weights exist offline.
"""
import sys

import torch
from transformers import Qwen3VLConfig, Qwen3VLModel, Qwen3VLPreTrainedModel

MODULE_NAME = "colpali_engine.models.test_suite_models_wide"
EMBED_DIM = 320


class ColQwen3(Qwen3VLPreTrainedModel):
    """Qwen3-VL backbone, text inputs (left padded, as the family's processor pads)."""

    def __init__(self, config, mask_non_image_embeddings=False):
        super().__init__(config)
        self.model = Qwen3VLModel(config)
        self.dim = EMBED_DIM
        self.custom_text_proj = torch.nn.Linear(config.text_config.hidden_size, self.dim)
        self.mask_non_image_embeddings = mask_non_image_embeddings
        self.post_init()

    def get_input_embeddings(self):
        return self.model.get_input_embeddings()

    def forward(self, *args, **kwargs):
        out = self.model(*args, **kwargs, use_cache=False, return_dict=True)
        proj = self.custom_text_proj(out.last_hidden_state)
        proj = proj / proj.norm(dim=-1, keepdim=True)
        proj = proj * kwargs["attention_mask"].unsqueeze(-1)
        if "pixel_values" in kwargs and self.mask_non_image_embeddings:
            proj = proj * (kwargs["input_ids"] == self.config.image_token_id).unsqueeze(-1)
        return proj


ColQwen3.__module__ = MODULE_NAME
sys.modules.setdefault(MODULE_NAME, sys.modules[__name__])


def tiny_colqwen3(hidden=128, seed=0):
    cfg = Qwen3VLConfig(
        text_config=dict(hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=1, head_dim=hidden // 2, vocab_size=300, max_position_embeddings=512,
                         rope_scaling={"rope_type": "default", "mrope_section": [hidden // 16, 3 * hidden // 32, 3 * hidden // 32],
                                       "mrope_interleaved": True},
                         bos_token_id=1, eos_token_id=2),
        vision_config=dict(depth=1, hidden_size=32, intermediate_size=64, num_heads=2, patch_size=14, spatial_merge_size=2,
                           temporal_patch_size=2, in_channels=3, out_hidden_size=hidden, num_position_embeddings=64,
                           deepstack_visual_indexes=[0]),
        image_token_id=299, video_token_id=298, vision_start_token_id=297, vision_end_token_id=296)
    torch.manual_seed(seed)
    return ColQwen3(cfg).eval(), ColQwen3
