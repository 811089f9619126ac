"""Col*-style retrieval models owned by this test suite: a transformers vision-language backbone followed by the embedding tail that
colpali_amd/models.py replaces with the fused head (projection to 128, L2 normalisation, attention mask, optional image-token mask).

They exist so that patch_colpali_engine(models=True) can be tested on real backbones from this repository alone.  The classes carry a
`colpali_engine.models.*` module name, which is how the patch recognises model classes; nothing else of `colpali_engine` is needed.
"""
import sys

import torch
from transformers import PaliGemmaModel, PaliGemmaPreTrainedModel, Qwen2VLModel, Qwen2VLPreTrainedModel

MODULE_NAME = "colpali_engine.models.test_suite_models"
EMBED_DIM = 128


def _embedding_tail(model, last_hidden_state, kwargs, image_token_id):
    proj = model.custom_text_proj(last_hidden_state)
    proj = proj / proj.norm(dim=-1, keepdim=True)
    proj = proj * kwargs["attention_mask"].unsqueeze(-1)
    if "pixel_values" in kwargs and model.mask_non_image_embeddings:
        proj = proj * (kwargs["input_ids"] == image_token_id).unsqueeze(-1)
    return proj


class ColPali(PaliGemmaPreTrainedModel):
    """PaliGemma backbone; the image token id is `config.image_token_index`."""

    def __init__(self, config, mask_non_image_embeddings=False):
        super().__init__(config)
        self.model = PaliGemmaModel(config)
        self.custom_text_proj = torch.nn.Linear(config.text_config.hidden_size, EMBED_DIM)
        self.mask_non_image_embeddings = mask_non_image_embeddings
        self.post_init()

    def get_input_embeddings(self):
        return self.model.get_input_embeddings()

    def forward(self, *args, **kwargs):
        if "pixel_values" in kwargs:
            kwargs["pixel_values"] = kwargs["pixel_values"].to(dtype=self.dtype)
        out = self.model(*args, **kwargs, use_cache=False, return_dict=True)
        return _embedding_tail(self, out.last_hidden_state, kwargs, self.config.image_token_index)


class ColQwen2(Qwen2VLPreTrainedModel):
    """Qwen2-VL backbone.  `pixel_values` arrive padded per image to a common patch count, as a batching processor hands them over; the
    forward keeps each image's t*h*w patches (image_grid_thw) before the backbone sees them."""

    def __init__(self, config, mask_non_image_embeddings=False):
        super().__init__(config)
        self.model = Qwen2VLModel(config)
        self.custom_text_proj = torch.nn.Linear(config.text_config.hidden_size, EMBED_DIM)
        self.mask_non_image_embeddings = mask_non_image_embeddings
        self.post_init()

    def get_input_embeddings(self):
        return self.model.get_input_embeddings()

    def forward(self, *args, **kwargs):
        call = dict(kwargs)
        if "pixel_values" in call:
            n_patches = call["image_grid_thw"].prod(dim=1).tolist()
            call["pixel_values"] = torch.cat([pv[:n] for pv, n in zip(call["pixel_values"], n_patches)], dim=0)
        out = self.model(*args, **call, use_cache=False, return_dict=True)
        return _embedding_tail(self, out.last_hidden_state, kwargs, self.config.image_token_id)


for _cls in (ColPali, ColQwen2):
    _cls.__module__ = MODULE_NAME
sys.modules.setdefault(MODULE_NAME, sys.modules[__name__])
