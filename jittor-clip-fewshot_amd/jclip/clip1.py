"""``jclip.clip1``: ``load_vlp`` -- the shallow-VPT model variant (reference jclip/clip1.py:189-213,
jclip/model1.py): same loader as ``jclip.clip.load`` plus 4 learnable visual prompt tokens appended
after the patch tokens (``model.visual.VPT``, model1.py:160-164,192-194)."""
from __future__ import annotations

from .clip import _load, available_models, load, tokenize  # noqa: F401

__all__ = ["available_models", "load", "load_vlp", "tokenize"]

DESIGN_DETAILS = {"trainer": "IVLP", "vision_depth": 3, "language_depth": 3, "vision_ctx": 4, "language_ctx": 4}


def load_vlp(name, download_root=None, mode="vit", device=None, design_details=None):
    """jclip/clip1.py:189-213.  The reference codes deep prompts but disables them (prompts_needed=0), and so does the
    default here: ``design_details`` entries override ``DESIGN_DETAILS``, and ``{"deep_prompts": True}`` turns on the
    per-block prompts of blocks 1 ... vision_depth-1 / language_depth-1 (``resblocks[i].VPT_shallow``)."""
    dd = dict(DESIGN_DETAILS)
    dd.update(design_details or {})
    return _load(name, dd, mode, device)
