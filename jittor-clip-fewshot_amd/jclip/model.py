"""CLIP model objects with the attribute surface of the reference's ``jclip/model.py`` (``CLIP``,
``VisionTransformer``, ``Transformer``, ``ResidualAttentionBlock``, ``build_model``) and, with
``design_details``, of ``jclip/model1.py`` (shallow VPT tokens, ``VisionTransformer.VPT``; with
``design_details["deep_prompts"]`` also the per-block prompts ``resblocks[i].VPT_shallow`` of
``ResidualAttentionBlock_IVLP``, which the reference codes but never enables).

These classes only HOLD parameters (device tensors, OpenAI-CLIP state-dict names) and expose the
replaceable ``resblocks[i].attn`` that ``apply_lora`` swaps.  All arithmetic runs in the HIP engine:
``encode_image`` / ``encode_text`` hand the whole tower to ``clipfs.engine`` (one C call per pass),
differentiable through ``torch.autograd`` with respect to the LoRA / prompt parameters only -- the
backbone is frozen (dgrad only), which is the reference's training regime
(mark_only_lora_as_trainable, lora_train_vlp.py:143-160).

A checkpoint without ``visual.proj`` is one of the RN50 family: ``build_model`` then builds ``ModifiedResNet``
(jclip/model_res.py), a frozen fp32 image tower run forward only by ``clipfs.resnet.ClipResNet``."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from .mha import MultiheadAttention


def _param(t: torch.Tensor) -> nn.Parameter:
    return nn.Parameter(t.contiguous(), requires_grad=False)


class LayerNorm(nn.Module):
    def __init__(self, weight: torch.Tensor, bias: torch.Tensor):
        super().__init__()
        self.weight = _param(weight)
        self.bias = _param(bias)
        self.eps = 1e-5


class Linear(nn.Module):
    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor]):
        super().__init__()
        self.weight = _param(weight)
        self.bias = _param(bias) if bias is not None else None
        self.out_features, self.in_features = weight.shape


class MLP(nn.Module):
    def __init__(self, sd: Dict[str, torch.Tensor], p: str):
        super().__init__()
        self.c_fc = Linear(sd[p + "c_fc.weight"], sd[p + "c_fc.bias"])
        self.c_proj = Linear(sd[p + "c_proj.weight"], sd[p + "c_proj.bias"])


class ResidualAttentionBlock(nn.Module):
    """jclip/model.py:42-62 (parameter holder; see module docstring)."""

    def __init__(self, sd: Dict[str, torch.Tensor], p: str, d_model: int, n_head: int, causal: bool,
                 prompt: Optional[torch.Tensor] = None):
        super().__init__()
        # deep prompt (ResidualAttentionBlock_IVLP, model1.py:64-127): replaces its rows of this block's input
        self.VPT_shallow = None if prompt is None else nn.Parameter(prompt.contiguous())
        self.attn = MultiheadAttention(d_model, n_head, sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"],
                                       sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"])
        self.ln_1 = LayerNorm(sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        self.mlp = MLP(sd, p + "mlp.")
        self.ln_2 = LayerNorm(sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
        self.causal = causal


def _deep_prompts(sd: Dict[str, torch.Tensor], prefix: str, width: int, depth: int, n_ctx: int, seed: int, device):
    """Prompts of blocks 1 ... depth-1 (block 0's rows are the embedding's VPT / ctx): the state-dict tensor
    ``{prefix}.resblocks.{i}.VPT_shallow`` when present, else normal(std 0.02) as model1.py:85-87.  A stored prompt
    of another shape (a checkpoint saved with another vision_ctx / language_ctx) is refused."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i in range(1, depth):
        key = f"{prefix}.resblocks.{i}.VPT_shallow"
        if key in sd:
            if tuple(sd[key].shape) != (n_ctx, width):
                raise ValueError(f"deep prompts: {key} has shape {tuple(sd[key].shape)}, the design details ask for "
                                 f"{(n_ctx, width)}")
            out[i] = sd[key]
        else:
            out[i] = (torch.randn(n_ctx, width, generator=g) * 0.02).to(device)
    return out


class Transformer(nn.Module):
    def __init__(self, sd: Dict[str, torch.Tensor], prefix: str, width: int, layers: int, heads: int, causal: bool,
                 prompt_depth: int = 1, prompt_rows: int = 0, prompt_tail: bool = False, prompt_seed: int = 0):
        """``prompt_depth`` > 1: blocks 1 ... depth-1 carry a deep prompt of ``prompt_rows`` rows, placed over the last rows
        of each sequence (``prompt_tail``: the vision tower's VPT rows) or over rows 1 ... prompt_rows (the text tower's
        ctx rows)."""
        super().__init__()
        self.width = width
        self.layers = layers
        self.heads = heads
        self.causal = causal
        self.prompt_depth = prompt_depth
        self.prompt_rows = prompt_rows if prompt_depth > 1 else 0
        self.prompt_tail = prompt_tail
        prompts = _deep_prompts(sd, prefix, width, prompt_depth, prompt_rows, prompt_seed,
                                sd[prefix + ".resblocks.0.ln_1.weight"].device)
        self.resblocks = nn.Sequential(*[
            ResidualAttentionBlock(sd, f"{prefix}.resblocks.{i}.", width, heads, causal, prompts.get(i))
            for i in range(layers)])


class _Conv1(nn.Module):
    def __init__(self, weight: torch.Tensor):
        super().__init__()
        self.weight = _param(weight)


class VisionTransformer(nn.Module):
    """jclip/model.py:80-126; with ``n_vpt > 0`` the shallow-VPT variant of jclip/model1.py:160-207."""

    def __init__(self, sd: Dict[str, torch.Tensor], input_resolution: int, patch_size: int, width: int, layers: int,
                 heads: int, output_dim: int, n_vpt: int = 0, prompt_depth: int = 1):
        super().__init__()
        self.input_resolution = input_resolution
        self.patch_size = patch_size
        self.output_dim = output_dim
        self.width = width
        self.conv1 = _Conv1(sd["visual.conv1.weight"])
        self.class_embedding = _param(sd["visual.class_embedding"])
        self.positional_embedding = _param(sd["visual.positional_embedding"])
        self.ln_pre = LayerNorm(sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
        self.transformer = Transformer(sd, "visual.transformer", width, layers, heads, causal=False,
                                       prompt_depth=prompt_depth, prompt_rows=n_vpt, prompt_tail=True, prompt_seed=1)
        self.ln_post = LayerNorm(sd["visual.ln_post.weight"], sd["visual.ln_post.bias"])
        self.proj = _param(sd["visual.proj"])
        if n_vpt > 0:
            if "visual.VPT" in sd:
                vpt = sd["visual.VPT"]
                # the deep prompts replace exactly the rows the VPT appended: a stored VPT of another row count would
                # put them over patch tokens
                if prompt_depth > 1 and tuple(vpt.shape) != (n_vpt, width):
                    raise ValueError(f"deep prompts: visual.VPT has shape {tuple(vpt.shape)}, vision_ctx asks for "
                                     f"{(n_vpt, width)}")
            else:  # normal_(ctx_vectors, std=0.02), model1.py:161-163
                g = torch.Generator().manual_seed(0)
                vpt = (torch.randn(n_vpt, width, generator=g) * 0.02).to(self.proj.device)
            self.VPT = nn.Parameter(vpt.contiguous())
        else:
            self.VPT = None

    @property
    def tokens(self) -> int:
        return (self.input_resolution // self.patch_size) ** 2 + 1 + (0 if self.VPT is None else self.VPT.shape[0])


class _BatchNorm(nn.Module):
    """Affine as frozen parameters, running statistics as buffers (the checkpoint's ``num_batches_tracked`` is not kept)."""

    def __init__(self, sd: Dict[str, torch.Tensor], p: str):
        super().__init__()
        self.weight = _param(sd[p + ".weight"])
        self.bias = _param(sd[p + ".bias"])
        self.register_buffer("running_mean", sd[p + ".running_mean"].contiguous())
        self.register_buffer("running_var", sd[p + ".running_var"].contiguous())
        self.eps = 1e-5


class Bottleneck(nn.Module):
    """jclip/model_res.py:84-121 (parameter holder)."""

    expansion = 4

    def __init__(self, sd: Dict[str, torch.Tensor], p: str, stride: int):
        super().__init__()
        self.stride = stride
        for i in (1, 2, 3):
            setattr(self, f"conv{i}", _Conv1(sd[f"{p}.conv{i}.weight"]))
            setattr(self, f"bn{i}", _BatchNorm(sd, f"{p}.bn{i}"))
        self.downsample = None
        if p + ".downsample.0.weight" in sd:  # children "0" (convolution) and "1" (BatchNorm); "-1" is the parameter-free pool
            self.downsample = nn.Sequential(_Conv1(sd[p + ".downsample.0.weight"]), _BatchNorm(sd, p + ".downsample.1"))


class AttentionPool2d(nn.Module):
    """jclip/model_res.py:65-82 (parameter holder; the semantics are the published ones, clipfs/resnet.py: ClipResNet)."""

    def __init__(self, sd: Dict[str, torch.Tensor], p: str, num_heads: int):
        super().__init__()
        self.positional_embedding = _param(sd[p + ".positional_embedding"])
        for name in ("k_proj", "q_proj", "v_proj", "c_proj"):
            setattr(self, name, Linear(sd[f"{p}.{name}.weight"], sd[f"{p}.{name}.bias"]))
        self.num_heads = num_heads


class ModifiedResNet(nn.Module):
    """The image tower of the RN50 family (jclip/model_res.py:123-170): every tensor under its checkpoint name, as a
    frozen parameter (running statistics: buffers), so ``CLIP.save`` / ``CLIP.load`` round-trip it.  ``forward`` hands the
    images to the HIP runner ``clipfs.resnet.ClipResNet``, which folds the BatchNorms once (rebuilt after ``CLIP.load``):
    forward only, fp32, BatchNorm on the running statistics whatever ``train()`` says -- the flagged deviations are in
    that class's docstring.  Nothing in this tower trains: ``VPT`` is None, there is no ``transformer`` to adapt."""

    is_modified_resnet = True
    VPT = None

    def __init__(self, sd: Dict[str, torch.Tensor], layers, output_dim: int, heads: int, input_resolution: int, width: int):
        super().__init__()
        self.layers = tuple(int(n) for n in layers)
        self.output_dim = output_dim
        self.input_resolution = input_resolution
        self.width = width
        self.heads = heads
        for i in (1, 2, 3):
            setattr(self, f"conv{i}", _Conv1(sd[f"visual.conv{i}.weight"]))
            setattr(self, f"bn{i}", _BatchNorm(sd, f"visual.bn{i}"))
        for li, nb in enumerate(self.layers):
            setattr(self, f"layer{li + 1}", nn.Sequential(*[
                Bottleneck(sd, f"visual.layer{li + 1}.{bi}", 2 if (bi == 0 and li > 0) else 1) for bi in range(nb)]))
        self.attnpool = AttentionPool2d(sd, "visual.attnpool", heads)
        self._runner = None

    @property
    def tokens(self) -> int:
        return (self.input_resolution // 32) ** 2 + 1

    @property
    def runner(self):
        if self._runner is None:
            from clipfs.resnet import ClipResNet
            self._runner = ClipResNet(self.state_dict(), self.conv1.weight.device)
        return self._runner

    def invalidate(self):
        """The tensors changed (``CLIP.load``): the runner's folded copies are stale."""
        self._runner = None

    @torch.no_grad()
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        return self.runner(images)

    execute = forward


class _Embedding(nn.Module):
    def __init__(self, weight: torch.Tensor):
        super().__init__()
        self.weight = _param(weight)

    @torch.no_grad()
    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        """Plain lookup (used by the prompt learner to initialise ctx, slow_pace.py:124-131)."""
        return self.weight.data[ids.to(self.weight.device).long()]

    execute = forward


class CLIP(nn.Module):
    """jclip/model.py:129-232."""

    def __init__(self, sd: Dict[str, torch.Tensor], embed_dim: int, image_resolution: int, vision_layers: int,
                 vision_width: int, vision_patch_size: int, context_length: int, vocab_size: int,
                 transformer_width: int, transformer_heads: int, transformer_layers: int, design_details=None):
        super().__init__()
        self.context_length = context_length
        self.vocab_size = vocab_size
        self.embed_dim = embed_dim
        n_vpt = int(design_details["vision_ctx"]) if design_details else 0
        if isinstance(vision_layers, (tuple, list)):  # jclip/model_res.py:227-235
            if n_vpt > 0 or (design_details and design_details.get("deep_prompts", False)
                             and int(design_details.get("vision_depth", 1)) > 1):
                raise ValueError("the image tower of this checkpoint is a ModifiedResNet (RN50 family): it has no token "
                                 "sequence for visual prompts -- pass design_details with vision_ctx=0 (and vision_depth=1)")
            _, t_depth, n_txt = _prompt_depths(design_details, 0, 1, transformer_layers)
            self.visual = ModifiedResNet(sd, vision_layers, embed_dim, vision_width * 32 // 64, image_resolution,
                                         vision_width)
        else:
            v_depth, t_depth, n_txt = _prompt_depths(design_details, n_vpt, vision_layers, transformer_layers)
            self.visual = VisionTransformer(sd, image_resolution, vision_patch_size, vision_width, vision_layers,
                                            vision_width // 64, embed_dim, n_vpt, v_depth)
        self.transformer = Transformer(sd, "transformer", transformer_width, transformer_layers, transformer_heads,
                                       causal=True, prompt_depth=t_depth, prompt_rows=n_txt, prompt_seed=2)
        self.token_embedding = _Embedding(sd["token_embedding.weight"])
        self.positional_embedding = _param(sd["positional_embedding"])
        self.ln_final = LayerNorm(sd["ln_final.weight"], sd["ln_final.bias"])
        self.text_projection = _param(sd["text_projection"])
        self.logit_scale = _param(sd["logit_scale"].reshape(()))
        self._engine = None

    # -- reference surface ---------------------------------------------------------------------
    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    @property
    def device(self):
        return self.visual.conv1.weight.device

    # -- Jittor Module.save / Module.load (slow_pace.py:1711, test.py:1820) -----------------------------------------
    def save(self, path: str) -> None:
        """``clip_model.save('test_pkl/clip_model.pkl')``: every parameter under its dotted name (with adapters:
        ``...attn.q_proj.weight`` / ``.bias`` / ``.w_lora_A`` / ``.w_lora_B`` ..., as the reference's module tree)."""
        from clipfs import module_io
        module_io.save_module(self, path)

    def load(self, path: str) -> None:
        from clipfs import module_io
        self.invalidate_engine()  # merged-weight copies (merge_lora) go first: the adapters are about to change
        module_io.load_module(self, path)
        if hasattr(self.visual, "invalidate"):
            self.visual.invalidate()  # a ModifiedResNet's runner holds BatchNorm-folded copies
        self.invalidate_engine()  # transposed / 16-bit weight copies of the engine are stale now

    def invalidate_engine(self):
        """Called when the module tree changes (apply_lora, FlatTrainables) so pointers are re-collected.  The
        engine's user-visible settings (precision mode, text trimming) carry over to the rebuilt engine.  Merged-weight
        copies (``lora_train_vlp.merge_lora``) live in the engine and go with it: the model is unmerged afterwards."""
        if self._engine is not None:
            self._engine_opts = (self._engine.precision, self._engine.trim_text, self._engine.sparse_backward,
                                 self._engine.prune_backward)
            if self._engine.merged:  # the merged-weight copies go with the engine: the model is unmerged again
                for m in self.modules():
                    if getattr(m, "merged", False):
                        m.merged = False
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            from clipfs.engine import Engine
            self._engine = Engine(self)
            opts = getattr(self, "_engine_opts", None)
            if opts is not None:
                (self._engine.precision, self._engine.trim_text, self._engine.sparse_backward,
                 self._engine.prune_backward) = opts
        return self._engine

    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        from clipfs.engine import encode_image
        return encode_image(self, image)

    def encode_image_tokens(self, image: torch.Tensor, with_class: bool = False):
        from clipfs.engine import encode_image_tokens
        return encode_image_tokens(self, image, with_class)

    def encode_text(self, text: torch.Tensor) -> torch.Tensor:
        from clipfs.engine import encode_text
        return encode_text(self, text)

    def forward(self, image, text):
        """CLIP.execute, jclip/model.py:217-232."""
        from clipfs.engine import clip_logits
        return clip_logits(self, image, text)

    execute = forward

    def cuda(self, device=None):  # tensors are created on the target device by build_model
        return self


def _prompt_depths(design_details, n_vpt: int, vision_layers: int, text_layers: int):
    """(vision depth, text depth, text prompt rows) of the deep prompts.  Off (depth 1 both) unless
    ``design_details["deep_prompts"]`` is true; then ``vision_depth`` / ``language_depth`` (1 ... layers; 1 = none).  The
    reference hard-codes 4 prompt rows per block (model1.py:80-83); here the rows are ``vision_ctx`` / ``language_ctx``
    (identical with the default 4)."""
    if not design_details or not design_details.get("deep_prompts", False):
        return 1, 1, 0
    v_depth = int(design_details.get("vision_depth", 1))
    t_depth = int(design_details.get("language_depth", 1))
    n_txt = int(design_details.get("language_ctx", 0))
    for name, depth, layers in (("vision_depth", v_depth, vision_layers), ("language_depth", t_depth, text_layers)):
        if not 1 <= depth <= layers:
            raise ValueError(f"deep prompts: {name} {depth} outside [1, {layers}]")
    if v_depth > 1 and n_vpt <= 0:
        raise ValueError("deep vision prompts replace the shallow VPT rows: they need vision_ctx > 0")
    if t_depth > 1 and n_txt <= 0:
        raise ValueError("deep text prompts replace the ctx rows 1 ... language_ctx: they need language_ctx > 0")
    return v_depth, t_depth, n_txt


def _infer(sd: Dict[str, torch.Tensor]):
    """Hyper-parameters from tensor shapes, jclip/model.py:235-274; a checkpoint without ``visual.proj`` is a
    ModifiedResNet (jclip/model_res.py:316-331): ``vision_layers`` is then the tuple of blocks per stage."""
    if "visual.proj" in sd:
        vision_width = sd["visual.conv1.weight"].shape[0]
        vision_layers = len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
        vision_patch_size = sd["visual.conv1.weight"].shape[-1]
        grid_size = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
        image_resolution = vision_patch_size * grid_size
    else:
        if "visual.layer1.0.conv1.weight" not in sd or "visual.attnpool.positional_embedding" not in sd:
            raise NotImplementedError("the checkpoint holds neither a ViT (visual.proj) nor a ModifiedResNet "
                                      "(visual.layer1.0.conv1.weight, visual.attnpool.positional_embedding) image tower")
        vision_layers = tuple(len({k.split(".")[2] for k in sd if k.startswith(f"visual.layer{b}.")}) for b in (1, 2, 3, 4))
        vision_width = sd["visual.layer1.0.conv1.weight"].shape[0]
        grid_size = round((sd["visual.attnpool.positional_embedding"].shape[0] - 1) ** 0.5)
        vision_patch_size = None
        image_resolution = grid_size * 32
    embed_dim = sd["text_projection"].shape[1]
    context_length = sd["positional_embedding"].shape[0]
    vocab_size = sd["token_embedding.weight"].shape[0]
    transformer_width = sd["ln_final.weight"].shape[0]
    transformer_heads = transformer_width // 64
    transformer_layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks")})
    return dict(embed_dim=embed_dim, image_resolution=image_resolution, vision_layers=vision_layers,
                vision_width=vision_width, vision_patch_size=vision_patch_size, context_length=context_length,
                vocab_size=vocab_size, transformer_width=transformer_width, transformer_heads=transformer_heads,
                transformer_layers=transformer_layers)


def build_model(state_dict: dict, design_details=None, device=None) -> CLIP:
    """jclip/model.py:235-285 (and model1.py:322-374 with ``design_details``).  ``state_dict`` values may be
    numpy arrays (a Jittor-saved pkl read by clipfs.safe_pkl) or torch tensors; they are moved to
    ``device`` (default cuda:0) as fp32.  The engine has no CPU path: a missing GPU raises."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("jclip needs an MI355X: the HIP engine has no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    sd = {}
    for k, v in state_dict.items():
        if k in ("input_resolution", "context_length", "vocab_size"):
            continue
        if k.endswith("num_batches_tracked"):  # BatchNorm's int64 counter (ModifiedResNet checkpoints): not a weight
            continue
        t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else torch.as_tensor(v)
        sd[k] = t.detach().to(device=device, dtype=torch.float32).contiguous()
    model = CLIP(sd, design_details=design_details, **_infer(sd))
    return model.eval()
