"""Adapter API of the reference's ``lora_train_vlp.py`` on the HIP engine: same names, argument
meaning and error behaviour, different machinery.

    apply_lora / get_lora_parameters / mark_only_lora_as_trainable / lora_state_dict /
    save_lora / load_lora        lora_train_vlp.py:122-179,516-635
    LoRALayer / LinearLoRA / PlainMultiheadAttentionLoRA      :185-306,377-513
    cls_acc / clip_classifier / encode_text_in_batches / solve_mta   :638-666,742-811,907-919
    LoRATrainer.step             the body of run_lora's loop, :956-1002 (+ AdamW :946)

What changes underneath: the q/k/v adapters of one attention block live in ONE stacked pair
(A [3r, d], B [3d, r]; ``q_proj.w_lora_A`` etc. are views), the low-rank update is applied in rank-r form
inside the QKV GEMM epilogue instead of materialising B@A (:218-221,302), and all trainable tensors of a
model are re-homed into one flat fp32 buffer so the data-parallel gradient exchange is a single
all-reduce and the optimiser a single fused launch."""
from __future__ import annotations

import contextlib
import math
import numbers
import os
import pickle
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from clipfs import ops, safe_pkl
from jclip import clip

INDEX_POSITIONS_TEXT = {
    'top1': [11], 'top2': [10, 11], 'top3': [9, 10, 11], 'bottom': [0, 1, 2, 3], 'mid': [4, 5, 6, 7],
    'up': [8, 9, 10, 11], 'half-up': [6, 7, 8, 9, 10, 11], 'half-bottom': [0, 1, 2, 3, 4, 5],
    'all': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]}

INDEX_POSITIONS_VISION = {
    'ViT-B/16': {'top': [11], 'top3': [9, 10, 11], 'bottom': [0, 1, 2, 3], 'mid': [4, 5, 6, 7], 'up': [8, 9, 10, 11],
                 'half-up': [6, 7, 8, 9, 10, 11], 'half-bottom': [0, 1, 2, 3, 4, 5],
                 'all': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]},
    'ViT-B/32': {'bottom': [0, 1, 2, 3], 'mid': [4, 5, 6, 7], 'up': [8, 9, 10, 11], 'half-up': [6, 7, 8, 9, 10, 11],
                 'half-bottom': [0, 1, 2, 3, 4, 5], 'all': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]},
    # reference quirk kept: 'all' stops at block 20 of 24 (lora_train_vlp.py:62)
    'ViT-L/14': {'bottom': [0, 1, 2, 3], 'mid': [4, 5, 6, 7], 'up': [8, 9, 10, 11], 'half-up': [6, 7, 8, 9, 10, 11],
                 'half-bottom': [0, 1, 2, 3, 4, 5], 'all': list(range(21))},
}

_PROJ_BIT = {'q': 1, 'k': 2, 'v': 4, 'o': 8}
_PROJ_NAME = {'q': 'q_proj', 'k': 'k_proj', 'v': 'v_proj', 'o': 'proj'}
# the MLP linears of a block (jclip/model.py:34-39): tokens of ``args.params`` = attribute names of ``block.mlp``
_MLP_TOKENS = ('c_fc', 'c_proj')
_MLP_BIT = {'c_fc': 16, 'c_proj': 32}


# ----------------------------------------------------------------------------------------------
# parameter filters (lora_train_vlp.py:122-179)
# ----------------------------------------------------------------------------------------------

def get_lora_parameters(model, bias='none'):
    params = []
    named = dict(model.named_parameters())
    for name, param in named.items():
        if bias == 'none':
            if 'lora_' in name:
                params.append(param)
        elif bias == 'all':
            if 'lora_' in name or 'bias' in name:
                params.append(param)
        elif bias == 'lora_only':
            if 'lora_' in name:
                params.append(param)
                bias_name = name.split('lora_')[0] + 'bias'
                if bias_name in named:
                    params.append(named[bias_name])
        else:
            raise NotImplementedError
    return params


def mark_only_lora_as_trainable(model, bias: str = 'none') -> None:
    """lora_train_vlp.py:143-160: freeze everything whose name has no ``lora_``; ``bias='all'`` re-enables every
    parameter named ``*bias*``, ``'lora_only'`` the bias of each LoRA-wrapped linear, anything else raises
    NotImplementedError.  The flags are set exactly as the reference sets them (so ``get_lora_parameters`` /
    optimiser parameter lists come out the same).  ``LoRATrainer`` trains exactly the biases flagged here (see
    ``trainable_biases``): the fused backward writes their gradients into the flat buffer next to the adapters', and the
    autograd route (``encode_image`` / ``encode_text``) returns them in ``param.grad``.  (The reference's own loop
    never trains a bias: its optimiser is built from ``get_lora_parameters(model)``, lora_train_vlp.py:946, and
    ``p.requires_grad_ = True`` at :151,:157 assigns an attribute instead of calling the method.)"""
    for n, p in model.named_parameters():
        if 'lora_' not in n:
            p.requires_grad_(False)
    if bias == 'none':
        return
    if bias == 'all':
        for n, p in model.named_parameters():
            if 'bias' in n:
                p.requires_grad_(True)
    elif bias == 'lora_only':
        for m in model.modules():
            if isinstance(m, LoRALayer) and getattr(m, 'bias', None) is not None:
                m.bias.requires_grad_(True)
    else:
        raise NotImplementedError


def lora_state_dict(model, bias: str = 'none'):
    sd = model.state_dict()
    if bias == 'none':
        return {k: sd[k] for k in sd if 'lora_' in k}
    if bias == 'all':
        return {k: sd[k] for k in sd if 'lora_' in k or 'bias' in k}
    if bias == 'lora_only':
        out = {}
        for k in sd:
            if 'lora_' in k:
                out[k] = sd[k]
                bn = k.split('lora_')[0] + 'bias'
                if bn in sd:
                    out[bn] = sd[bn]
        return out
    raise NotImplementedError


# ----------------------------------------------------------------------------------------------
# LoRA layers
# ----------------------------------------------------------------------------------------------

class LoRALayer:
    """lora_train_vlp.py:185-245 (state only).  Training always runs the additive form, the branch the reference
    executes in train mode.  ``merged`` is the reference's flag with a narrower trigger: it is True
    exactly while ``merge_lora`` has folded this layer's adapter into a COPY of its weight (``merged_lora`` /
    ``evaluate_lora(merged=True)``), never because of ``eval()``; ``weight`` itself is never written, so
    ``unmerge_lora`` restores the model bit for bit (the reference's ``sub_lora_data``, :236-245, subtracts in fp32)."""

    def __init__(self, r: int, lora_alpha: int, fan_in_fan_out: bool = False, dropout_rate: float = 0):
        self.r = r
        self.lora_alpha = lora_alpha
        self.dropout_rate = dropout_rate
        if self.r > 0:
            self.scaling = self.lora_alpha / math.sqrt(self.r)  # :197 -- alpha / sqrt(r), not alpha / r
        self.merged = False
        self.fan_in_fan_out = fan_in_fan_out
        self.params_with_lora = {}
        self._merge_owner = None  # the CLIP model whose ``merge_lora`` set ``merged`` (a weak reference)


class LinearLoRA(nn.Module, LoRALayer):
    """One adapted projection (lora_train_vlp.py:248-306).  ``weight`` / ``bias`` / ``w_lora_A`` /
    ``w_lora_B`` are views into the owning attention block's stacked tensors."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], a_view: torch.Tensor, b_view: torch.Tensor,
                 r: int, lora_alpha: int, dropout_rate: float):
        nn.Module.__init__(self)
        LoRALayer.__init__(self, r=r, lora_alpha=lora_alpha, dropout_rate=dropout_rate)
        self.weight = nn.Parameter(weight, requires_grad=False)
        self.bias = nn.Parameter(bias, requires_grad=False) if bias is not None else None
        self.out_features, self.in_features = weight.shape
        self.params_with_lora = {'weight': 'w'}
        self.w_lora_A = nn.Parameter(a_view)
        self.w_lora_B = nn.Parameter(b_view)

    def merge_BA(self, param_name: str = 'weight') -> torch.Tensor:
        """B @ A (:218-221); host-side helper for inspection (``merge_lora`` folds on the GPU, clipfs_lora_merge)."""
        return (self.w_lora_B.data @ self.w_lora_A.data).reshape(self.weight.shape)


def mlp_lora_linear(linear, r: int, lora_alpha: int, dropout_rate: float, gen: torch.Generator) -> LinearLoRA:
    """``LinearLoRA`` over one MLP linear (``mlp.c_fc``: d -> 4d, ``mlp.c_proj``: 4d -> d), sharing its weight and bias
    storage.  A [r, in] ~ U(+-1/sqrt(in_features)), B [out, r] = 0 (lora_train_vlp.py:209-213).  Unlike the attention
    projections' views these adapters own their tensors; their gradient slots are ``w_lora_A.grad_slot`` /
    ``w_lora_B.grad_slot`` (views of the flat gradient buffer once ``FlatTrainables`` has re-homed them)."""
    out_f, in_f = linear.weight.shape
    dev = linear.weight.device
    a = ((torch.rand(r, in_f, generator=gen) * 2 - 1) / math.sqrt(in_f)).to(dev)
    m = LinearLoRA(linear.weight.data, None if linear.bias is None else linear.bias.data, a,
                   torch.zeros(out_f, r, device=dev), r, lora_alpha, dropout_rate)
    if linear.bias is not None:
        m.bias.requires_grad_(linear.bias.requires_grad)
    m.is_mlp_lora = True
    for p in (m.w_lora_A, m.w_lora_B):
        p.grad_slot = torch.zeros_like(p.data)
    return m


def mlp_adapters(blk) -> List[Tuple[str, LinearLoRA]]:
    """[(token, LinearLoRA)] of the adapted MLP linears of one block, c_fc before c_proj."""
    return [(tok, getattr(blk.mlp, tok)) for tok in _MLP_TOKENS
            if getattr(getattr(blk.mlp, tok), 'is_mlp_lora', False) and getattr(blk.mlp, tok).r > 0]


class _FrozenLinear(nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)
        self.bias = nn.Parameter(bias, requires_grad=False) if bias is not None else None
        self.out_features, self.in_features = weight.shape


class PlainMultiheadAttentionLoRA(nn.Module, LoRALayer):
    """lora_train_vlp.py:377-513.  Splits the packed in-projection into q/k/v views (rows [0:d], [d:2d],
    [2d:3d], :395-409) WITHOUT copying -- the stacked tensor stays the GEMM operand -- and attaches
    LoRA pairs to the projections named in ``enable_lora``."""

    is_lora_mha = True

    def __init__(self, existing_mha, enable_lora: Sequence[str] = ('q', 'k', 'v', 'o'), r: int = 0, lora_alpha: int = 1,
                 dropout_rate: float = 0., seed: Optional[int] = None, **kwargs):
        nn.Module.__init__(self)
        LoRALayer.__init__(self, r=r, lora_alpha=lora_alpha, dropout_rate=dropout_rate)
        self.dropout = 0
        self.embed_dim = d = existing_mha.embed_dim
        self.kdim, self.vdim = existing_mha.kdim, existing_mha.vdim
        self._qkv_same_embed_dim = existing_mha._qkv_same_embed_dim
        self.num_heads = existing_mha.num_heads
        self.batch_first = existing_mha.batch_first
        self.head_dim = existing_mha.head_dim
        dev = existing_mha.in_proj_weight.device
        # stacked base weights (shared storage with the module being replaced)
        self.qkv_weight = existing_mha.in_proj_weight.data
        self.qkv_bias = existing_mha.in_proj_bias.data
        self._o_w = existing_mha.out_proj.weight.data
        self._o_b = existing_mha.out_proj.bias.data
        self.enable_lora = list(enable_lora)
        self.lora_mask = 0
        for item in self.enable_lora:
            if item not in _PROJ_BIT:
                raise ValueError(f"unknown projection {item!r} (expected q, k, v, o)")
            self.lora_mask |= _PROJ_BIT[item]
        if r <= 0:
            self.lora_mask = 0
        # stacked adapter storage; A ~ kaiming_uniform(a=sqrt(5)) == U(+-1/sqrt(in)), B = 0  (:209-213)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(torch.initial_seed() if seed is None else seed)
        rr = max(r, 1)
        bound = 1.0 / math.sqrt(d)

        def init_a(rows):
            return ((torch.rand(rows, d, generator=gen) * 2 - 1) * bound).to(dev)

        self.lora_A_qkv = torch.zeros(3 * rr, d, device=dev)
        self.lora_B_qkv = torch.zeros(3 * d, rr, device=dev)
        self.grad_A_qkv = torch.zeros_like(self.lora_A_qkv)
        self.grad_B_qkv = torch.zeros_like(self.lora_B_qkv)
        self.lora_A_o = torch.zeros(rr, d, device=dev)
        self.lora_B_o = torch.zeros(d, rr, device=dev)
        self.grad_A_o = torch.zeros_like(self.lora_A_o)
        self.grad_B_o = torch.zeros_like(self.lora_B_o)
        for s, item in enumerate(('q', 'k', 'v')):
            if self.lora_mask & _PROJ_BIT[item]:
                self.lora_A_qkv[s * rr:(s + 1) * rr] = init_a(rr)
        if self.lora_mask & 8:
            self.lora_A_o[:] = init_a(rr)
        self._bind_views()

    def _bind_views(self):
        d, r = self.embed_dim, max(self.r, 1)
        mods = {}
        for s, (item, name) in enumerate((('q', 'q_proj'), ('k', 'k_proj'), ('v', 'v_proj'))):
            w, b = self.qkv_weight[s * d:(s + 1) * d], self.qkv_bias[s * d:(s + 1) * d]
            if self.lora_mask & _PROJ_BIT[item]:
                mods[name] = LinearLoRA(w, b, self.lora_A_qkv[s * r:(s + 1) * r], self.lora_B_qkv[s * d:(s + 1) * d],
                                        self.r, self.lora_alpha, self.dropout_rate)
            else:
                mods[name] = _FrozenLinear(w, b)
        ow, ob = self._o_w, self._o_b
        if self.lora_mask & 8:
            mods['proj'] = LinearLoRA(ow, ob, self.lora_A_o, self.lora_B_o, self.r, self.lora_alpha, self.dropout_rate)
        else:
            mods['proj'] = _FrozenLinear(ow, ob)
        for k, m in mods.items():
            old = getattr(self, k, None)
            if isinstance(old, LinearLoRA) and isinstance(m, LinearLoRA):
                m.w_lora_A.requires_grad_(old.w_lora_A.requires_grad)
                m.w_lora_B.requires_grad_(old.w_lora_B.requires_grad)
            if old is not None and old.bias is not None and m.bias is not None:
                m.bias.requires_grad_(old.bias.requires_grad)  # a bias flagged trainable stays flagged
            setattr(self, k, m)

    # -- engine hooks -------------------------------------------------------------------------------
    def stacked(self):
        """[(name, param tensor, grad tensor)] of the stacked trainables of this block."""
        out = []
        if self.lora_mask & 7:
            out += [("lora_A_qkv", self.lora_A_qkv, self.grad_A_qkv), ("lora_B_qkv", self.lora_B_qkv, self.grad_B_qkv)]
        if self.lora_mask & 8:
            out += [("lora_A_o", self.lora_A_o, self.grad_A_o), ("lora_B_o", self.lora_B_o, self.grad_B_o)]
        return out

    def rebind(self, name: str, param: torch.Tensor, grad: torch.Tensor):
        """Move one stacked tensor into externally owned storage (flat buffer) and refresh the views."""
        setattr(self, name, param)
        setattr(self, "grad_" + name[len("lora_"):], grad)
        self._bind_views()

    def trainable_pairs(self):
        d, r = self.embed_dim, max(self.r, 1)
        out = []
        for s, (item, name) in enumerate((('q', 'q_proj'), ('k', 'k_proj'), ('v', 'v_proj'))):
            if self.lora_mask & _PROJ_BIT[item]:
                m = getattr(self, name)
                out.append((m.w_lora_A, self.grad_A_qkv[s * r:(s + 1) * r]))
                out.append((m.w_lora_B, self.grad_B_qkv[s * d:(s + 1) * d]))
        if self.lora_mask & 8:
            out.append((self.proj.w_lora_A, self.grad_A_o))
            out.append((self.proj.w_lora_B, self.grad_B_o))
        return out

    @torch.no_grad()
    def forward(self, query, key=None, value=None, need_weights=False, attn_mask=None, **_):
        """Direct call of one adapted attention block (lora_train_vlp.py:431-513): [L, N, d] in, ([L, N, d], None)
        out, causal iff an ``attn_mask`` is given -- the same kernels the fused tower sequences (rank-r LoRA down
        projection with the Philox dropout of train mode, QKV GEMM with the LoRA up-projection in its epilogue,
        attention, output projection).  Inference only, like ``jclip.mha.MultiheadAttention.forward``: training
        differentiates through ``encode_image`` / ``encode_text`` (the tower), not through single blocks."""
        if need_weights:
            raise NotImplementedError("attention weights are never materialised (need_weights=False only)")
        L, N, d = query.shape
        if attn_mask is not None:
            # the kernels implement exactly one mask: the causal -inf-above-the-diagonal mask of the text tower
            # (jclip/model.py:189-193); anything else would be applied silently wrong
            am = torch.as_tensor(attn_mask)
            causal = torch.full((L, L), float("-inf"), device=am.device, dtype=torch.float32).triu_(1)
            if tuple(am.shape) != (L, L) or not torch.equal(am.float(), causal):
                raise NotImplementedError("attn_mask must be the causal mask (-inf above the diagonal, 0 elsewhere)")
        r = self.r
        x = query.permute(1, 0, 2).reshape(N * L, d).contiguous().float()
        p = float(self.dropout_rate) if self.training else 0.0
        seed = 0
        if p > 0:
            self._direct_calls = getattr(self, "_direct_calls", 0) + 1
            seed = (0x9E3779B97F4A7C15 * self._direct_calls + 0x5EED) & 0xFFFFFFFFFFFFFFFF or 1
        qkv_mask = self.lora_mask & 7
        if qkv_mask and r > 0:
            t = ops.lora_down(x, self.lora_A_qkv, r, 3, seg_mask=qkv_mask, p=p, seed=seed, stream_base=0)
            qkv = ops.gemm_nt(x, self.qkv_weight, bias=self.qkv_bias, lora_t=t, lora_b=self.lora_B_qkv, lora_seg_width=d,
                              lora_scale=float(self.scaling))
        else:
            qkv = ops.gemm_nt(x, self.qkv_weight, bias=self.qkv_bias)
        o = ops.attention_fwd(qkv, N, L, self.num_heads, attn_mask is not None)
        if (self.lora_mask & 8) and r > 0:
            t = ops.lora_down(o, self.lora_A_o, r, 1, p=p, seed=seed, stream_base=3)
            y = ops.gemm_nt(o, self._o_w, bias=self._o_b, lora_t=t, lora_b=self.lora_B_o, lora_seg_width=d,
                            lora_scale=float(self.scaling))
        else:
            y = ops.gemm_nt(o, self._o_w, bias=self._o_b)
        return y.reshape(N, L, d).permute(1, 0, 2).contiguous(), None

    execute = forward


def apply_lora(args, clip_model):
    """lora_train_vlp.py:516-548: text blocks first, then vision blocks; a block is adapted when its
    ``attn`` is (still) a ``MultiheadAttention``.

    ``args.params`` takes ``c_fc`` and ``c_proj`` beside ``q k v o``: the selected blocks' ``mlp.c_fc`` / ``mlp.c_proj`` are
    wrapped in ``LinearLoRA`` (parameters ``...mlp.c_fc.w_lora_A`` and so on).  The list still holds one entry per adapted
    block, the block's ``PlainMultiheadAttentionLoRA`` -- also for a block adapted in its MLP only, whose attention module
    then carries no adapter (``lora_mask`` 0); the entry's ``c_fc`` / ``c_proj`` attributes are the wrapped MLP linears."""
    list_lora_layers = []
    for tok in args.params:
        if tok not in _PROJ_BIT and tok not in _MLP_TOKENS:
            raise ValueError(f"unknown projection {tok!r} (expected q, k, v, o, c_fc, c_proj)")
    attn_tokens = [tok for tok in args.params if tok in _PROJ_BIT]
    mlp_tokens = [tok for tok in _MLP_TOKENS if tok in args.params]
    gen = torch.Generator(device="cpu")
    gen.manual_seed(torch.initial_seed())

    def adapt(blocks, indices):
        for i, block in enumerate(blocks):
            if i in indices:
                sub = block.attn
                if sub.__class__.__name__ == 'MultiheadAttention':
                    new = PlainMultiheadAttentionLoRA(sub, enable_lora=attn_tokens, r=args.r, lora_alpha=args.alpha,
                                                      dropout_rate=args.dropout_rate)
                    block.attn = new
                    if args.r > 0:
                        for tok in mlp_tokens:
                            lin = mlp_lora_linear(getattr(block.mlp, tok), args.r, args.alpha, args.dropout_rate, gen)
                            setattr(block.mlp, tok, lin)
                            # reachable from the list entry without registering the module a second time
                            object.__setattr__(new, tok, lin)
                    list_lora_layers.append(new)

    if args.encoder in ('vision', 'both') and getattr(clip_model.visual, "transformer", None) is None:
        raise ValueError(f"encoder={args.encoder!r}: the image tower is a ModifiedResNet (RN50 family), which has no "
                         "transformer blocks to adapt -- pass encoder='text'")
    if args.encoder == 'text' or args.encoder == 'both':
        adapt(clip_model.transformer.resblocks, INDEX_POSITIONS_TEXT[args.position])
    if args.encoder == 'vision' or args.encoder == 'both':
        adapt(clip_model.visual.transformer.resblocks, INDEX_POSITIONS_VISION[args.backbone][args.position])
    clip_model.invalidate_engine()
    return list_lora_layers


# ----------------------------------------------------------------------------------------------
# checkpoint schema (lora_train_vlp.py:551-635)
# ----------------------------------------------------------------------------------------------

def _layer_weights(args, layer) -> dict:
    out = {}
    for p in ('q', 'k', 'v', 'o'):
        if p in args.params:
            m = getattr(layer, _PROJ_NAME[p])
            out[_PROJ_NAME[p]] = {'w_lora_A': m.w_lora_A.detach().cpu().numpy().copy(),
                                  'w_lora_B': m.w_lora_B.detach().cpu().numpy().copy()}
    for tok in _MLP_TOKENS:  # the MLP adapters, under their own token
        if tok in args.params and getattr(layer, tok, None) is not None:
            m = getattr(layer, tok)
            out[tok] = {'w_lora_A': m.w_lora_A.detach().cpu().numpy().copy(),
                        'w_lora_B': m.w_lora_B.detach().cpu().numpy().copy()}
    return out


def save_lora(args, epoch, list_lora_layers, save_path: str = 'lora_weights1/lora_weights.pkl'):
    """Same schema and default path as the reference (:551-593); a plain pickle of numpy arrays, which is
    what ``jt.save`` writes, so either side can read the other's file."""
    weights = {f'layer_{i}': _layer_weights(args, layer) for i, layer in enumerate(list_lora_layers)}
    metadata = {'r': args.r, 'alpha': args.alpha, 'encoder': args.encoder, 'params': args.params,
                'position': args.position}
    os.makedirs(os.path.dirname(save_path) or '.', exist_ok=True)
    with open(save_path, 'wb') as f:
        pickle.dump({'weights': weights, 'metadata': metadata}, f, protocol=4)
    print(f'LoRA weights saved to {save_path}')


def load_lora(args, list_lora_layers, load_path):
    """:596-635 -- FileNotFoundError when missing, ValueError on any metadata mismatch.  The file is read
    with the inert reader (clipfs.safe_pkl): nothing in it is executed."""
    if not os.path.exists(load_path):
        raise FileNotFoundError(f'File {load_path} does not exist.')
    loaded = safe_pkl.load(load_path)
    md = loaded['metadata']
    if md['r'] != args.r:
        raise ValueError(f"r mismatch: expected {args.r}, found {md['r']}")
    if md['alpha'] != args.alpha:
        raise ValueError(f"alpha mismatch: expected {args.alpha}, found {md['alpha']}")
    if md['encoder'] != args.encoder:
        raise ValueError(f"Encoder mismatch: expected {args.encoder}, found {md['encoder']}")
    if list(md['params']) != list(args.params):
        raise ValueError(f"Params mismatch: expected {args.params}, found {md['params']}")
    if md['position'] != args.position:
        raise ValueError(f"Position mismatch: expected {args.position}, found {md['position']}")
    weights = loaded['weights']
    _unmerge_layers(list_lora_layers)  # merged copies (merge_lora) of the values about to change are dropped first
    with torch.no_grad():
        for i, layer in enumerate(list_lora_layers):
            lw = weights[f'layer_{i}']
            for p in ('q', 'k', 'v', 'o'):
                name = _PROJ_NAME[p]
                if p in args.params and name in lw:
                    m = getattr(layer, name)
                    m.w_lora_A.data.copy_(torch.from_numpy(np.ascontiguousarray(lw[name]['w_lora_A'])))
                    m.w_lora_B.data.copy_(torch.from_numpy(np.ascontiguousarray(lw[name]['w_lora_B'])))
            for tok in _MLP_TOKENS:
                m = getattr(layer, tok, None)
                if tok in args.params and tok in lw and m is not None:
                    m.w_lora_A.data.copy_(torch.from_numpy(np.ascontiguousarray(lw[tok]['w_lora_A'])))
                    m.w_lora_B.data.copy_(torch.from_numpy(np.ascontiguousarray(lw[tok]['w_lora_B'])))
    print(f'LoRA weights loaded from {load_path}')


# ----------------------------------------------------------------------------------------------
# merged-weight evaluation and export (LoRALayer.merge_BA / add_lora_data / sub_lora_data / lora_train, :218-245)
# ----------------------------------------------------------------------------------------------

def _lora_layers(clip_model) -> List[LoRALayer]:
    return [m for m in clip_model.modules() if isinstance(m, LoRALayer)]


def is_merged(clip_model) -> bool:
    """Whether ``merge_lora`` is in effect (no engine is built to answer)."""
    eng = getattr(clip_model, '_engine', None)
    return eng is not None and eng.merged


def merge_lora(clip_model) -> int:
    """Fold every adapter of both towers (attention q / k / v / o, MLP c_fc / c_proj; a ModifiedResNet model: the text
    tower) into COPIES of the weights, W + scaling * B A, with one clipfs_lora_merge launch per tower, and run every
    later forward on them: the towers then see a model without adapters, so an MLP adapter no longer costs the live-row
    text forward, the one-row last block or the fp16 storage mode.  The master weights and the adapters are only read.
    Sets ``merged`` on every ``LoRALayer`` and returns the number of projections folded; called again it refreshes the
    copies from the current adapter values; a model without adapters returns 0 and changes nothing.  While merged the
    model is forward-only and dropout-free: the autograd route, the trainers and a train-mode forward with adapter
    dropout raise ValueError (``unmerge_lora``)."""
    n = clip_model.engine.merge()
    if n:
        owner = weakref.ref(clip_model)
        for m in _lora_layers(clip_model):
            m.merged, m._merge_owner = True, owner
    return n


def unmerge_lora(clip_model) -> None:
    """Drop the merged copies and clear the flags.  The master weights were never written: the model is bit for bit the
    one before ``merge_lora``."""
    eng = getattr(clip_model, '_engine', None)
    if eng is not None:
        eng.unmerge()
    for m in _lora_layers(clip_model):
        m.merged, m._merge_owner = False, None


def _unmerge_layers(list_lora_layers) -> None:
    """``unmerge_lora`` of the model(s) the given layers were merged in: the writers of adapter values call this first, so
    a stale merged copy can never be evaluated."""
    for layer in list_lora_layers:
        owner = getattr(layer, '_merge_owner', None)
        model = owner() if (owner is not None and getattr(layer, 'merged', False)) else None
        if model is not None:
            unmerge_lora(model)


@contextlib.contextmanager
def merged_lora(clip_model):
    """``with merged_lora(model): ...`` evaluates on merged weights and restores the previous state on exit (also on an
    exception): unmerged again, or, inside an outer merge, merged afresh."""
    was = is_merged(clip_model)
    merge_lora(clip_model)
    try:
        yield clip_model
    finally:
        if was:
            merge_lora(clip_model)
        else:
            unmerge_lora(clip_model)


def merged_state_dict(clip_model, prompt_ctx=None) -> Dict[str, torch.Tensor]:
    """The model as a PLAIN CLIP checkpoint: CPU fp32 tensors under the keys ``jclip.model.build_model`` reads
    (``...attn.in_proj_weight``, ``...attn.out_proj.weight``, ``...mlp.c_fc.weight``, ...), adapters folded in
    (clipfs_lora_merge, the weights ``merge_lora`` evaluates on), current biases, no ``lora`` key.  The model's merge state
    is left as found.  Learned prompts have no place in a plain checkpoint: a model with VPT tokens or deep prompts, or
    a ``prompt_ctx``, is refused by name."""
    if prompt_ctx is not None:
        raise ValueError("merged_state_dict: prompt ctx tokens cannot be stored in a plain CLIP checkpoint")
    if getattr(clip_model.visual, 'VPT', None) is not None:
        raise ValueError("merged_state_dict: the model has VPT tokens (visual.VPT), which a plain CLIP checkpoint cannot hold")
    for tname, tower in towers(clip_model):
        if any(getattr(blk, 'VPT_shallow', None) is not None for blk in tower.resblocks):
            raise ValueError(f"merged_state_dict: the {tname} tower has deep prompts (VPT_shallow), which a plain CLIP "
                             "checkpoint cannot hold")
    eng = clip_model.engine
    was = eng.merged
    eng.merge()  # engine state only: the LoRALayer flags keep saying what the caller set
    try:
        sd = {}
        for name, t in clip_model.state_dict().items():
            if 'lora_' in name or '.attn.q_proj.' in name or '.attn.k_proj.' in name or '.attn.v_proj.' in name \
                    or '.attn.proj.' in name:
                continue
            sd[name] = t
        rts = {'text': eng.txt} if eng.resnet else {'text': eng.txt, 'vision': eng.vis}
        for tname, tower in towers(clip_model):
            prefix = 'transformer' if tname == 'text' else 'visual.transformer'
            folded = rts[tname]._merged or {}
            for i, blk in enumerate(tower.resblocks):
                a, f, p = blk.attn, folded.get(i, {}), f'{prefix}.resblocks.{i}.'
                if getattr(a, 'is_lora_mha', False):
                    sd[p + 'attn.in_proj_weight'] = f.get('qkv', a.qkv_weight)
                    sd[p + 'attn.in_proj_bias'] = a.qkv_bias
                    sd[p + 'attn.out_proj.weight'] = f.get('o', a.proj.weight.data)
                    sd[p + 'attn.out_proj.bias'] = a.proj.bias.data
                if 'fc' in f:
                    sd[p + 'mlp.c_fc.weight'] = f['fc']
                if 'pr' in f:
                    sd[p + 'mlp.c_proj.weight'] = f['pr']
        return {k: v.detach().to(device='cpu', dtype=torch.float32).contiguous().clone() for k, v in sd.items()}
    finally:
        if not was:
            eng.unmerge()


# ----------------------------------------------------------------------------------------------
# evaluation helpers (lora_train_vlp.py:638-666,742-811,907-919)
# ----------------------------------------------------------------------------------------------

def cls_acc(output, target, topk=1):
    """:638-644 (top-k on the GPU; ties resolved towards the smaller class index)."""
    pred = ops.topk(output.contiguous().float(), topk).long()
    correct = pred.eq(target.to(pred.device).view(-1, 1).expand_as(pred))
    return 100.0 * float(correct.float().sum().item()) / target.shape[0]


def encode_text_in_batches(clip_model, texts, batch_size=32):
    """:907-919 -- the DIFFERENTIABLE text path of the training loop (called at :975 under
    ``clip_model.train()``; the text-tower LoRA is trained through it), so no ``no_grad`` here:
    ``encode_text`` decides by ``requires_grad``.  Captions are independent rows, so the engine encodes
    them in one pass; ``batch_size`` is accepted for signature compatibility."""
    if len(texts) == 0:
        raise ValueError("No embeddings were generated. Please check your batch processing.")
    return clip_model.encode_text(clip.tokenize(list(texts)))


@torch.no_grad()
def clip_classifier(templates_dict, clip_model):
    """:647-666: per class, encode every template, L2-normalise, mean, L2-normalise -> [1, C, d]
    (one batched text pass instead of one launch chain per template)."""
    cats = list(templates_dict.keys())
    counts = {len(templates_dict[c]) for c in cats}
    if len(counts) != 1:
        raise ValueError("every class must have the same number of templates")
    t = counts.pop()
    texts = [tpl for c in cats for tpl in templates_dict[c]]
    emb = clip_model.encode_text(clip.tokenize(texts))
    w = ops.class_mean_fwd(emb.contiguous(), len(cats), t)  # [C, d]
    return w.unsqueeze(0)  # [1, C, d] like the reference's jt.stack(..., dim=1); callers .squeeze(0).t()


@torch.no_grad()
def solve_mta(image_features, text_features):
    """:742-811: image_features [V, d] unit rows (row 0 = centre view), text_features [d, C]
    -> ``mode @ text * 100`` [1, C].  One kernel, no host sync."""
    text = text_features.t().contiguous().float()
    _, logits = ops.mta(image_features.contiguous().float().unsqueeze(0), text, want_mode=False)
    return logits


@torch.no_grad()
def evaluate_views(clip_model, views, target, textual_features):
    """The per-batch body of evaluate_lora (:823-841) for ``n_img`` images at once: ``views`` [n_img, V, 3, R, R]
    (view 0 = the centre view, the rest the random crops the loader stacks behind it), ``target`` [n_img],
    ``textual_features`` [d, C] unit columns.  ONE image-tower pass over all n_img * V views, one MTA launch.
    Returns the number of correct top-1 predictions (mta, centre view, view ensemble)."""
    n_img, V = views.shape[:2]
    text_cd = textual_features.t().contiguous().float()
    feats = ops.l2norm_fwd(clip_model.encode_image(views.reshape(n_img * V, *views.shape[2:])).contiguous())
    fv = feats.reshape(n_img, V, -1)
    _, mta = ops.mta(fv, text_cd, want_mode=False)                       # solve_mta(...) = 100 * mode @ text  (:834)
    base = ops.gemm_nt(fv[:, 0].contiguous(), text_cd)                   # image_features[0] @ textual_features (:835)
    ens = ops.gemm_nt(fv.mean(dim=1).contiguous(), text_cd)              # (features @ text).mean(0) = mean(features) @ text (:837)
    tgt = target.to(mta.device).long().view(-1)
    return tuple(int((ops.topk(x.contiguous(), 1).long().view(-1) == tgt).sum().item()) for x in (mta, base, ens))


@torch.no_grad()
def evaluate_lora(args, clip_model, loader, templates=None, textual_features=None, merged: bool = False):
    """lora_train_vlp.py:813-846: MTA / centre-view / view-ensemble top-1 accuracy (in %) over a loader that yields
    ``(image [n,1,3,R,R] | [n,3,R,R], images [n,1,N,3,R,R] | [n,N,3,R,R], target, impath)`` -- the centre view and the N
    random crops of each image.  The text classifier comes from ``templates`` ({class: [captions]}, the reference reads
    them from the 'text_template' folder, :816-817) or is passed in as ``textual_features`` [d, C].  ``merged=True``
    evaluates under ``merged_lora``: the adapters folded into copies of the weights (what the reference's eval mode
    does in place, :236-245), the model's merge state left as found."""
    if merged:
        with merged_lora(clip_model):
            return evaluate_lora(args, clip_model, loader, templates, textual_features)
    clip_model.eval()
    if textual_features is None:
        if templates is None:
            raise ValueError("evaluate_lora needs `templates` ({class: [captions]}) or `textual_features` [d, C]")
        textual_features = clip_classifier(templates, clip_model).squeeze(0).t()
    dev = clip_model.device
    acc = acc1 = acc2 = 0
    tot = 0
    for batch in loader:
        image, images, target = batch[0], batch[1], batch[2]
        image = torch.as_tensor(image).to(dev).float()
        images = torch.as_tensor(images).to(dev).float()
        if image.dim() == 5:
            image = image.squeeze(1)                                     # :826
        if images.dim() == 6:
            images = images.squeeze(1)                                   # :827
        if images.dim() == 4:                                            # the reference's batch-size-1 loader: [N,3,R,R]
            images = images.unsqueeze(0)
        views = torch.cat([image.unsqueeze(1), images], dim=1)           # jt.concat((image, images)), per image (:829)
        target = torch.as_tensor(target).view(-1)
        c = evaluate_views(clip_model, views, target, textual_features)
        acc, acc1, acc2 = acc + c[0], acc1 + c[1], acc2 + c[2]
        tot += views.shape[0]
    if tot == 0:
        raise ValueError("evaluate_lora: the loader yielded no images")
    return 100.0 * acc / tot, 100.0 * acc1 / tot, 100.0 * acc2 / tot


@torch.no_grad()
def evaluate_retrieval(model, images, captions, image_groups=None, caption_groups=None, ks=(1, 5, 10)):
    """Recall@k of image -> text and text -> image retrieval over ``images`` [B, 3, R, R] and ``captions`` [M, 77]: a
    query is a hit at k when ANY of its positives (the rows of the other side whose group equals its own; with both
    groups None, M == B and row i pairs with row i) is among its k best matches (ties to the lower index, ``ops.topk``).
    Returns {"i2t": {k: recall}, "t2i": {k: recall}} as fractions of B and of M (k is capped at the other side's size).
    Synchronises (it returns Python floats)."""
    eng = model.engine
    dev = model.device
    B, M = images.shape[0], captions.shape[0]
    if (image_groups is None) != (caption_groups is None):
        raise ValueError("evaluate_retrieval needs both image_groups and caption_groups, or neither")
    if image_groups is None:
        if B != M:
            raise ValueError(f"evaluate_retrieval without groups pairs image i with caption i: {B} images, {M} captions")
        image_groups = caption_groups = torch.arange(B)
    ig, cg = image_groups.to(dev).long(), caption_groups.to(dev).long()
    feat, _ = eng.vit_forward(images.to(dev), False, 0)
    emb, _ = eng.text_forward(captions, None, False, 0)
    img, txt = ops.l2norm_fwd(feat), ops.class_mean_fwd(emb, M, 1)
    out = {}
    for name, q, k, qg, kg in (("i2t", img, txt, ig, cg), ("t2i", txt, img, cg, ig)):
        n = k.shape[0]
        top = ops.topk(ops.gemm_nt(q, k, alpha=100.0), min(max(ks), n)).long()
        hit = (kg[top] == qg[:, None]) & (qg[:, None] >= 0)
        out[name] = {kk: int(hit[:, :min(kk, n)].any(dim=1).sum()) / q.shape[0] for kk in ks}
    return out


# ----------------------------------------------------------------------------------------------
# flat trainable buffer + stage-1 step (lora_train_vlp.py:946,956-1002)
# ----------------------------------------------------------------------------------------------

def towers(model) -> List[Tuple[str, nn.Module]]:
    """(name, transformer) of the towers that have blocks to adapt: text, then vision.  A ModifiedResNet image tower
    (RN50 family) has no transformer and is left out: nothing of it trains."""
    vt = getattr(model.visual, "transformer", None)
    return [("text", model.transformer)] + ([] if vt is None else [("vision", vt)])


def trainable_biases(model) -> List[Tuple[str, nn.Parameter]]:
    """(name, parameter) of the biases ``LoRATrainer`` trains: exactly those with ``requires_grad=True``, in
    ``model.named_parameters()`` order.  The flags come from ``mark_only_lora_as_trainable(model, bias)``:

    - 'none': no bias;
    - 'all': every bias of both towers (block LayerNorms, packed in-projection or its q / k / v views, out projection,
      c_fc, c_proj) plus ``visual.ln_pre`` / ``visual.ln_post`` / ``ln_final``;
    - 'lora_only': the biases of the LoRA-wrapped linears (``q_proj.bias`` ... ``proj.bias`` of the enabled projections).

    The 'lora_only' rule deliberately follows the FLAGS, not ``get_lora_parameters(model, 'lora_only')``: the reference's
    filter builds the bias name as ``name.split('lora_')[0] + 'bias'`` = ``...q_proj.w_bias`` (the adapter is called
    ``w_lora_A``), finds no such parameter and so hands the optimiser no bias at all -- kept as it is in
    ``get_lora_parameters`` (reference-faithful), not repeated here.

    The VPT tokens and the deep prompts (``resblocks.{i}.VPT_shallow``) are trained too, but are not biases: they are left
    out here (``FlatTrainables`` places them).  Any other CLIP parameter flagged trainable (a weight, an embedding, a
    LayerNorm gain) has no gradient in the fused backward: ValueError naming it, instead of silently leaving it
    untouched."""
    from clipfs.engine import image_biases, text_biases
    known = {id(p) for p in image_biases(model) + text_biases(model) if p is not None}
    out, bad = [], []
    for n, p in model.named_parameters():
        if not p.requires_grad or 'lora_' in n:
            continue
        if id(p) in known:
            out.append((n, p))
        elif n != 'visual.VPT' and not n.endswith('.VPT_shallow'):  # VPT: an extra tensor (LoRATrainer); deep prompts
            bad.append(n)
    if bad:
        raise ValueError("the fused backward computes gradients for LoRA adapters, prompt / VPT tokens and biases only; "
                         f"these parameters are flagged trainable but would never be updated: {', '.join(bad)}")
    return out


def trainable_deep_prompts(model) -> List[nn.Parameter]:
    """The deep prompts (``resblocks.{i}.VPT_shallow``) with ``requires_grad``: text tower, then vision, block order."""
    from clipfs.engine import deep_prompts
    return [p for _, tower in towers(model) for p in deep_prompts(tower) if p.requires_grad]


class FlatTrainables:
    """Re-homes every stacked LoRA tensor (text blocks, then vision blocks: apply_lora order), the
    optional prompt / VPT tokens and the trainable biases (``trainable_biases``) into ONE contiguous fp32 buffer
    with matching gradient and AdamW moment buffers: a single RCCL all-reduce and a single optimiser launch per step.

    Trainable deep prompts (``resblocks.{i}.VPT_shallow`` with ``requires_grad``; text tower, then vision, block order)
    follow the extra tensors, and biases go last, so with neither flagged the buffer is exactly what it was without
    them.  A deep prompt becomes a view of the buffer with ``grad_slot`` the matching gradient view, as a bias does.  Each trainable bias parameter
    becomes a view of the buffer (``state_dict`` returns the trained values) with ``grad_slot`` the matching view of the
    gradient buffer.  The packed in-projection bias the QKV GEMM reads: when all three q / k / v views of a LoRA block
    train, their slices are adjacent and the packed tensor IS that 3d slice; when only some do (``lora_only`` with
    ``params=['q', 'v']``), the trained segments get their own slices and ``sync_packed`` copies them into the packed
    tensor (3d floats per block) -- a frozen segment is never in the buffer, so AdamW's weight decay cannot touch it.

    Adapters frozen with ``requires_grad_(False)`` are left out the same way (all or nothing per block, as the fused
    backward sees them: ``clipfs.engine._lora_trains``): they keep their own storage, get no gradient slot and are never
    moved by AdamW (the stage-2 layout, slow_pace.py:1556-1564: LoRA applied but frozen)."""

    def __init__(self, model, extra: Sequence[nn.Parameter] = ()):
        from clipfs.engine import _lora_trains, _mlp_lora_trains
        if is_merged(model):  # re-homing the adapters rebuilds the engine, which would silently drop the merged copies
            raise ValueError("the LoRA adapters are merged into the weights (merge_lora), which is forward-only -- call "
                             "unmerge_lora before building a trainer")
        self.model = model
        bias_names = [n for n, _ in trainable_biases(model)]
        entries = []
        mlp_params = []  # trainable MLP adapters (mlp.c_fc / mlp.c_proj): A then B, after the attention adapters
        labels = []      # one name per segment of the buffer, in buffer order (``segments``)
        mlp_labels = []
        for tname, tower in towers(model):
            for i, blk in enumerate(tower.resblocks):
                a = blk.attn
                if getattr(a, "is_lora_mha", False) and _lora_trains(a, f"{tname} block {i}"):
                    for name, p, _ in a.stacked():
                        entries.append((a, name, p))
                        labels.append(f"{tname}.{i}.attn.{name}/mask{a.lora_mask}")
                for tok, m in mlp_adapters(blk):
                    if _mlp_lora_trains(m, f"{tname} block {i} mlp.{tok}"):
                        mlp_params += [m.w_lora_A, m.w_lora_B]
                        mlp_labels += [f"{tname}.{i}.mlp.{tok}.w_lora_A", f"{tname}.{i}.mlp.{tok}.w_lora_B"]
        n_bias = sum(p.numel() for _, p in trainable_biases(model))
        deep = trainable_deep_prompts(model)
        n = (sum(p.numel() for _, _, p in entries) + sum(p.numel() for p in mlp_params) + sum(p.numel() for p in extra)
             + sum(p.numel() for p in deep) + n_bias)
        if n == 0:
            raise ValueError("model has nothing to train: no trainable adapter, bias or extra tensor (call apply_lora first)")
        dev = model.device
        self.params = torch.zeros(n, device=dev)
        self.grads = torch.zeros(n, device=dev)
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        off = 0
        for a, name, p in entries:
            k = p.numel()
            self.params[off:off + k].copy_(p.reshape(-1))
            a.rebind(name, self.params[off:off + k].view_as(p), self.grads[off:off + k].view_as(p))
            off += k
        self.mlp_params = mlp_params
        for p in mlp_params:  # (none without c_fc / c_proj in apply_lora's params: the layout is then unchanged)
            k = p.numel()
            self.params[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.params[off:off + k].view_as(p)
            p.grad_slot = self.grads[off:off + k].view_as(p)
            off += k
        self.extra = []
        for p in extra:
            k = p.numel()
            self.params[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.params[off:off + k].view_as(p)
            p.grad_slot = self.grads[off:off + k].view_as(p)
            self.extra.append(p)
            off += k
        self.deep_prompts = deep
        for p in deep:
            k = p.numel()
            self.params[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.params[off:off + k].view_as(p)
            p.grad_slot = self.grads[off:off + k].view_as(p)
            off += k
        # biases (after the LoRA rebinds above: those rebuild the q / k / v / proj modules, flags carried over)
        named = dict(model.named_parameters())
        self.bias_names = bias_names
        self.bias_offset = off
        self._packed_dst, self._packed_src = [], []
        owner = {}  # id(q/k/v_proj.bias) -> (attention block, segment)
        for _, tower in towers(model):
            for blk in tower.resblocks:
                a = blk.attn
                if getattr(a, "is_lora_mha", False):
                    for s, nm in enumerate(("q_proj", "k_proj", "v_proj")):
                        owner[id(getattr(a, nm).bias)] = (a, s)
        seg_off = {}  # attention block -> {segment: offset of its slice}
        for name in bias_names:
            p = named[name]
            k = p.numel()
            view = self.params[off:off + k].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad_slot = self.grads[off:off + k].view_as(p)
            if id(p) in owner:
                a, s = owner[id(p)]
                seg_off.setdefault(a, {})[s] = off
            off += k
        for _, tower in towers(model):
            for blk in tower.resblocks:
                a = blk.attn
                if getattr(a, "is_lora_mha", False) and a.proj.bias.requires_grad:
                    a._o_b = a.proj.bias.data  # the direct (single-block) forward reads the same storage
        for a, segs in seg_off.items():
            d = a.embed_dim
            if len(segs) == 3 and segs[1] == segs[0] + d and segs[2] == segs[0] + 2 * d:
                # adjacent in the buffer (named_parameters order q, k, v): the packed bias becomes that slice
                a.qkv_bias = self.params[segs[0]:segs[0] + 3 * d]
            else:
                for s, o in segs.items():
                    self._packed_dst.append(a.qkv_bias[s * d:(s + 1) * d])
                    self._packed_src.append(self.params[o:o + d])
        assert off == n
        self.numel = n
        # ordered (name, size) of every segment: the layout fingerprint a saved optimiser state is checked against
        sizes = ([p.numel() for _, _, p in entries] + [p.numel() for p in mlp_params] + [p.numel() for p in extra]
                 + [p.numel() for p in deep] + [named[nm].numel() for nm in bias_names])
        labels += mlp_labels + [f"extra.{j}" for j in range(len(self.extra))] + [f"deep_prompt.{j}" for j in range(len(deep))]
        labels += [f"bias.{nm}" for nm in bias_names]
        self.segments = [(nm, int(k)) for nm, k in zip(labels, sizes)]
        assert len(labels) == len(sizes) and sum(sizes) == n
        self.sync_packed()
        model.invalidate_engine()

    def sync_packed(self):
        """Copy the trained q / k / v bias segments into the packed in-projection biases of the blocks where only some of
        the three train (nothing to do otherwise)."""
        if self._packed_dst:
            with torch.no_grad():
                torch._foreach_copy_(self._packed_dst, self._packed_src)

    def zero_grad(self):
        self.grads.zero_()


def _check_loss_scale(loss_scale, init_scale, growth_factor, backoff_factor, growth_interval):
    """Validate the loss-scaling arguments of ``LoRATrainer``; returns None (off), 'static' or 'dynamic'."""
    if loss_scale is None:
        return None
    if isinstance(loss_scale, str):
        if loss_scale != "dynamic":
            raise ValueError(f"loss_scale must be None, a positive number or 'dynamic', not {loss_scale!r}")
        if not (math.isfinite(init_scale) and init_scale > 0):
            raise ValueError(f"init_scale must be a positive finite number, not {init_scale!r}")
        if not (math.isfinite(growth_factor) and growth_factor > 1):
            raise ValueError(f"growth_factor must be > 1, not {growth_factor!r}")
        if not 0 < backoff_factor < 1:
            raise ValueError(f"backoff_factor must lie in (0, 1), not {backoff_factor!r}")
        if int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError(f"growth_interval must be a positive integer, not {growth_interval!r}")
        return "dynamic"
    if isinstance(loss_scale, bool) or not isinstance(loss_scale, numbers.Real) or not math.isfinite(loss_scale) \
            or loss_scale <= 0:
        raise ValueError(f"loss_scale must be None, a positive number or 'dynamic', not {loss_scale!r}")
    return "static"


def _check_step_options(max_grad_norm, ema_decay):
    """Validate the clipping / EMA arguments of the trainers (None = off)."""
    for name, x in (("max_grad_norm", max_grad_norm), ("ema_decay", ema_decay)):
        if x is not None and (isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(x)):
            raise ValueError(f"{name} must be None or a finite number, not {x!r}")
    if max_grad_norm is not None and not 0 < max_grad_norm <= float(np.finfo(np.float32).max):
        raise ValueError(f"max_grad_norm must be None or a positive number that fp32 holds, not {max_grad_norm!r}")
    if ema_decay is not None and not (0 < float(np.float32(ema_decay)) < 1):
        raise ValueError(f"ema_decay must be None or lie in (0, 1) as an fp32 number, not {ema_decay!r}")


class FlatStepTrainer:
    """Base of the trainers that step ONE flat buffer (``LoRATrainer``, ``slow_pace.FusedStage2Trainer``): everything
    around the forward / backward that does not depend on the objective.

    Contract.  A subclass's ``__init__`` (explicit arguments, no ``**kwargs``) first validates with ``_check_loss_scale``
    and ``_check_step_options`` -- before it touches the model -- then sets ``self.model`` (a model with an ``engine``),
    builds ``self.flat`` (``FlatTrainables``) and, if it has one, ``self.sched`` (a scheduler with ``step()`` and
    ``base_lr`` / ``T_max`` / ``eta_min`` / ``last_epoch``), and then calls ``_init_flat_step`` once, with its
    collective counts per step (class-sharded text tower, replicated).  It implements ``_after_update`` (what
    follows the AdamW launch) and its own ``forward_backward`` / ``step``, which call ``_refuse_sharded_dropout``.

    The base then guarantees: the hyper-parameters ``lr`` / ``wd`` / ``betas`` / ``eps`` and the call counter ``t``; the
    data-parallel attributes ``pg`` / ``rank`` / ``world`` / ``live`` / ``shard_text`` / ``collectives_per_step``, the
    exchange buffers, the side stream and the collective timers (``time_collectives``, ``collective_times_ms``);
    ``overlap_towers`` and ``last_plan``; the loss-scaling state (``loss_scaling``, ``scale_state``, ``_scaler_rule``) with
    its host views ``loss_scale_value`` / ``skipped_steps`` / ``optimizer_steps``; the clipping and EMA state below;
    ``optimizer_step`` (shadow refusal, all-reduce when ``live``, ``t += 1``, ``_apply_update``, ``_after_update``); and
    ``state_dict`` / ``load_state_dict`` over all of it.  A subclass with state of its own does not override those two:
    it implements ``_own_state`` / ``_check_own_state`` / ``_load_own_state`` (all three do nothing here).

    Loss scaling (``loss_scale`` ...): see ``LoRATrainer``.  ``scale_state`` is the device record (clipfs.h
    CLIPFS_SCALER_*), None = off; ``_scaler_rule`` the scaler's constants (growth, backoff, interval).

    ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_``'s rule on the UNSCALED gradient, on the device: after the
    all-reduce (every rank forms the same norm from the same bytes: no new collective) and after the scaler's decision,
    two more launches (sum of squares, decision) and the multiplier folded into AdamW's gradient scale: 1 -> 3 launches
    per optimiser step, 3 -> 5 with loss scaling, no host synchronisation.  ``last_grad_norm`` / ``last_clip_coef`` read
    the device record back (they synchronise; ``step`` never uses them).  A non-finite norm without loss scaling gives
    a coefficient of 0 and a poisoned update, as torch with ``error_if_nonfinite=False``: ``loss_scale`` skips such steps.

    ``ema_decay``: a flat fp32 shadow beside ``flat.m`` / ``flat.v``, set to the parameters at construction (the
    reference's ``EMA.register``, lora_train_vlp.py:870-904) and updated inside the AdamW launch
    (``shadow = decay * shadow + (1 - decay) * param``, :887); a skipped step leaves it untouched.  ``apply_shadow()`` puts
    the averaged values into ``flat.params`` for evaluation and ``restore()`` brings the live ones back.

    With both None the step is the launches it was without them."""

    def _init_flat_step(self, lr, weight_decay, betas, eps, process_group, shard_text, collectives, loss_scale,
                        init_scale, growth_factor, backoff_factor, growth_interval, max_grad_norm, ema_decay):
        """Everything of the contract above; called once, after ``self.model`` and ``self.flat`` are in place.
        ``collectives``: the subclass's collectives per step, (class-sharded text tower, replicated)."""
        from clipfs import dist as D
        dev = self.flat.params.device
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.t = 0
        self.pg = process_group
        self.rank, self.world = D.world_info(process_group)
        self.shard_text = shard_text and self.live
        self.collectives_per_step = collectives[0 if self.shard_text else 1] if self.live else 0
        self.overlap_towers = True  # text tower on a side HIP stream (set False to serialise, e.g. for per-kernel timing)
        # class-sharded text tower: fixed exchange buffers (allocated on first use, never re-zeroed: padding rows of
        # the send block / the gradient table are written by nobody and stay zero)
        self._xbuf = {}
        self.last_plan = None  # gradient floors of the last forward_backward: {"text": lo or None, "vision": lo or None}
        self.time_collectives = False      # bench: bracket every collective with HIP events on the launch stream
        self._coll_events = []
        # loss scaling: the device record (clipfs.h CLIPFS_SCALER_*) and the scaler's constants; None = off
        self.loss_scaling = _check_loss_scale(loss_scale, init_scale, growth_factor, backoff_factor, growth_interval)
        self.scale_state = None
        if self.loss_scaling == "dynamic":
            self._scaler_rule = (float(growth_factor), float(backoff_factor), int(growth_interval))
            self.scale_state = ops.new_scaler_state(float(init_scale), dev)
        elif self.loss_scaling == "static":
            self._scaler_rule = (1.0, 1.0, 0)  # never grows, never backs off; still skips a non-finite step
            self.scale_state = ops.new_scaler_state(float(loss_scale), dev)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.clip_state = self._sumsq_work = self.ema_shadow = self._ema_backup = None
        if self.max_grad_norm is not None:
            self.clip_state = ops.new_clip_state(dev)
            self._sumsq_work = ops.grad_sumsq_work(self.flat.numel, dev)
        if self.ema_decay is not None:
            self.ema_shadow = self.flat.params.clone()

    @property
    def live(self) -> bool:
        """Whether the collectives run: more than one rank, or ``clipfs.dist.FORCE_COLLECTIVES`` (read at each use)."""
        from clipfs import dist as D
        return self.world > 1 or D.FORCE_COLLECTIVES

    def _refuse_sharded_dropout(self):
        """Every ``forward_backward`` calls this before it launches anything."""
        eng = self.model.engine
        if self.shard_text and eng.trim_text and self.model.training and eng.txt.lora_dropout_rate() > 0:
            # dropout masks are indexed by token row = caption * seq + position; trimming makes `seq` the local shard's
            # last EOT, so ranks would index different (and overlapping) rows than the one-process run
            raise ValueError("trim_text cannot be combined with a class-sharded text tower and LoRA dropout > 0: the "
                             "Philox rows would depend on each rank's trimmed length (use trim_text=False or shard_text=False)")

    def optimizer_step(self):
        from clipfs import dist as D
        if self.shadow_applied:
            raise RuntimeError("optimizer_step while the EMA shadow is applied: call restore() first")
        if self.live:
            # replicated text tower (shard_text=False): every rank back-propagated the text gradient of ITS images
            # only, so this same sum is already the batch total (d_txt is linear in the local dlogits)
            self._timed("all_reduce", lambda: D.allreduce_sum_(self.flat.grads, self.pg))
        self.t += 1
        self._apply_update()  # AdamW, behind the scaler's and the clip's launches when those are on
        self._after_update()

    def _after_update(self):
        """What a subclass does after the AdamW launch of ``optimizer_step``."""
        raise NotImplementedError

    # (tail_n, weight decay, lower bound, upper bound) of the flat buffer's last entries where a subclass gives them an
    # update that differs from plain AdamW (``LoRAPairTrainer``'s trained log-temperature); None: the plain launch
    tail_update = None

    def _apply_update(self):
        """The launches of one optimiser step after the all-reduce (``self.t`` already counts this step): the one AdamW
        launch, which takes every record that is on (None = off), behind the scaler's and the clip's own launches."""
        f = self.flat
        if self.scale_state is not None:
            growth, backoff, interval = self._scaler_rule
            ops.grads_nonfinite(f.grads, self.scale_state)
            ops.scaler_decide(self.scale_state, self.lr, self.betas, growth, backoff, interval)
        if self.clip_state is not None:
            ops.grad_sumsq(f.grads, self._sumsq_work)
            ops.clip_decide(self._sumsq_work, f.numel, self.max_grad_norm, self.clip_state, self.scale_state)
        if self.tail_update is None:
            ops.adamw_ext(f.params, f.grads, f.m, f.v, self.t, self.lr, self.betas, self.eps, self.wd, 1.0,
                          self.scale_state, self.clip_state, self.ema_shadow, self.ema_decay or 0.0)
        else:  # the buffer's last entries with a decay and bounds of their own: the same one launch
            tail_n, tail_wd, tail_min, tail_max = self.tail_update
            ops.adamw_tail(f.params, f.grads, f.m, f.v, self.t, self.lr, self.betas, self.eps, self.wd, 1.0,
                           self.scale_state, self.clip_state, self.ema_shadow, self.ema_decay or 0.0, tail_n=tail_n,
                           tail_weight_decay=tail_wd, tail_min=tail_min, tail_max=tail_max)

    # -- loss scaling: host views of the device record (each one synchronises) -------------------------
    def _scaler_word(self, index: int, as_int: bool):
        if self.scale_state is None:
            return None
        st = self.scale_state.cpu()
        return int(st.view(torch.int32)[index]) if as_int else float(st[index])

    @property
    def loss_scale_value(self) -> Optional[float]:
        """The scale the next ``forward_backward`` applies (None with loss scaling off)."""
        return self._scaler_word(ops._lib.SCALER_SCALE, False)

    @property
    def skipped_steps(self) -> int:
        """``optimizer_step`` calls that changed nothing because a gradient was NaN / inf (0 with loss scaling off)."""
        return self._scaler_word(ops._lib.SCALER_SKIPPED, True) or 0

    @property
    def optimizer_steps(self) -> int:
        """AdamW steps applied: ``t`` minus the skipped steps."""
        return self.t if self.scale_state is None else self._scaler_word(ops._lib.SCALER_STEP, True)

    # -- collectives ---------------------------------------------------------------------------------
    def _exchange_buffers(self, classes: int, width: int):
        from clipfs import dist as D
        key = (classes, width)
        b = self._xbuf.get(key)
        if b is None:
            s = D.block_rows(classes, self.world)
            dev = self.flat.params.device
            b = dict(S=s, send=torch.zeros(s, width, device=dev), full=torch.empty(self.world * s, width, device=dev),
                     dfull=torch.zeros(self.world * s, width, device=dev), dmine=torch.empty(s, width, device=dev))
            self._xbuf = {key: b}
        return b

    def _timed(self, name, fn):
        if not self.time_collectives:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self._coll_events.append((name, e0, e1))
        return out

    def collective_times_ms(self):
        """{name: [ms, ...]} of the collectives bracketed since the last call (needs a prior synchronize)."""
        out = {}
        for name, e0, e1 in self._coll_events:
            out.setdefault(name, []).append(e0.elapsed_time(e1))
        self._coll_events = []
        return out

    def _side_stream(self):
        # one per device for everything in the process (clipfs/streams.py: HIP maps streams onto a handful of hardware
        # queues, and a fresh stream per user ends up sharing a queue with another one)
        from clipfs import streams
        return streams.side_stream(self.model.device)

    # -- clipping: host views of the device record (each one synchronises) ----------------------------
    @property
    def last_grad_norm(self) -> Optional[float]:
        """The unscaled global 2-norm of the gradients of the last ``optimizer_step`` (None with clipping off)."""
        return None if self.clip_state is None else float(self.clip_state[ops._lib.CLIP_NORM].item())

    @property
    def last_clip_coef(self) -> Optional[float]:
        """The factor the last ``optimizer_step`` multiplied the gradients by, in (0, 1] (None with clipping off)."""
        return None if self.clip_state is None else float(self.clip_state[ops._lib.CLIP_COEF].item())

    # -- EMA: evaluation-time swaps ---------------------------------------------------------------------
    @property
    def shadow_applied(self) -> bool:
        return self._ema_backup is not None

    @torch.no_grad()
    def apply_shadow(self):
        """Put the averaged values into the flat parameter buffer (the live ones are kept for ``restore``)."""
        if self.ema_shadow is None:
            raise RuntimeError("apply_shadow needs ema_decay")
        if self._ema_backup is not None:
            raise RuntimeError("the EMA shadow is already applied: call restore() first")
        self._ema_backup = self.flat.params.clone()
        self.flat.params.copy_(self.ema_shadow)
        self.flat.sync_packed()

    @torch.no_grad()
    def restore(self):
        """Bring back the live parameters ``apply_shadow`` set aside."""
        if self._ema_backup is None:
            raise RuntimeError("restore without a preceding apply_shadow")
        self.flat.params.copy_(self._ema_backup)
        self._ema_backup = None
        self.flat.sync_packed()

    # -- resumable state ----------------------------------------------------------------------------------
    def _switches(self) -> Dict[str, bool]:
        return {"loss_scale": self.scale_state is not None, "max_grad_norm": self.clip_state is not None,
                "ema_decay": self.ema_shadow is not None}

    def state_dict(self) -> dict:
        """Everything a run needs to go on where it stopped, as CPU tensors and plain Python values (store it with
        ``torch.save``; adapter files of ``save_lora`` are another matter): the flat parameters and AdamW moments, the EMA
        shadow (and the live values set aside while it is applied), the loss-scaling and clip records, ``t``, ``lr``, the
        scheduler position (stage 2), the engine's dropout seed state, the hyper-parameters and the layout of the flat
        buffer; and what the subclass adds (``_own_state``: ``LoRATrainer``'s ``pair_loss`` and sigmoid head).
        Synchronises."""
        cpu = lambda x: None if x is None else x.detach().cpu().clone()
        eng = self.model.engine
        sched = getattr(self, "sched", None)
        return {
            **self._own_state(),
            "layout": [(n, k) for n, k in self.flat.segments],
            "switches": self._switches(),
            "params": cpu(self.flat.params), "m": cpu(self.flat.m), "v": cpu(self.flat.v),
            "ema_shadow": cpu(self.ema_shadow), "shadow_applied": self._ema_backup is not None,
            "ema_backup": cpu(self._ema_backup),
            "scale_state": cpu(self.scale_state), "clip_state": cpu(self.clip_state),
            "t": int(self.t), "lr": float(self.lr),
            "scheduler": None if sched is None else {"base_lr": sched.base_lr, "T_max": sched.T_max,
                                                     "eta_min": sched.eta_min, "last_epoch": sched.last_epoch},
            "engine": {"seed_base": int(eng.seed_base), "step": int(eng.step)},
            "hyper": {"weight_decay": float(self.wd), "betas": (float(self.betas[0]), float(self.betas[1])),
                      "eps": float(self.eps), "max_grad_norm": self.max_grad_norm, "ema_decay": self.ema_decay,
                      "loss_scaling": self.loss_scaling,
                      "scaler_rule": None if self.scale_state is None else tuple(self._scaler_rule)},
        }

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """Take back a ``state_dict()``.  The trainer must have been built like the one that wrote it: the same flat
        layout and the same of loss scaling, clipping and EMA switched on -- a ``ValueError`` names what differs and
        nothing is changed; a subclass refuses the same way what does not fit its own additions (``LoRATrainer``: a
        state written under the other ``pair_loss``).  Everything else (hyper-parameters included) is restored from
        ``sd``."""
        mine, theirs = [(n, k) for n, k in self.flat.segments], [(n, int(k)) for n, k in sd["layout"]]
        if mine != theirs:
            a, b = dict(theirs), dict(mine)
            diff = ([f"{n}: saved {a[n]} floats, this trainer {b[n]}" for n in a if n in b and a[n] != b[n]]
                    + [f"{n}: only in the saved state" for n in a if n not in b]
                    + [f"{n}: only in this trainer" for n in b if n not in a]) or ["the segments come in another order"]
            raise ValueError("the saved state belongs to another flat layout (" + "; ".join(diff[:4])
                             + (f"; and {len(diff) - 4} more" if len(diff) > 4 else "") + ")")
        sw = self._switches()
        bad = [f"{k} is {'on' if sd['switches'][k] else 'off'} in the saved state and {'on' if sw[k] else 'off'} in this "
               "trainer" for k in sw if bool(sd["switches"][k]) != sw[k]]
        if bad:
            raise ValueError("the saved state was written with other options: " + "; ".join(bad))
        sched = getattr(self, "sched", None)
        if (sched is None) != (sd["scheduler"] is None):
            raise ValueError("the saved state " + ("has no" if sched is not None else "carries a")
                             + " scheduler position: it was written by the other kind of trainer")
        self._check_own_state(sd)
        f = self.flat
        for dst, key in ((f.params, "params"), (f.m, "m"), (f.v, "v"), (self.ema_shadow, "ema_shadow"),
                         (self.scale_state, "scale_state"), (self.clip_state, "clip_state")):
            if dst is not None:
                dst.copy_(sd[key])
        self._ema_backup = sd["ema_backup"].to(f.params.device) if sd["shadow_applied"] else None
        self.t, self.lr = int(sd["t"]), float(sd["lr"])
        if sched is not None:
            s = sd["scheduler"]
            sched.base_lr, sched.T_max, sched.eta_min = float(s["base_lr"]), int(s["T_max"]), float(s["eta_min"])
            sched.last_epoch = int(s["last_epoch"])
        eng = self.model.engine
        eng.seed_base, eng.step = int(sd["engine"]["seed_base"]), int(sd["engine"]["step"])
        h = sd["hyper"]
        self.wd, self.betas, self.eps = float(h["weight_decay"]), tuple(h["betas"]), float(h["eps"])
        self.max_grad_norm, self.ema_decay, self.loss_scaling = h["max_grad_norm"], h["ema_decay"], h["loss_scaling"]
        if self.scale_state is not None:
            self._scaler_rule = tuple(h["scaler_rule"])
        self._load_own_state(sd)
        f.sync_packed()

    def _own_state(self) -> dict:
        """What a subclass's ``state_dict`` adds to the base's (plain Python values and CPU tensors)."""
        return {}

    def _check_own_state(self, sd: dict) -> None:
        """Raise ``ValueError`` where ``sd`` does not fit what the subclass added; nothing has been changed yet."""

    def _load_own_state(self, sd: dict) -> None:
        """Take back what ``_own_state`` added."""


class LoRATrainer(FlatStepTrainer):
    """One object = the state of run_lora (:921-1023) that matters for the hot path: model with adapters,
    flat trainables, AdamW moments, step counter.  ``step`` is the loop body :956-1002:

        text features of every class (with grad)  ->  per class normalise/mean/normalise
        image features of the batch               ->  normalise
        logits = 100 * img @ txt^T ; mean cross entropy ; backward into LoRA (+ prompt) ; AdamW

    Data-parallel: every rank holds the full model, takes its shard of the image batch, and the flat
    gradient buffer is summed with one all-reduce (losses are pre-scaled by B_local / B_global).

    Loss scaling (opt-in, for the fp16 storage mode whose backward keeps activation gradients as f16 images; allowed
    and harmless in the other modes).  ``loss_scale=None`` is the unscaled step, launch for launch.  A positive number is
    a static scale; ``"dynamic"`` starts at ``init_scale`` (65536), multiplies by ``growth_factor`` after
    ``growth_interval`` consecutive clean steps and by ``backoff_factor`` after a step whose gradients held NaN / inf.
    Either kind SKIPS such a step: parameters and moments stay bitwise untouched.  The logits gradient is multiplied by
    the scale on the device, ``flat.grads`` holds SCALED gradients between ``forward_backward`` and ``optimizer_step``
    (several ``forward_backward`` calls accumulate under one scale), and ``optimizer_step`` is three launches (non-finite
    check, decision, AdamW) instead of one, with no host synchronisation; under data parallelism the check runs after
    the all-reduce, so every rank takes the same decision without a further collective.  ``t`` still counts
    ``optimizer_step`` calls; with scaling on, AdamW's step number is ``optimizer_steps``, which leaves skipped steps
    out.  ``loss_scale_value`` / ``skipped_steps`` / ``optimizer_steps`` read the device record back (they synchronise;
    ``step`` never uses them).  Not covered: the autograd route of ``encode_image`` / ``encode_text`` (stage 2 scales
    through ``slow_pace.Stage2Trainer(..., fused=True)``); bias training still needs a non-fp16 mode.

    ``max_grad_norm`` / ``ema_decay`` (both off by default) and ``state_dict`` / ``load_state_dict``: see
    ``FlatStepTrainer``.

    ``pair_loss`` / ``pair_head`` / ``train_pair_head``: the objective of ``step_pairs``.  On this class they are the
    constants "infonce" / None / False: the multi-positive InfoNCE loss at the host constant ``logit_scale``.  The
    constructor of ``LoRAPairTrainer`` (below) is where they are chosen; ``state_dict`` records ``pair_loss`` and the
    head, and ``load_state_dict`` refuses a state written under the other ``pair_loss``."""

    pair_loss = "infonce"
    pair_head = None
    train_pair_head = False

    def __init__(self, model, lr: float = 2e-4, weight_decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 logit_scale: float = 100.0, prompt_ctx: Optional[nn.Parameter] = None, process_group=None,
                 shard_text: bool = True, loss_scale=None, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, init_scale: float = 65536.0, max_grad_norm: Optional[float] = None,
                 ema_decay: Optional[float] = None):
        _check_loss_scale(loss_scale, init_scale, growth_factor, backoff_factor, growth_interval)
        _check_step_options(max_grad_norm, ema_decay)
        self.model = model
        extra = []
        if prompt_ctx is not None:
            extra.append(prompt_ctx)
        if model.visual.VPT is not None and model.visual.VPT.requires_grad:
            extra.append(model.visual.VPT)
        if self.train_pair_head:  # LoRAPairTrainer: the sigmoid head, after the prompt ctx and VPT
            extra.append(self.pair_head)
        self.flat = FlatTrainables(model, extra)
        if model.engine.precision == "fp16":
            for tname, tower in towers(model):
                for i, blk in enumerate(tower.resblocks):
                    for tok, _ in mlp_adapters(blk):
                        raise ValueError(f"{tname} block {i} has a {tok} adapter: MLP adapters are not supported in the fp16 "
                                         "storage mode (LayerNorm 2's output, the activation and the MLP gradient exist only "
                                         "as f16 images there): use precision 'fp32' or 'bf16x3'")
        if self.flat.bias_names and model.engine.precision == "fp16":
            raise ValueError("bias training is not supported in the fp16 storage mode (dqkv and the MLP gradient exist "
                             "only as f16 images there): use precision 'fp32' or 'bf16x3'")
        self.prompt_ctx = prompt_ctx
        self.logit_scale = logit_scale
        self._pbuf = {}  # exchange buffers of forward_backward_pairs
        # all_gather + reduce_scatter + all_reduce, or the all_reduce alone (forward_backward recounts from text_lo)
        self._init_flat_step(lr, weight_decay, betas, eps, process_group, shard_text, (3, 1), loss_scale, init_scale,
                             growth_factor, backoff_factor, growth_interval, max_grad_norm, ema_decay)

    def forward_backward(self, images, captions, target, templates_per_class: int = 1, global_batch: Optional[int] = None,
                         row_offset: int = 0):
        """``images`` / ``target`` are THIS RANK's shard of the batch (rows ``row_offset ...`` of the global batch),
        ``captions`` the full caption table [C * t, 77] (class major).  Accumulates gradients into the flat buffer;
        returns (loss_sum_local [1], correct_local [1], logits_local [B_local, C]).

        Collectives (world > 1, class-sharded text): all_gather of the class-feature block, reduce_scatter of its
        gradient (here), all_reduce of the flat gradient (optimizer_step) -- clipfs/dist.py.

        A tower with nothing to train (gradient floor None, ``Engine.image_plan`` / ``text_plan``) runs its no-grad
        forward and gets no backward; its side of the logits gradient is not formed, and a frozen class-sharded text
        tower skips the reduce_scatter (every rank holds the same flags, so the ranks agree).  ``last_plan`` records the
        floors."""
        from clipfs import dist as D
        m = self.model
        eng = m.engine
        eng.refuse_merged("LoRATrainer.forward_backward")  # merged weights (merge_lora) are forward-only
        self.flat.sync_packed()  # packed q/k/v biases of partially trained blocks (no-op otherwise)
        seed = eng.next_seed() if m.training else 0
        B = images.shape[0]
        gb = global_batch or B * self.world
        t = templates_per_class
        classes = captions.shape[0] // t
        d = m.embed_dim
        c_lo, c_hi = D.block_bounds(classes, self.rank, self.world) if self.shard_text else (0, classes)
        self._refuse_sharded_dropout()
        xb = self._exchange_buffers(classes, d) if self.shard_text else None
        text_lo = eng.text_plan(self.prompt_ctx is not None)
        vis_lo = eng.image_plan()
        self.last_plan = {"text": text_lo, "vision": vis_lo}
        if self.live:
            self.collectives_per_step = (3 if text_lo is not None else 2) if self.shard_text else 1
        # The two towers are independent until the logits: the text tower runs on a side HIP stream so that
        # its kernels fill the CUs the image tower's launches leave idle (small per-rank batches) and vice versa.
        main = torch.cuda.current_stream()
        side = self._side_stream() if self.overlap_towers else main
        side.wait_stream(main)
        emb = tctx = txt = None
        with torch.cuda.stream(side):
            if c_hi > c_lo:
                # dropout masks are indexed by GLOBAL rows (row0): a sharded run draws the masks of the one-process run
                emb, tctx = eng.text_forward(captions[c_lo * t:c_hi * t], self.prompt_ctx, True, seed, row0=c_lo * t)
                txt = ops.class_mean_fwd(emb, c_hi - c_lo, t, out=None if xb is None else xb["send"][:c_hi - c_lo])
        feat, ictx = eng.vit_forward(images, True, seed, row0=row_offset)
        img_n, inv = ops.l2norm_fwd(feat, save_inv=True)
        main.wait_stream(side)
        if self.shard_text:
            full = self._timed("all_gather", lambda: D.allgather_blocks(xb["send"], xb["full"], self.pg))
            txt = full[:classes]
        logits = ops.gemm_nt(img_n, txt, alpha=self.logit_scale)
        self.last_features = (img_n, txt)  # unit image features of this rank's shard, unit class features [C, d] (tests)
        loss_sum, dl, correct = ops.cross_entropy(logits, target, True, grad_scale=B / gb, scale_state=self.scale_state)
        if vis_lo is not None:
            d_img_n = ops.matmul_small(dl, txt, B, d, classes, classes, 1, d, 1, self.logit_scale)
        if text_lo is not None:
            d_txt = ops.matmul_small(dl, img_n, classes, d, B, 1, classes, d, 1, self.logit_scale,
                                     out=None if xb is None else xb["dfull"][:classes])
            if self.shard_text:  # every rank needs the batch-total gradient of ITS classes only
                mine = self._timed("reduce_scatter", lambda: D.reduce_scatter_blocks(xb["dfull"], xb["dmine"], self.pg))
                d_txt_local = mine[:c_hi - c_lo]
            else:
                d_txt_local = d_txt
            side.wait_stream(main)
            with torch.cuda.stream(side):
                if c_hi > c_lo:
                    d_emb = ops.class_mean_bwd(emb, d_txt_local, c_hi - c_lo, t)
                    slot = None if self.prompt_ctx is None else self.prompt_ctx.grad_slot
                    eng.text_backward(tctx, d_emb, slot)
        if vis_lo is not None:
            eng.vit_backward(ictx, ops.l2norm_bwd(d_img_n, img_n, inv))
        main.wait_stream(side)
        return loss_sum, correct, logits

    def _after_update(self):
        self.flat.sync_packed()

    def step(self, images, captions, target, templates_per_class: int = 1, global_batch: Optional[int] = None,
             row_offset: int = 0):
        self.flat.zero_grad()
        out = self.forward_backward(images, captions, target, templates_per_class, global_batch, row_offset)
        self.optimizer_step()
        return out

    # -- contrastive (image, caption) pairs ----------------------------------------------------------------
    def _pair_buffers(self, images: int, captions: int, width: int):
        """The fixed exchange buffers of ``forward_backward_pairs`` under data parallelism, per side ("img", "cap"): the
        send block (padding rows written by nobody: they stay zero), the gathered table, its gradient table, this rank's
        block of the reduced gradient; and one int32 pair for both group vectors."""
        from clipfs import dist as D
        key = (images, captions, width)
        b = self._pbuf.get(key)
        if b is None:
            dev = self.flat.params.device
            b = {}
            for side, n in (("img", images), ("cap", captions)):
                s = D.block_rows(n, self.world)
                b[side] = dict(S=s, send=torch.zeros(s, width, device=dev), full=torch.empty(self.world * s, width, device=dev),
                               dfull=torch.empty(self.world * s, width, device=dev), dmine=torch.empty(s, width, device=dev))
            s2 = b["img"]["S"] + b["cap"]["S"]
            b["gsend"] = torch.full((1, s2), -1, device=dev, dtype=torch.int32)
            b["gfull"] = torch.empty(self.world, s2, device=dev, dtype=torch.int32)
            self._pbuf = {key: b}
        return b

    def forward_backward_pairs(self, images, captions, image_groups=None, caption_groups=None,
                               global_batch: Optional[int] = None, global_captions: Optional[int] = None,
                               row_offset: int = 0, caption_offset: int = 0):
        """CLIP's own objective over (image, caption) pairs with group ids: every caption whose group equals an image's is
        its positive (the UniCL / supervised-contrastive form), in both directions:

            loss = 1/2 ( (1/B_g) sum over images of loss_i  +  (1/M_g) sum over captions of loss_j )

        with loss_i the multi-positive InfoNCE row loss of ``ops.contrastive_objective``.  The sums are divided by the
        ROW COUNTS B_g and M_g, not by the number of rows that have a positive: the latter would need a device -> host
        read, and this method never synchronises.

        ``images`` [B, 3, R, R] and ``captions`` [M, 77] are THIS RANK's rows (``row_offset`` / ``caption_offset`` of
        the global batch of ``global_batch`` images and ``global_captions`` captions); M need not equal B (unique class
        captions, several captions per image).  ``image_groups`` [B] / ``caption_groups`` [M] are integer ids >= 0 (a
        negative id masks the row out); with both None the rows are pairs: M_g == B_g and group = global row index.
        Accumulates gradients into the flat buffer; returns (loss_sum_local [1], correct_i2t_local [1],
        correct_t2i_local [1]): this rank's share of the loss above and the local images / captions whose best match is
        a positive.

        Towers, side stream, gradient floors (``last_plan``), dropout rows by global row, loss scaling: as
        ``forward_backward``.  A tower with nothing to train gets no feature gradient formed and no backward.

        Data parallel (class-sharded text only: ``shard_text=False`` is refused): rank r holds image rows
        ``block_bounds(B_g, r, world)`` and caption rows ``block_bounds(M_g, r, world)``.  Its unit image block and unit
        caption block are all-gathered (padding rows zero, group -1), given groups are gathered as one int32 vector;
        the objective runs twice (local images x all captions, local captions x all images); the two gathered-feature
        gradient tables are reduce-scattered; ``optimizer_step`` all-reduces the flat gradient.  Collectives per step:
        2 all_gather (+ 1 with given groups) + 1 reduce_scatter per trained tower + 1 all_reduce -- 5 for plain pairs,
        6 with groups (``collectives_per_step``).

        ``pair_loss="sigmoid"``: loss = (1/B_g) sum over all live (image, caption) cells of the binary loss of
        ``ops.sigmoid_objective`` -- ONE objective call, local images x all captions, which covers every cell once.  A
        live image without a positive caption still pays its negative terms.  Returns (loss_sum_local,
        correct_i2t_local, None): a text -> image hit count would need a second walk and is not formed.  Data parallel:
        only the caption block is all-gathered (and the caption groups when given); image features and image groups
        stay local, the caption-gradient table is written afresh and reduce-scattered, and the flat all-reduce sums the
        ranks' shares of the head's gradient: 3 collectives for plain pairs, 4 with groups, one fewer with the text tower
        frozen.  Everything else is as above.

        ``pair_loss="clip"``: the first loss above at the logit scale exp(pair_head[0]), read on the device (and trained
        with ``train_pair_head``).  One process: ONE symmetric call of ``ops.clip_pairs_objective`` (four launches, one
        walk of the logits per gradient).  Data parallel: the exchange above unchanged, the two calls one-directional
        (``weight_k = 0``); the head's gradient accumulates over both and the flat all-reduce sums the ranks' shares."""
        from clipfs import dist as D
        m = self.model
        eng = m.engine
        eng.refuse_merged("LoRATrainer.forward_backward_pairs")
        live = self.live
        if live and not self.shard_text:
            raise ValueError("forward_backward_pairs: shard_text=False is not supported for pairs (every rank would encode "
                             "every caption): build the trainer with shard_text=True")
        if (image_groups is None) != (caption_groups is None):
            raise ValueError("forward_backward_pairs needs both image_groups and caption_groups, or neither")
        B, M = images.shape[0], captions.shape[0]
        Bg, Mg = global_batch or B * self.world, global_captions or M * self.world
        paired = image_groups is None
        if paired and Mg != Bg:
            raise ValueError(f"forward_backward_pairs without groups pairs image i with caption i: {Bg} images, {Mg} captions")
        b_lo, b_hi = D.block_bounds(Bg, self.rank, self.world) if live else (row_offset, row_offset + B)
        c_lo, c_hi = D.block_bounds(Mg, self.rank, self.world) if live else (caption_offset, caption_offset + M)
        if B < 1 or M < 1 or (live and (B, M, row_offset, caption_offset) != (b_hi - b_lo, c_hi - c_lo, b_lo, c_lo)):
            raise ValueError(f"forward_backward_pairs: rank {self.rank} of {self.world} takes image rows [{b_lo}, {b_hi}) and "
                             f"caption rows [{c_lo}, {c_hi}) (block_bounds, at least one of each), got {B} images at "
                             f"{row_offset} and {M} captions at {caption_offset}")
        self.flat.sync_packed()
        seed = eng.next_seed() if m.training else 0
        d = m.embed_dim
        dev = self.flat.params.device
        self._refuse_sharded_dropout()
        xb = self._pair_buffers(Bg, Mg, d) if live else None
        text_lo = eng.text_plan(self.prompt_ctx is not None)
        vis_lo = eng.image_plan()
        want_i, want_t = vis_lo is not None, text_lo is not None
        self.last_plan = {"text": text_lo, "vision": vis_lo}
        sigmoid = self.pair_loss == "sigmoid"
        if live and sigmoid:
            self.collectives_per_step = 1 + (0 if paired else 1) + int(want_t) + 1
        elif live:
            self.collectives_per_step = 2 + (0 if paired else 1) + int(want_i) + int(want_t) + 1
        main = torch.cuda.current_stream()
        side = self._side_stream() if self.overlap_towers else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            emb, tctx = eng.text_forward(captions, self.prompt_ctx, True, seed, row0=caption_offset)
            txt = ops.class_mean_fwd(emb, M, 1, out=None if xb is None else xb["cap"]["send"][:M])  # unit rows
        feat, ictx = eng.vit_forward(images, True, seed, row0=row_offset)
        img_n, inv = ops.l2norm_fwd(feat, save_inv=True, out=None if xb is None else xb["img"]["send"][:B])
        if paired:
            ig = torch.arange(row_offset, row_offset + B, device=dev, dtype=torch.int32)
            cg = torch.arange(caption_offset, caption_offset + M, device=dev, dtype=torch.int32)
        else:
            ig = image_groups.to(device=dev, dtype=torch.int32).contiguous()
            cg = caption_groups.to(device=dev, dtype=torch.int32).contiguous()
        main.wait_stream(side)
        self.last_features = (img_n, txt)
        if sigmoid:
            loss_sum, c_it, d_img_own, d_txt_all = self._sigmoid_pairs(img_n, txt, ig, cg, xb, Mg, Bg, paired, want_i, want_t)
            c_ti = None
            scatter_images = False  # the images' gradient is complete on its rank: every cell of a row was scored here
        else:
            if live:
                si, sc = xb["img"]["S"], xb["cap"]["S"]
                img_all = self._timed("all_gather", lambda: D.allgather_blocks(xb["img"]["send"], xb["img"]["full"], self.pg))
                txt_all = self._timed("all_gather", lambda: D.allgather_blocks(xb["cap"]["send"], xb["cap"]["full"], self.pg))
                if paired:  # global row g carries group g, padding rows -1: nothing to exchange
                    ig_all = torch.arange(self.world * si, device=dev, dtype=torch.int32)
                    cg_all = torch.arange(self.world * sc, device=dev, dtype=torch.int32)
                    ig_all[Bg:] = -1
                    cg_all[Mg:] = -1
                else:
                    xb["gsend"][0, :B] = ig
                    xb["gsend"][0, si:si + M] = cg
                    g_all = self._timed("all_gather", lambda: D.allgather_blocks(xb["gsend"], xb["gfull"], self.pg))
                    ig_all, cg_all = g_all[:, :si].reshape(-1), g_all[:, si:].reshape(-1)
                d_txt_all, d_img_all = (xb["cap"]["dfull"] if want_t else None), (xb["img"]["dfull"] if want_i else None)
                my_img, my_cap = self.rank * si, self.rank * sc
            else:
                img_all, txt_all, ig_all, cg_all = img_n, txt, ig, cg
                d_txt_all = torch.empty(M, d, device=dev) if want_t else None
                d_img_all = None
                my_img = my_cap = 0
            s = self.logit_scale
            if self.pair_loss == "clip":
                head = self.pair_head.data
                dhead = self.pair_head.grad_slot if self.train_pair_head else None
            if self.pair_loss == "clip" and not live:
                # ONE symmetric call: both directions' statistics, one walk of the logits per gradient
                loss_sum, _, _, hits, d_img_own, _, _ = ops.clip_pairs_objective(
                    img_n, txt, ig, cg, head, 0.5 / Bg, 0.5 / Mg, self.scale_state, dk=d_txt_all, dhead=dhead,
                    want_dq=want_i, want_dk=False, want_dhead=False, accumulate=(False, False, True))
                c_it, c_ti = hits[:1], hits[1:]
            elif self.pair_loss == "clip":
                # the exchange below, call for call, with the scale read on the device; dhead accumulates over both
                l_it, _, _, hits, d_img_own, _, _ = ops.clip_pairs_objective(
                    img_n, txt_all, ig, cg_all, head, 0.5 / Bg, 0.0, self.scale_state, dk=d_txt_all, dhead=dhead,
                    want_dq=want_i, want_dk=False, want_dhead=False, accumulate=(False, False, True))
                l_ti, _, _, hits_t, _, _, _ = ops.clip_pairs_objective(
                    txt, img_all, cg, ig_all, head, 0.5 / Mg, 0.0, self.scale_state,
                    dq=d_txt_all[my_cap:my_cap + M] if want_t else None, dk=d_img_all, dhead=dhead,
                    want_dq=False, want_dk=False, want_dhead=False, accumulate=(True, False, True))
                loss_sum, c_it, c_ti = l_it + l_ti, hits[:1], hits_t[:1]
            else:
                # local images x all captions: the images' own gradient, and the caption-gradient table written afresh
                l_it, _, c_it, d_img_own, _ = ops.contrastive_objective(img_n, txt_all, ig, cg_all, s, 0.5 / Bg,
                                                                        self.scale_state, dk=d_txt_all, want_dq=want_i,
                                                                        want_dk=False, accumulate=False)
                # local captions x all images: added into this rank's rows of the caption table; the image side is added
                # to the images' own gradient (one process) or written afresh into the image-gradient table (data parallel)
                l_ti, _, c_ti, _, _ = ops.contrastive_objective(txt, img_all, cg, ig_all, s, 0.5 / Mg, self.scale_state,
                                                                dq=d_txt_all[my_cap:my_cap + M] if want_t else None,
                                                                dk=d_img_all if live else d_img_own, want_dq=False,
                                                                want_dk=False, accumulate=(True, not live))
                loss_sum = l_it + l_ti
            scatter_images = live  # each rank holds a share of every image's gradient from the captions' direction
        if want_t:
            if live:
                mine = self._timed("reduce_scatter", lambda: D.reduce_scatter_blocks(xb["cap"]["dfull"], xb["cap"]["dmine"], self.pg))
                d_txt_local = mine[:M]
            else:
                d_txt_local = d_txt_all
            side.wait_stream(main)
            with torch.cuda.stream(side):
                d_emb = ops.class_mean_bwd(emb, d_txt_local, M, 1)
                eng.text_backward(tctx, d_emb, None if self.prompt_ctx is None else self.prompt_ctx.grad_slot)
        if want_i:
            if scatter_images:
                d_img_all[my_img:my_img + B].add_(d_img_own)
                mine = self._timed("reduce_scatter", lambda: D.reduce_scatter_blocks(xb["img"]["dfull"], xb["img"]["dmine"], self.pg))
                d_img_n = mine[:B]
            else:
                d_img_n = d_img_own
            eng.vit_backward(ictx, ops.l2norm_bwd(d_img_n.contiguous(), img_n, inv))
        main.wait_stream(side)
        return loss_sum, c_it, c_ti

    def _sigmoid_pairs(self, img_n, txt, ig, cg, xb, Mg, Bg, paired, want_i, want_t):
        """The sigmoid objective of ``forward_backward_pairs``: this rank's unit images against ALL unit captions in one
        call.  Returns (loss_sum_local, correct_i2t_local, the images' gradient or None, the caption-gradient table
        (written afresh; data parallel: the gathered table, to be reduce-scattered) or None)."""
        from clipfs import dist as D
        dev = self.flat.params.device
        M, d = txt.shape
        if self.live:
            si, sc = xb["img"]["S"], xb["cap"]["S"]
            txt_all = self._timed("all_gather", lambda: D.allgather_blocks(xb["cap"]["send"], xb["cap"]["full"], self.pg))
            if paired:  # global row g carries group g, padding rows -1: nothing to exchange
                cg_all = torch.arange(self.world * sc, device=dev, dtype=torch.int32)
                cg_all[Mg:] = -1
            else:  # the caption half of the group vector alone: image groups stay local
                xb["gsend"][0, si:si + M] = cg
                g_all = self._timed("all_gather", lambda: D.allgather_blocks(xb["gsend"], xb["gfull"], self.pg))
                cg_all = g_all[:, si:].reshape(-1)
            d_txt_all = xb["cap"]["dfull"] if want_t else None
        else:
            txt_all, cg_all = txt, cg
            d_txt_all = torch.empty(M, d, device=dev) if want_t else None
        dhead = self.pair_head.grad_slot if self.train_pair_head else None
        loss_sum, _, c_it, d_img_own, _, _ = ops.sigmoid_objective(
            img_n, txt_all, ig, cg_all, self.pair_head.data, 1.0 / Bg, self.scale_state, dk=d_txt_all, dhead=dhead,
            want_dq=want_i, want_dk=False, want_dhead=False, accumulate=(False, False, True))
        return loss_sum, c_it, d_img_own, d_txt_all

    @property
    def pair_scale_value(self) -> Optional[float]:
        """t = exp(pair_head[0]) of the sigmoid objective, s of the "clip" one (None under ``pair_loss="infonce"``).
        Synchronises."""
        return None if self.pair_head is None else float(math.exp(self.pair_head.data[0].item()))

    @property
    def pair_bias_value(self) -> Optional[float]:
        """b = pair_head[1] of the sigmoid objective (None under the other two).  Synchronises."""
        return None if self.pair_head is None or self.pair_head.numel() < 2 else float(self.pair_head.data[1].item())

    def _own_state(self) -> dict:
        """``pair_loss`` and the sigmoid head (None under "infonce"; a trained head is also part of ``params``)."""
        return {"pair_loss": self.pair_loss,
                "pair_head": None if self.pair_head is None else self.pair_head.data.detach().cpu().clone()}

    def _check_own_state(self, sd: dict) -> None:
        theirs = sd.get("pair_loss", "infonce")  # a state without the key was written before the argument existed
        if theirs != self.pair_loss:
            raise ValueError(f"the saved state was written with pair_loss={theirs!r} and this trainer was built with "
                             f"pair_loss={self.pair_loss!r}")

    def _load_own_state(self, sd: dict) -> None:
        if self.pair_head is not None and not self.train_pair_head:  # a trained head came back with ``params``
            self.pair_head.data.copy_(sd["pair_head"])

    def step_pairs(self, images, captions, image_groups=None, caption_groups=None, global_batch: Optional[int] = None,
                   global_captions: Optional[int] = None, row_offset: int = 0, caption_offset: int = 0):
        """``zero_grad``, ``forward_backward_pairs``, ``optimizer_step``: one training step on (image, caption) pairs."""
        self.flat.zero_grad()
        out = self.forward_backward_pairs(images, captions, image_groups, caption_groups, global_batch, global_captions,
                                          row_offset, caption_offset)
        self.optimizer_step()
        return out


class LoRAPairTrainer(LoRATrainer):
    """``LoRATrainer`` with the objective of ``step_pairs`` chosen at construction: the arguments ``pair_loss``,
    ``pair_scale``, ``pair_bias``, ``train_pair_head``, ``pair_scale_max`` and ``pair_head_weight_decay`` after
    ``LoRATrainer``'s own, everything else inherited
    (``LoRATrainer``'s constructor keeps its parameter list, which the suite pins).

    ``pair_loss="clip"`` is the InfoNCE loss with CLIP's own temperature: ``pair_head`` is ONE float on the device,
    log(``logit_scale``), read by ``ops.clip_pairs_objective`` (``pair_scale`` / ``pair_bias`` belong to "sigmoid" and are
    refused).  With ``train_pair_head=True`` it is trained as CLIP and OpenCLIP train it: the buffer's last entry, free of
    weight decay (``pair_head_weight_decay``: None = 0 here, the buffer's decay under "sigmoid") and clamped at
    log(``pair_scale_max``) after every update (100, CLIP's ln 100; None: no clamp; under the other two it must stay at
    its default and does nothing).  The decay and the clamp ride in the one AdamW launch (``ops.adamw_tail``), issued
    only where they differ from plain AdamW.

    ``pair_loss="infonce"`` (the default) builds exactly a ``LoRATrainer``: the same flat layout, the same launches.
    ``"sigmoid"`` is the pairwise sigmoid (SigLIP) loss of ``ops.sigmoid_objective`` with ``pair_head``, a two-float DEVICE
    parameter (log ``pair_scale``, ``pair_bias``) that the kernels read (SigLIP's initial point is t = 10, b = -10).  With
    ``train_pair_head=True`` it is the LAST extra tensor of the flat buffer (after the prompt ctx and VPT), its
    ``grad_slot`` is where the objective accumulates d loss / d (log t, b), the flat all-reduce sums the ranks' shares,
    and AdamW moves it like every other entry -- INCLUDING the buffer's uniform weight decay, which pulls log t and b
    towards 0, unless ``pair_head_weight_decay`` says otherwise.  A head that is not trained stays outside the buffer (the
    flat layout is the default trainer's) and its gradient is not formed.  ``pair_scale_value`` / ``pair_bias_value`` read
    it back (they synchronise; ``step_pairs`` never uses them)."""

    def __init__(self, model, lr: float = 2e-4, weight_decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 logit_scale: float = 100.0, prompt_ctx: Optional[nn.Parameter] = None, process_group=None,
                 shard_text: bool = True, loss_scale=None, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, init_scale: float = 65536.0, max_grad_norm: Optional[float] = None,
                 ema_decay: Optional[float] = None, pair_loss: str = "infonce", pair_scale: float = 10.0,
                 pair_bias: float = -10.0, train_pair_head: bool = False, pair_scale_max: Optional[float] = 100.0,
                 pair_head_weight_decay: Optional[float] = None):
        _check_loss_scale(loss_scale, init_scale, growth_factor, backoff_factor, growth_interval)
        _check_step_options(max_grad_norm, ema_decay)
        if pair_loss not in ("infonce", "sigmoid", "clip"):
            raise ValueError(f"pair_loss must be 'infonce', 'sigmoid' or 'clip', not {pair_loss!r}")
        if pair_head_weight_decay is not None and (isinstance(pair_head_weight_decay, bool)
                                                   or not isinstance(pair_head_weight_decay, numbers.Real)
                                                   or not math.isfinite(pair_head_weight_decay) or pair_head_weight_decay < 0):
            raise ValueError(f"pair_head_weight_decay must be None or a finite number >= 0, not {pair_head_weight_decay!r}")
        if pair_scale_max is not None and (isinstance(pair_scale_max, bool) or not isinstance(pair_scale_max, numbers.Real)
                                           or not math.isfinite(pair_scale_max) or pair_scale_max <= 0):
            raise ValueError(f"pair_scale_max must be None or a positive finite number, not {pair_scale_max!r}")
        if pair_loss != "clip" and pair_scale_max != 100.0:
            raise ValueError(f"pair_scale_max needs pair_loss='clip' (under {pair_loss!r} nothing is clamped): leave it at its "
                             "default")
        if pair_loss == "clip":
            for name, x, default in (("pair_scale", pair_scale, 10.0), ("pair_bias", pair_bias, -10.0)):
                if x != default:
                    raise ValueError(f"{name} belongs to pair_loss='sigmoid': under 'clip' the scale starts at logit_scale "
                                     "and there is no bias")
            if isinstance(logit_scale, bool) or not isinstance(logit_scale, numbers.Real) or not math.isfinite(logit_scale) \
                    or logit_scale <= 0:
                raise ValueError(f"logit_scale must be a positive finite number under pair_loss='clip' (the head holds its "
                                 f"logarithm), not {logit_scale!r}")
            self.pair_loss = pair_loss
            self.train_pair_head = bool(train_pair_head)
            self.pair_head = nn.Parameter(torch.tensor([math.log(logit_scale)], device=model.device, dtype=torch.float32),
                                          requires_grad=self.train_pair_head)
        elif pair_loss == "sigmoid":
            for name, x in (("pair_scale", pair_scale), ("pair_bias", pair_bias)):
                if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(x):
                    raise ValueError(f"{name} must be a finite number, not {x!r}")
            if pair_scale <= 0:
                raise ValueError(f"pair_scale must be positive (the head holds its logarithm), not {pair_scale!r}")
            self.pair_loss = pair_loss
            self.train_pair_head = bool(train_pair_head)
            self.pair_head = nn.Parameter(torch.tensor([math.log(pair_scale), pair_bias], device=model.device,
                                                       dtype=torch.float32), requires_grad=self.train_pair_head)
        elif train_pair_head:
            raise ValueError("train_pair_head needs pair_loss='sigmoid' or 'clip' (under 'infonce' the logit_scale is a "
                             "host constant)")
        super().__init__(model, lr, weight_decay, betas, eps, logit_scale, prompt_ctx, process_group, shard_text, loss_scale,
                         growth_factor, backoff_factor, growth_interval, init_scale, max_grad_norm, ema_decay)
        self.pair_scale_max = pair_scale_max if pair_loss == "clip" else None
        self.pair_head_weight_decay = pair_head_weight_decay
        if self.train_pair_head:
            # the head is the buffer's tail: its decay (None: the buffer's under "sigmoid", 0 under "clip") and the clamp
            # of log s; where both are what plain AdamW does anyway, the plain launch is issued
            tail_wd = pair_head_weight_decay if pair_head_weight_decay is not None else (0.0 if pair_loss == "clip" else self.wd)
            tail_max = math.log(self.pair_scale_max) if self.pair_scale_max is not None else math.inf
            if tail_wd != self.wd or tail_max != math.inf:
                self.tail_update = (self.pair_head.numel(), float(tail_wd), -math.inf, tail_max)


def gpu_train_loader(root: str, split: str = 'train', image_dir: str = '', batch_size: int = 256, scale=(0.05, 1.0),
                     normalize: bool = True, seed: int = 0, rank: int = 0, world: int = 1, prefetch: bool = True,
                     size: int = 224, threads: int = 8, device=None):
    """lora_train_vlp.py:1196-1218 on the GPU: ``JtDataset(root, split, transform=train_tranform1, mode='train')`` +
    ``DataLoader(batch_size=256, shuffle=True)``.  The images listed in ``{root}/{split}.txt`` (paths relative to
    ``image_dir``, like the reference's ``read_split(split_path, '')``) are decoded once into a device pool; each batch is
    RandomResizedCrop(224, scale) -> RandomHorizontalFlip -> ImageNormalize (``normalize``) made by one kernel launch.
    Yields ``(images, raw, target, index)`` (clipfs.data.TrainLoader); call ``set_epoch`` or iterate again for the next
    epoch."""
    from clipfs import data
    paths, labels = data.read_split(os.path.join(root, f'{split}.txt'), image_dir)
    pool = data.ImagePool.from_files(paths, labels, threads=threads, device=device)
    return data.TrainLoader(pool, batch_size=batch_size, scale=scale, size=size, shuffle=True, seed=seed,
                            outputs=("clip",) if normalize else ("raw",), rank=rank, world=world, prefetch=prefetch)
