"""Host runtime of the HIP engine: collects device pointers from the ``jclip`` model objects into the
C descriptors of include/clipfs.h, owns activation workspaces, and runs the towers forward/backward
with ONE C call per pass (csrc/tower.hip sequences the kernels).  PyTorch supplies device memory,
streams and ``torch.distributed`` only.

Replaces, for the hot path: VisionTransformer.execute / CLIP.encode_text / CLIP.execute
(jclip/model.py:104-126,202-232), TextEncoder.execute (slow_pace.py:837-848), the step body of
run_lora (lora_train_vlp.py:956-1002) and Jittor's autograd + AdamW behind it."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, ops
from ._lib import Block, Tower, check


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _bias_slot(p: Optional[torch.nn.Parameter]) -> Optional[torch.Tensor]:
    """Gradient slot of a trainable bias or deep prompt (``grad_slot``, attached by FlatTrainables or the autograd
    route), else None: a frozen bias gets no slot, and the backward launches nothing for it."""
    if p is None or not p.requires_grad:
        return None
    return getattr(p, "grad_slot", None)


def _lora_trains(a, where: str) -> bool:
    """Whether the LoRA adapters of one attention block train (``requires_grad`` of their A / B).  All or nothing per
    block: a block with some adapters frozen and others trainable is refused rather than training the frozen half."""
    flags = {p.requires_grad for p, _ in a.trainable_pairs()}
    if len(flags) > 1:
        raise ValueError(f"{where}: some of its LoRA adapters are frozen and others trainable; freeze or train the "
                         "q / k / v / o adapters of a block together")
    return flags == {True}


def _mlp_lora_trains(m, where: str) -> bool:
    """Whether one MLP adapter (a ``LinearLoRA`` on ``mlp.c_fc`` / ``mlp.c_proj``) trains; A and B go together."""
    if m.w_lora_A.requires_grad != m.w_lora_B.requires_grad:
        raise ValueError(f"{where}: one of w_lora_A / w_lora_B is frozen and the other trainable; freeze or train both")
    return bool(m.w_lora_A.requires_grad)


def _mlp_adapters(blk):
    """[(token, LinearLoRA)] of the block's adapted MLP linears (lora_train_vlp.mlp_adapters, without the import cycle)."""
    return [(tok, getattr(blk.mlp, tok)) for tok in ("c_fc", "c_proj")
            if getattr(getattr(blk.mlp, tok), "is_mlp_lora", False) and getattr(blk.mlp, tok).r > 0]


def _blk_biases(blk) -> List[torch.nn.Parameter]:
    """The bias parameters of one block (LoRA blocks: the q / k / v views of the packed in-projection bias)."""
    a = blk.attn
    if getattr(a, "is_lora_mha", False):
        out = [a.q_proj.bias, a.k_proj.bias, a.v_proj.bias, a.proj.bias]
    else:
        out = [a.in_proj_bias, a.out_proj.bias]
    return out + [blk.ln_1.bias, blk.ln_2.bias, blk.mlp.c_fc.bias, blk.mlp.c_proj.bias]


def _mix_seed(base: int, step: int) -> int:
    """64-bit non-zero dropout seed for (base, step) -- splitmix64 finaliser."""
    z = (base * 0x9E3779B97F4A7C15 + step * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    z ^= z >> 31
    return z or 1


class _TowerRT:
    """One transformer tower: pointer collection + workspace cache."""

    def __init__(self, transformer, seq: int, stream0: int, name: str = "tower"):
        self.mod = transformer
        self.name = name
        self.seq = seq
        self.width = transformer.width
        self.heads = transformer.heads
        self.layers = transformer.layers
        self.causal = bool(transformer.causal)
        self.stream0 = stream0
        self._bufs: Dict[Tuple[str, int], torch.Tensor] = {}
        self._wt: Dict[int, Dict[str, torch.Tensor]] = {}
        self._planes: Dict[Tuple[int, str, str], torch.Tensor] = {}
        self.precision = "fp32"  # "fp32": exact v_mfma_f32_32x32x2_f32 | "bf16x3": split-bf16, 3 MFMA products
        self.lora_r = 0
        self.lora_scale = 0.0
        self.lora_dropout = 0.0
        # merged-weight cache (``merge``): {block: {"qkv" | "o" | "fc" | "pr": W + scale * B A, fp32}} for the ADAPTED
        # projections only; None = the additive form (every path as if this cache did not exist)
        self._merged: Optional[Dict[int, Dict[str, torch.Tensor]]] = None

    # -- merged weights --------------------------------------------------------------------------
    def _adapted(self):
        """([(block, name, w, a, b, nseg, seg_mask)], r, scale) of the tower's adapted projections in the stacked layouts
        the tower kernels read (qkv: A [3r, d], B [3d, r], one bit per segment; o / fc / pr: one segment)."""
        out, r, scale = [], 0, 0.0

        def shared(m):
            nonlocal r, scale
            if r and (m.r != r or abs(m.scaling - scale) > 0):
                raise ValueError("all LoRA layers of one tower must share r / alpha / dropout")
            r, scale = m.r, float(m.scaling)

        for i, blk in enumerate(self.mod.resblocks):
            a = blk.attn
            if getattr(a, "is_lora_mha", False) and a.r > 0 and a.lora_mask:
                shared(a)
                if a.lora_mask & 7:
                    out.append((i, "qkv", a.qkv_weight, a.lora_A_qkv, a.lora_B_qkv, 3, a.lora_mask & 7))
                if a.lora_mask & 8:
                    out.append((i, "o", a.proj.weight.data, a.lora_A_o, a.lora_B_o, 1, 1))
            for tok, m in _mlp_adapters(blk):
                shared(m)
                out.append((i, "fc" if tok == "c_fc" else "pr", m.weight.data, m.w_lora_A.data, m.w_lora_B.data, 1, 1))
        return out, r, scale

    def merge(self) -> int:
        """Fold every adapter of the tower into copies of its weights with ONE clipfs_lora_merge launch (the 16-bit
        planes of the current precision in the same pass); the master weights are only read.  Returns the number of
        projections folded (q, k and v count one each); 0 = nothing to fold, the tower stays unmerged."""
        jobs, r, scale = self._adapted()
        self.unmerge()
        if not jobs:
            return 0
        fmt = ops.PLANE_FORMATS[self.precision]
        merged: Dict[int, Dict[str, torch.Tensor]] = {}
        table = []
        for i, name, w, a, b, nseg, mask in jobs:
            out = torch.empty_like(w)
            planes = ops.empty_planes(out, fmt)
            table.append((w, a.contiguous(), b.contiguous(), nseg, mask, out, planes))
            merged.setdefault(i, {})[name] = out
            if planes is not None:
                self._planes[(i, "m_" + name, self.precision)] = planes
        ops.lora_merge(table, r, scale, fmt)
        self._merged = merged
        return sum(bin(mask).count("1") for *_, mask in jobs)

    def unmerge(self) -> None:
        self._merged = None
        for key in [k for k in self._planes if k[1].startswith("m_")]:
            del self._planes[key]

    def _point_merged(self, b, i: int, m: Dict[str, torch.Tensor]) -> None:
        """Block pointers of the folded projections of block i (planes of another precision than the merge's are built
        from the folded fp32 copy on first use: bitwise what the merge kernel writes)."""
        for name, w in m.items():
            setattr(b, "w_" + name, _ptr(w))
            if self.precision != "fp32":
                setattr(b, "w_" + name + "_p", _ptr(self._plane(i, "m_" + name, w)))

    # -- descriptor ------------------------------------------------------------------------------
    def _transposed(self, i: int, blk) -> Dict[str, torch.Tensor]:
        wt = self._wt.get(i)
        if wt is None:
            a = blk.attn
            w_qkv = a.qkv_weight if getattr(a, "is_lora_mha", False) else a.in_proj_weight
            w_o = a.proj.weight if getattr(a, "is_lora_mha", False) else a.out_proj.weight
            wt = {"qkv": w_qkv.data.t().contiguous(), "o": w_o.data.t().contiguous(),
                  "fc": blk.mlp.c_fc.weight.data.t().contiguous(), "pr": blk.mlp.c_proj.weight.data.t().contiguous()}
            self._wt[i] = wt
        return wt

    def _plane(self, i: int, name: str, w: torch.Tensor) -> torch.Tensor:
        key = (i, name, self.precision)
        pl = self._planes.get(key)
        if pl is None:
            pl = ops.split_bf16(w.contiguous()) if self.precision == "bf16x3" else ops.to_f16(w.contiguous())
            self._planes[key] = pl
        return pl

    def _block_trains(self, i: int, blk) -> bool:
        """Whether block i gets any gradient slot in ``descriptor`` (a trainable adapter, bias or deep prompt)."""
        a = blk.attn
        if getattr(a, "is_lora_mha", False) and a.r > 0 and _lora_trains(a, f"{self.name} block {i}"):
            return True
        if any(_mlp_lora_trains(m, f"{self.name} block {i} mlp.{tok}") for tok, m in _mlp_adapters(blk)):
            return True
        if _bias_slot(getattr(blk, "VPT_shallow", None)) is not None:
            return True
        return any(_bias_slot(p) is not None for p in _blk_biases(blk))

    def grad_floor(self, needs_input_grad: bool, head_trains: bool = False) -> Optional[int]:
        """The tower's gradient floor (clipfs_tower.grad_lo): the lowest block with a gradient slot; 0 when the tower
        input needs a gradient (prompt ctx, VPT, ln_pre's bias: that gradient runs through every block); None when
        nothing in the tower or its head trains (no backward at all).  A head-only layout (ln_post / ln_final bias
        trained, every block frozen) keeps the top block: the head's input is that block's output."""
        if needs_input_grad:
            return 0
        for i, blk in enumerate(self.mod.resblocks):
            if self._block_trains(i, blk):
                return i
        return self.layers - 1 if head_trains else None

    def descriptor(self, train: bool, seed: int, seq: Optional[int] = None, row0: int = 0, grad_lo: int = 0) -> Tower:
        merged = self._merged
        if merged is not None:
            # a merged tower is forward-only and dropout-free: nothing was saved for a backward through W + s B A, and a
            # train-mode forward of the additive form would drop
            if train:
                raise ValueError(f"{self.name} tower: its LoRA adapters are merged into the weights (merge_lora), which "
                                 "is forward-only -- call unmerge_lora before a forward that keeps activations")
            if seed and self.lora_dropout_rate() > 0:
                raise ValueError(f"{self.name} tower: a train-mode forward with adapter dropout "
                                 f"{self.lora_dropout_rate():g} cannot run on merged weights -- call unmerge_lora (or "
                                 "model.eval()) first")
        blocks = (Block * self.layers)()
        r, scale, p = 0, 0.0, 0.0
        # deep prompts: the vision tower's last prompt_rows rows (its VPT rows), the text tower's rows 1 ... prompt_rows
        n_pr = getattr(self.mod, "prompt_rows", 0)
        first = (seq or self.seq) - n_pr if getattr(self.mod, "prompt_tail", False) else 1
        for i, blk in enumerate(self.mod.resblocks):
            a = blk.attn
            b = blocks[i]
            vp = getattr(blk, "VPT_shallow", None)
            if vp is not None:
                # the kernels read prompt_rows rows of the prompt and add as many into its slot: both must be exactly
                # [n_pr, width] fp32 on this device (the row count comes from the tensor and must match the placement)
                g = _bias_slot(vp)
                ok = (vp.dim() == 2 and tuple(vp.shape) == (n_pr, self.width) and vp.dtype == torch.float32
                      and vp.is_contiguous() and vp.device == self.mod.resblocks[0].ln_1.weight.device and first >= 1)
                if g is not None:
                    ok = ok and g.shape == vp.shape and g.dtype == torch.float32 and g.is_contiguous() and g.device == vp.device
                if not ok:
                    raise ValueError(f"{self.name} block {i}: deep prompt {tuple(vp.shape)} (slot "
                                     f"{None if g is None else tuple(g.shape)}) does not fit the tower's placement of "
                                     f"{n_pr} rows of width {self.width} from row {first}")
                b.prompt, b.g_prompt = _ptr(vp), _ptr(g)
                b.prompt_first, b.prompt_rows = first, vp.shape[0]
            lora = getattr(a, "is_lora_mha", False)
            if lora:
                w_qkv, b_qkv, w_o, b_o = a.qkv_weight, a.qkv_bias, a.proj.weight, a.proj.bias
            else:
                w_qkv, b_qkv, w_o, b_o = a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias
            b.ln1_g, b.ln1_b = _ptr(blk.ln_1.weight), _ptr(blk.ln_1.bias)
            b.ln2_g, b.ln2_b = _ptr(blk.ln_2.weight), _ptr(blk.ln_2.bias)
            b.w_qkv, b.b_qkv = _ptr(w_qkv), _ptr(b_qkv)
            b.w_o, b.b_o = _ptr(w_o), _ptr(b_o)
            b.w_fc, b.b_fc = _ptr(blk.mlp.c_fc.weight), _ptr(blk.mlp.c_fc.bias)
            b.w_pr, b.b_pr = _ptr(blk.mlp.c_proj.weight), _ptr(blk.mlp.c_proj.bias)
            # bias gradient slots (NULL = frozen): the q / k / v segments of the packed in-projection bias separately
            if lora:
                gq, gk, gv = (_bias_slot(getattr(a, n).bias) for n in ("q_proj", "k_proj", "v_proj"))
                go = _bias_slot(a.proj.bias)
            else:
                g = _bias_slot(a.in_proj_bias)
                d = self.width
                gq, gk, gv = (None, None, None) if g is None else (g[:d], g[d:2 * d], g[2 * d:])
                go = _bias_slot(a.out_proj.bias)
            b.g_b_q, b.g_b_k, b.g_b_v, b.g_b_o = _ptr(gq), _ptr(gk), _ptr(gv), _ptr(go)
            b.g_ln1_b, b.g_ln2_b = _ptr(_bias_slot(blk.ln_1.bias)), _ptr(_bias_slot(blk.ln_2.bias))
            b.g_b_fc, b.g_b_pr = _ptr(_bias_slot(blk.mlp.c_fc.bias)), _ptr(_bias_slot(blk.mlp.c_proj.bias))
            if train:
                wt = self._transposed(i, blk)
                b.w_qkv_t, b.w_o_t, b.w_fc_t, b.w_pr_t = _ptr(wt["qkv"]), _ptr(wt["o"]), _ptr(wt["fc"]), _ptr(wt["pr"])
            if self.precision != "fp32":
                b.w_qkv_p = _ptr(self._plane(i, "qkv", w_qkv.data))
                b.w_o_p = _ptr(self._plane(i, "o", w_o.data))
                b.w_fc_p = _ptr(self._plane(i, "fc", blk.mlp.c_fc.weight.data))
                b.w_pr_p = _ptr(self._plane(i, "pr", blk.mlp.c_proj.weight.data))
                if train:
                    b.w_qkv_t_p = _ptr(self._plane(i, "qkv_t", wt["qkv"]))
                    b.w_o_t_p = _ptr(self._plane(i, "o_t", wt["o"]))
                    b.w_fc_t_p = _ptr(self._plane(i, "fc_t", wt["fc"]))
                    b.w_pr_t_p = _ptr(self._plane(i, "pr_t", wt["pr"]))
            b.lora_mask = 0
            if merged is not None:  # an ordinary model to every kernel and mode query: no adapter pointers, lora_r 0
                if i in merged:
                    self._point_merged(b, i, merged[i])
                continue
            if lora and a.r > 0:
                if r and (a.r != r or abs(a.scaling - scale) > 0 or abs(a.dropout_rate - p) > 0):
                    raise ValueError("all LoRA layers of one tower must share r / alpha / dropout")
                r, scale, p = a.r, float(a.scaling), float(a.dropout_rate)
                b.lora_mask = a.lora_mask
                # gradient slots only for trainable adapters: NULL slots = frozen, the tower computes the adapter's
                # input-gradient contribution only and AdamW never sees it
                trains = _lora_trains(a, f"{self.name} block {i}")
                b.lora_a_qkv, b.lora_b_qkv = _ptr(a.lora_A_qkv), _ptr(a.lora_B_qkv)
                if trains:
                    b.g_lora_a_qkv, b.g_lora_b_qkv = _ptr(a.grad_A_qkv), _ptr(a.grad_B_qkv)
                if a.lora_mask & 8:
                    b.lora_a_o, b.lora_b_o = _ptr(a.lora_A_o), _ptr(a.lora_B_o)
                    if trains:
                        b.g_lora_a_o, b.g_lora_b_o = _ptr(a.grad_A_o), _ptr(a.grad_B_o)
            for tok, m in _mlp_adapters(blk):  # lora_mask bits 4 (c_fc) and 5 (c_proj)
                if r and (m.r != r or abs(m.scaling - scale) > 0 or abs(m.dropout_rate - p) > 0):
                    raise ValueError("all LoRA layers of one tower must share r / alpha / dropout")
                r, scale, p = m.r, float(m.scaling), float(m.dropout_rate)
                trains = _mlp_lora_trains(m, f"{self.name} block {i} mlp.{tok}")
                for q in (m.w_lora_A, m.w_lora_B):
                    if not (q.dtype == torch.float32 and q.is_contiguous() and q.data_ptr() % 16 == 0):
                        raise ValueError(f"{self.name} block {i} mlp.{tok}: adapter tensors must be contiguous fp32, 16-byte aligned")
                    if trains:
                        _ensure_slot(q)
                ga, gb = (_ptr(m.w_lora_A.grad_slot), _ptr(m.w_lora_B.grad_slot)) if trains else (None, None)
                if tok == "c_fc":
                    b.lora_mask |= 16
                    b.lora_a_fc, b.lora_b_fc, b.g_lora_a_fc, b.g_lora_b_fc = _ptr(m.w_lora_A), _ptr(m.w_lora_B), ga, gb
                else:
                    b.lora_mask |= 32
                    b.lora_a_pr, b.lora_b_pr, b.g_lora_a_pr, b.g_lora_b_pr = _ptr(m.w_lora_A), _ptr(m.w_lora_B), ga, gb
        t = _lib.new_tower()
        t.width, t.heads, t.layers, t.seq, t.causal = (self.width, self.heads, self.layers, seq or self.seq,
                                                       int(self.causal))
        t.lora_r, t.lora_scale, t.lora_dropout = r, scale, p
        # dropout follows the MODULE's train mode (LinearLoRA.execute, lora_train_vlp.py:297-298), not whether
        # activations are saved: a no-grad forward in train mode (slow_pace.py:1659-1661) still drops
        t.dropout_seed = seed if p > 0 else 0
        t.dropout_stream0 = self.stream0
        t.dropout_row0 = row0 * (seq or self.seq)  # first TOKEN row of this call in the global batch
        t.weight_format = {"fp32": 0, "bf16x3": 1, "fp16": 2}[self.precision]
        t.grad_lo = grad_lo
        t.blocks = C.cast(blocks, C.POINTER(Block))
        t._blocks_keepalive = blocks  # ctypes array must outlive the call
        self.lora_r, self.lora_scale, self.lora_dropout = r, scale, p
        return t

    def lora_dropout_rate(self) -> float:
        return max([float(b.attn.dropout_rate) for b in self.mod.resblocks
                    if getattr(b.attn, "is_lora_mha", False) and b.attn.r > 0]
                   + [float(m.dropout_rate) for b in self.mod.resblocks for _, m in _mlp_adapters(b)], default=0.0)

    def has_lora(self) -> bool:
        return any((getattr(b.attn, "is_lora_mha", False) and b.attn.r > 0) or _mlp_adapters(b) for b in self.mod.resblocks)

    # -- workspaces -----------------------------------------------------------------------------
    def buffer(self, kind: str, n_floats: int, device) -> torch.Tensor:
        key = (kind, n_floats)
        buf = self._bufs.get(key)
        if buf is None:
            # drop stale sizes of the same kind before allocating (batch size changed)
            for k in [k for k in self._bufs if k[0] == kind]:
                del self._bufs[k]
            buf = torch.empty(max(n_floats, 4), device=device, dtype=torch.float32)
            self._bufs[key] = buf
        return buf

    def _attach_counters(self, t: Tower, batch: int, device) -> None:
        """Split-K arrival counters of the tower's GEMMs: zeroed once here, left zero by every launch; one buffer per
        tower (the two towers run on different streams)."""
        n = _lib.load().clipfs_tower_counter_ints(C.byref(t), batch)
        if n == 0:
            return
        buf = self._bufs.get(("counters", 0))
        if buf is None or buf.numel() < n:
            buf = torch.zeros(n, device=device, dtype=torch.int32)
            self._bufs[("counters", 0)] = buf
        t.gemm_counters, t.gemm_counters_ints = buf.data_ptr(), buf.numel()

    def forward(self, x: torch.Tensor, batch: int, train: bool, seed: int, seq: Optional[int] = None,
                own_saved: bool = False, row0: int = 0, rows: Optional[torch.Tensor] = None, grad_lo: int = 0,
                pack: Optional[Tuple[torch.Tensor, int]] = None, desc: Optional[Tower] = None):
        """``train`` = keep the activations the backward needs.  ``own_saved``: give this call its OWN saved-activation
        tensor (the autograd route: several grad-enabled forwards of one tower may precede one backward, e.g. the 13
        caption chunks of encode_text_in_batches, lora_train_vlp.py:905-912); otherwise the per-tower cached buffer
        is reused (LoRATrainer: exactly one forward per backward).  ``grad_lo``: the gradient floor (``grad_floor``);
        only blocks grad_lo ... top keep activations, and the backward must be given the same floor.  ``pack``: (plan, R)
        of ``Engine._pack_plan`` with ``rows``: every block runs on the live rows (clipfs_tower_fwd_packed; the caller
        checked ``pack_fwd_mode``), and the backward is ``backward_packed(..., saved_packed=True)``.  ``desc``: this
        call's descriptor when the caller already built it (the same arguments)."""
        lib = _lib.load()
        t = desc if desc is not None else self.descriptor(train, seed, seq, row0, grad_lo if train else 0)
        self._attach_counters(t, batch, x.device)
        scratch = self.buffer("scratch", lib.clipfs_tower_scratch_floats(C.byref(t), batch), x.device)
        saved = None
        if train:
            n = lib.clipfs_tower_saved_floats(C.byref(t), batch)
            saved = torch.empty(max(n, 4), device=x.device, dtype=torch.float32) if own_saved else \
                self.buffer("saved", n, x.device)
        if rows is not None:
            # the caller reads one row per sequence (``rows`` [batch] int32): the last block's output projection and MLP
            # run on those rows only; the matching backward is ``backward_sparse`` with the same rows
            assert rows.dtype == torch.int32 and rows.is_cuda and rows.numel() >= batch
        if pack is not None:
            assert rows is not None
            plan, R = pack
            check(lib.clipfs_tower_fwd_packed(C.byref(t), x.data_ptr(), rows.data_ptr(), plan.data_ptr(), R, batch, _ptr(saved),
                                              scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "tower_fwd_packed")
        elif rows is not None:
            check(lib.clipfs_tower_fwd_rows(C.byref(t), x.data_ptr(), rows.data_ptr(), batch, _ptr(saved), scratch.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "tower_fwd_rows")
        else:
            check(lib.clipfs_tower_fwd(C.byref(t), x.data_ptr(), batch, _ptr(saved), scratch.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "tower_fwd")
        return saved

    def backward(self, dx: torch.Tensor, batch: int, saved: torch.Tensor, seed: int, stop_at_input: bool,
                 seq: Optional[int] = None, row0: int = 0, grad_lo: int = 0):
        lib = _lib.load()
        t = self.descriptor(True, seed, seq, row0, grad_lo)
        self._attach_counters(t, batch, dx.device)
        scratch = self.buffer("scratch", lib.clipfs_tower_scratch_floats(C.byref(t), batch), dx.device)
        check(lib.clipfs_tower_bwd(C.byref(t), dx.data_ptr(), batch, saved.data_ptr(), scratch.data_ptr(),
                                   int(stop_at_input), torch.cuda.current_stream().cuda_stream), "tower_bwd")


    def backward_sparse(self, dxs: torch.Tensor, rows: torch.Tensor, batch: int, saved: torch.Tensor, seed: int,
                        stop_at_input: bool, seq: Optional[int] = None, row0: int = 0, grad_lo: int = 0) -> torch.Tensor:
        """Backward from a gradient that is non-zero in ONE row per sequence (``dxs`` [batch, width] at token ``rows``
        [batch] int32): the class token of the image head, the EOT token of the text head.  Returns the dense gradient
        wrt the tower input (uninitialised when ``stop_at_input``)."""
        lib = _lib.load()
        t = self.descriptor(True, seed, seq, row0, grad_lo)
        self._attach_counters(t, batch, dxs.device)
        scratch = self.buffer("scratch", lib.clipfs_tower_scratch_floats(C.byref(t), batch), dxs.device)
        dx = torch.empty(batch * (seq or self.seq), self.width, device=dxs.device, dtype=torch.float32)
        check(lib.clipfs_tower_bwd_sparse(C.byref(t), dxs.data_ptr(), rows.data_ptr(), dx.data_ptr(), batch, saved.data_ptr(),
                                          scratch.data_ptr(), int(stop_at_input), torch.cuda.current_stream().cuda_stream),
              "tower_bwd_sparse")
        return dx

    def backward_packed(self, dxs: torch.Tensor, rows: torch.Tensor, plan: torch.Tensor, R: int, batch: int,
                        saved: torch.Tensor, seed: int, stop_at_input: bool, seq: Optional[int] = None, row0: int = 0,
                        grad_lo: int = 0, saved_packed: bool = False) -> torch.Tensor:
        """``backward_sparse`` of a causal tower on its live rows only (clipfs_tower_bwd_packed; ``plan`` / ``R`` from
        ``Engine._pack_plan``).  Same return value; runs the dense rows where the library does not pack.
        ``saved_packed``: ``saved`` is the live-row forward's (clipfs_tower_bwd_packed_saved)."""
        lib = _lib.load()
        t = self.descriptor(True, seed, seq, row0, grad_lo)
        self._attach_counters(t, batch, dxs.device)
        scratch = self.buffer("scratch", lib.clipfs_tower_scratch_floats(C.byref(t), batch), dxs.device)
        dx = torch.empty(batch * (seq or self.seq), self.width, device=dxs.device, dtype=torch.float32)
        fn = lib.clipfs_tower_bwd_packed_saved if saved_packed else lib.clipfs_tower_bwd_packed
        check(fn(C.byref(t), dxs.data_ptr(), rows.data_ptr(), plan.data_ptr(), R, dx.data_ptr(), batch, saved.data_ptr(),
                 scratch.data_ptr(), int(stop_at_input), torch.cuda.current_stream().cuda_stream),
              "tower_bwd_packed_saved" if saved_packed else "tower_bwd_packed")
        return dx

    def pack_mode(self, batch: int, R: int, seed: int, seq: Optional[int] = None, grad_lo: int = 0,
                  train: bool = True) -> bool:
        """Whether ``backward_packed`` runs packed for this geometry (clipfs_tower_pack_mode)."""
        t = self.descriptor(train, seed, seq, 0, grad_lo)
        return bool(_lib.load().clipfs_tower_pack_mode(C.byref(t), batch, R))

    @staticmethod
    def pack_modes(desc: Tower, batch: int, R: int) -> Tuple[bool, bool]:
        """(clipfs_tower_pack_mode, clipfs_tower_pack_fwd_mode) for an already built descriptor."""
        lib = _lib.load()
        return bool(lib.clipfs_tower_pack_mode(C.byref(desc), batch, R)), bool(lib.clipfs_tower_pack_fwd_mode(C.byref(desc), batch, R))

    def pack_fwd_mode(self, batch: int, R: int, seed: int, seq: Optional[int] = None, grad_lo: int = 0,
                      train: bool = True) -> bool:
        """Whether ``forward(..., pack=...)`` runs on the live rows for this geometry (clipfs_tower_pack_fwd_mode)."""
        t = self.descriptor(train, seed, seq, 0, grad_lo)
        return bool(_lib.load().clipfs_tower_pack_fwd_mode(C.byref(t), batch, R))


class Engine:
    def __init__(self, model):
        self.model = model
        v = model.visual
        # A ModifiedResNet image tower (RN50 family, jclip.model.ModifiedResNet) is a frozen fp32 feature extractor with a
        # runner of its own (clipfs/resnet.py: ClipResNet): no tower runtime (``vis``), no projection copy, no backward.
        self.resnet = _is_resnet(v)
        if not self.resnet:
            self.vis = _TowerRT(v.transformer, v.tokens, stream0=1000, name="vision")
        self.txt = _TowerRT(model.transformer, model.context_length, stream0=0, name="text")
        if not self.resnet:
            self.vproj_t = v.proj.data.t().contiguous()              # [E, width]  (NT form of x @ proj)
        self.tproj_t = model.text_projection.data.t().contiguous()   # [E, width]
        self.seed_base = 0x5EED
        self.step = 0
        # Optional (off by default): run the text tower only on positions <= the last EOT of the batch.  Under the
        # causal mask nothing after a caption's EOT can influence its EOT feature, nor receive gradient from it, so
        # the reference's rows EOT+1..76 (jclip/model.py:202-215 encodes all 77) are dead work.  With LoRA dropout the
        # masks are indexed by token row = caption * (trimmed seq) + position: a trimmed run draws a different (equally
        # valid) mask stream than the untrimmed one, and LoRATrainer refuses trim_text + class-sharded text + dropout.
        self.trim_text = False
        self._trim_cache = {}
        # One row per sequence in the LAST block: the heads read the class token / the EOT token only, so after the last
        # attention everything is computed for that row alone -- forward (clipfs_tower_fwd_rows: output projection,
        # LayerNorm 2, MLP) and backward (clipfs_tower_bwd_sparse).  False = every block dense in both directions, the
        # gradient rows scattered into a zero-filled tensor (identical features and gradients; kept as the A/B
        # reference, bench.py reports it as a variant).  The name predates the forward half.
        self.sparse_backward = True
        # Gradient floor per tower (_TowerRT.grad_floor): blocks below the lowest one that trains keep no activations and
        # get no backward, and a tower with nothing to train gets no backward at all (LoRATrainer).  Features and
        # gradients are bitwise those of the full-depth path.  False = every tower saves and back-propagates every block
        # (the A/B reference; frozen adapters are still never trained).
        self.prune_backward = True
        # Text backward on live rows only (clipfs_tower_bwd_packed): under the causal mask a caption's gradient is zero
        # on every row after its EOT, so below the last block's compact part the text tower back-propagates the
        # R = sum (eot + 1) rows 0 .. eot of each caption (31 % of the rows for the bench's captions).  Applies on the
        # one-row path only (``sparse_backward``).  Loss and logits are unchanged; parameter gradients differ only in
        # summation order.  False = every row of every block (the A/B reference).
        self.pack_text_backward = True
        # Text FORWARD on the same live rows (clipfs_tower_fwd_packed): row i of a causal block reads rows <= i only, so
        # every block runs on the R packed rows and the last block's compact part on the EOT rows; the backward then reads
        # the packed saved tensors in place.  Applies where the backward packs (needs ``pack_text_backward``) and the
        # library's clipfs_tower_pack_fwd_mode agrees, in training and in no-grad forwards alike.  Every feature, dropout
        # mask and gradient is bitwise that of the dense forward.  False = the dense forward (the A/B reference).
        self.pack_text_forward = True
        self._pack_cache = {}

    @property
    def precision(self) -> str:
        return self.txt.precision if self.resnet else self.vis.precision

    @precision.setter
    def precision(self, mode: str) -> None:
        """"fp32" (default): every GEMM on the exact fp32 MFMA.  "bf16x3": the tower GEMMs (97 % of the FLOPs) run
        as split-bf16 with three bf16 MFMA products per operand pair, fp32 accumulate (weights are split once;
        logits move by ~2e-4 on 100 x cosine, inside the 1e-3 budget).  LayerNorm, attention, LoRA, the patch /
        projection / logits GEMMs and all reductions stay fp32.  "fp16": the same GEMMs with f16 operands
        (v_mfma_f32_32x32x16_f16, fp32 accumulate) -- cfg-5's "MFMA fp16 path"; tolerance ~1e-2 on the logits.
        A ModifiedResNet image tower stays fp32 in every mode: the setting then reaches the text tower only."""
        if mode not in ("fp32", "bf16x3", "fp16"):
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'fp16'")
        if not self.resnet:
            self.vis.precision = mode
        self.txt.precision = mode

    # -- merged weights -------------------------------------------------------------------------------
    def _towers(self) -> List[_TowerRT]:
        return [self.txt] if self.resnet else [self.txt, self.vis]

    @property
    def merged(self) -> bool:
        """Whether the towers run on folded copies of their weights (``merge``): then every forward is the one of a model
        that never had adapters, and anything that needs the additive form (a backward, adapter dropout) is refused."""
        return any(t._merged is not None for t in self._towers())

    def merge(self) -> int:
        """Fold the adapters of both towers (one launch per tower that has any); the number of projections folded."""
        try:
            return sum(t.merge() for t in self._towers())
        except Exception:
            self.unmerge()  # never one tower merged and the other not
            raise

    def unmerge(self) -> None:
        for t in self._towers():
            t.unmerge()

    def refuse_merged(self, what: str) -> None:
        if self.merged:
            raise ValueError(f"{what}: the LoRA adapters are merged into the weights (merge_lora), which is forward-only "
                             "-- call unmerge_lora first")

    # -- backward plan --------------------------------------------------------------------------------
    def image_plan(self) -> Optional[int]:
        """Gradient floor of the image tower (None: nothing of it trains).  0 with a VPT or a trainable ln_pre bias.
        Always None for a ModifiedResNet: the trunk is frozen."""
        if self.resnet:
            return None
        if not self.prune_backward:
            return 0
        v = self.model.visual
        return self.vis.grad_floor(v.VPT is not None or _bias_slot(v.ln_pre.bias) is not None,
                                   _bias_slot(v.ln_post.bias) is not None)

    def text_plan(self, has_ctx: bool) -> Optional[int]:
        """Gradient floor of the text tower (None: nothing of it trains).  0 with prompt ctx tokens."""
        if not self.prune_backward:
            return 0
        return self.txt.grad_floor(has_ctx, _bias_slot(self.model.ln_final.bias) is not None)

    # -- seeds ------------------------------------------------------------------------------------
    def next_seed(self) -> int:
        self.step += 1
        return _mix_seed(self.seed_base, self.step)

    # -- image tower --------------------------------------------------------------------------------
    def vit_forward(self, images: torch.Tensor, train: bool, seed: int = 0, own_saved: bool = False, row0: int = 0):
        """``row0``: index of images[0] in the GLOBAL batch (data-parallel shard) -- only the dropout masks see it.
        ``train``: keep what the backward needs; with nothing of the image side to train (``image_plan`` None) the pass
        is the no-grad one and the returned ctx is None.  A ModifiedResNet tower (frozen, no dropout) always is."""
        lo = self.image_plan() if train else 0
        if lo is None:
            train = False
        m = self.model
        v = m.visual
        assert images.is_cuda and images.dtype == torch.float32, "images: fp32 device tensor [B,3,R,R]"
        images = images.contiguous()
        B = images.shape[0]
        if images.shape[1] != 3 or images.shape[2] != v.input_resolution or images.shape[3] != v.input_resolution:
            raise ValueError(f"expected images [B,3,{v.input_resolution},{v.input_resolution}], got {tuple(images.shape)}")
        if self.resnet:
            return v(images), None
        L, d = v.tokens, v.width
        P = (v.input_resolution // v.patch_size) ** 2
        x0 = torch.empty(B * L, d, device=images.device, dtype=torch.float32)
        ops.patch_embed(images, v.conv1.weight.data, v.positional_embedding.data, x0, L)
        ops.vit_fill_special(x0, v.class_embedding.data, v.positional_embedding.data,
                             None if v.VPT is None else v.VPT.data, B, L, P)
        need_pre = train and v.VPT is not None
        if need_pre:
            x, mean0, rstd0 = ops.layernorm_fwd(x0, v.ln_pre.weight.data, v.ln_pre.bias.data, save_stats=True)
        else:
            x = ops.layernorm_fwd(x0, v.ln_pre.weight.data, v.ln_pre.bias.data)
            mean0 = rstd0 = None
        # only the class-token row of each image is read below (jclip/model.py:121-124)
        one_row = bool(self.sparse_backward)
        saved = self.vis.forward(x, B, train, seed, own_saved=own_saved, row0=row0,
                                 rows=self._class_rows(B, images.device) if one_row else None, grad_lo=lo)
        if train:
            y, mean1, rstd1 = ops.layernorm_fwd(x, v.ln_post.weight.data, v.ln_post.bias.data, ldx=L * d, rows=B,
                                                save_stats=True)
        else:
            y = ops.layernorm_fwd(x, v.ln_post.weight.data, v.ln_post.bias.data, ldx=L * d, rows=B)
            mean1 = rstd1 = None
        feat = ops.gemm_nt(y, self.vproj_t)
        ctx = None
        if train:
            ctx = dict(B=B, x_final=x, saved=saved, stats=(mean1, rstd1), seed=seed, row0=row0, one_row=one_row,
                       pre=(x0, mean0, rstd0) if need_pre else None, lo=lo)
        return feat, ctx

    def vit_tokens(self, images: torch.Tensor, seed: int = 0):
        """Every row of the image tower through ln_post and proj, without a graph: (tokens [B, P, embed] -- the P patch
        rows; the class row and the VPT rows are dropped -- and the class-row feature [B, embed]).  The tower runs its
        dense forward: the one-row last block of ``vit_forward`` leaves the patch rows of the last block unfinished."""
        if self.resnet:
            raise ValueError("encode_image_tokens: a ModifiedResNet tower has no local tokens here -- its attention-pool head "
                             "computes the one query row only (ViT towers only)")
        v = self.model.visual
        assert images.is_cuda and images.dtype == torch.float32, "images: fp32 device tensor [B,3,R,R]"
        images = images.contiguous()
        B = images.shape[0]
        if images.shape[1] != 3 or images.shape[2] != v.input_resolution or images.shape[3] != v.input_resolution:
            raise ValueError(f"expected images [B,3,{v.input_resolution},{v.input_resolution}], got {tuple(images.shape)}")
        L, d = v.tokens, v.width
        P = (v.input_resolution // v.patch_size) ** 2
        x0 = torch.empty(B * L, d, device=images.device, dtype=torch.float32)
        ops.patch_embed(images, v.conv1.weight.data, v.positional_embedding.data, x0, L)
        ops.vit_fill_special(x0, v.class_embedding.data, v.positional_embedding.data,
                             None if v.VPT is None else v.VPT.data, B, L, P)
        x = ops.layernorm_fwd(x0, v.ln_pre.weight.data, v.ln_pre.bias.data)
        self.vis.forward(x, B, False, seed)
        y = ops.layernorm_fwd(x, v.ln_post.weight.data, v.ln_post.bias.data)
        feat = ops.gemm_nt(y, self.vproj_t).view(B, L, -1)
        return feat[:, 1:1 + P].contiguous(), feat[:, 0].contiguous()

    def vit_backward(self, ctx: dict, dfeat: torch.Tensor) -> None:
        """Accumulates into the LoRA gradient slots (and VPT.grad_slot, and the slots of trainable biases)."""
        v = self.model.visual
        B, L, d = ctx["B"], v.tokens, v.width
        dy = ops.gemm_nt(dfeat.contiguous(), v.proj.data)  # [B, width] = dfeat @ proj^T
        g_post = _bias_slot(v.ln_post.bias)
        if g_post is not None:
            ops.bias_grad(dy, g_post)
        # ln_pre's bias gradient is the column sum of the gradient wrt the tower input: block 0 then runs to the end
        g_pre = _bias_slot(v.ln_pre.bias)
        mean1, rstd1 = ctx["stats"]
        # only the class-token row of each image carries gradient (jclip/model.py:121-124): it stays compact [B, width]
        # and the tower's last block works on B rows (clipfs_tower_bwd_sparse) -- no zero-filled [B*L, width] tensor
        dcls = ops.layernorm_bwd(dy, ctx["x_final"], v.ln_post.weight.data, mean1, rstd1, ldx=L * d)
        has_vpt = v.VPT is not None
        stop = not (has_vpt or g_pre is not None)
        if ctx["one_row"]:  # the forward that produced ``saved`` decides (its last block kept one row per image)
            dx = self.vis.backward_sparse(dcls, self._class_rows(B, dfeat.device), B, ctx["saved"], ctx["seed"],
                                          stop_at_input=stop, row0=ctx["row0"], grad_lo=ctx["lo"])
        else:
            dx = ops.scatter_rows(dcls, self._class_rows(B, dfeat.device), L)
            self.vis.backward(dx, B, ctx["saved"], ctx["seed"], stop_at_input=stop, row0=ctx["row0"], grad_lo=ctx["lo"])
        if g_pre is not None:
            ops.bias_grad(dx, g_pre)
        if has_vpt:
            x0, mean0, rstd0 = ctx["pre"]
            dx0 = ops.layernorm_bwd(dx, x0, v.ln_pre.weight.data, mean0, rstd0)
            P = (v.input_resolution // v.patch_size) ** 2
            ops.token_rows_grad(dx0, v.VPT.grad_slot, B, L, 1 + P)

    def _class_rows(self, batch: int, device) -> torch.Tensor:
        z = getattr(self, "_zero_rows", None)
        if z is None or z.numel() < batch or z.device != device:
            z = torch.zeros(max(batch, 256), device=device, dtype=torch.int32)
            self._zero_rows = z
        return z[:batch]

    # -- text tower --------------------------------------------------------------------------------
    def _effective_ids(self, ids: torch.Tensor):
        """(ids possibly truncated to the batch's last EOT, effective sequence length)."""
        if not self.trim_text:
            return ids, ids.shape[1]
        key = (ids.data_ptr(), tuple(ids.shape), ids._version)
        hit = self._trim_cache.get(key)
        if hit is None:
            leff = int(ids.argmax(dim=-1).max().item()) + 1  # one host sync per distinct caption table
            hit = (ids[:, :leff].contiguous(), leff)
            self._trim_cache = {key: hit}
        return hit

    def _pack_plan(self, ids: torch.Tensor, ids_host: Optional[torch.Tensor] = None):
        """(plan, R) of clipfs_tower_bwd_packed for a caption table ``ids`` [n, seq]: off [n + 1] | eotp [n] | map [R], int32
        on the device.  Built once per distinct table, cached like ``_effective_ids``; the entry holds ``ids`` so that its
        storage cannot be reused under the same key.  ``ids_host``: the same table still on the host (the drop-in route
        uploads its ids every call): the plan is then built there and uploaded with them, with no device-to-host sync."""
        key = (ids.data_ptr(), tuple(ids.shape), ids._version)
        hit = self._pack_cache.get(key)
        if hit is None:
            n, seq = ids.shape
            src = ids if ids_host is None else ids_host[:, :seq]
            if ids_host is None:
                lens = ops.eot_index(ids).to(torch.int64) + 1
            else:  # first maximum, as clipfs_eot_index
                lens = src.to(torch.int64).argmax(dim=-1) + 1
            off = torch.zeros(n + 1, device=src.device, dtype=torch.int64)
            off[1:] = torch.cumsum(lens, 0)
            R = int(off[-1].item())  # device tables: one host sync per distinct caption table
            cap = torch.repeat_interleave(torch.arange(n, device=src.device), lens, output_size=R)
            rows = cap * seq + torch.arange(R, device=src.device) - off[cap]
            plan = torch.cat([off, off[1:] - 1, rows]).to(device=ids.device, dtype=torch.int32)
            hit = (plan, R, ids)
            if len(self._pack_cache) >= 4:  # a few tables (training captions, eval captions) without rebuilding
                self._pack_cache.pop(next(iter(self._pack_cache)))
            self._pack_cache[key] = hit
        return hit[0], hit[1]

    def text_forward(self, ids: torch.Tensor, prompt_ctx: Optional[torch.Tensor], train: bool, seed: int = 0,
                     own_saved: bool = False, row0: int = 0):
        """As ``vit_forward``: with nothing of the text side to train (``text_plan`` None) the pass is the no-grad one
        and the returned ctx is None."""
        lo = self.text_plan(prompt_ctx is not None) if train else 0
        if lo is None:
            train = False
        m = self.model
        ids_host = ids if not ids.is_cuda else None
        ids = ids.to(device=m.device, dtype=torch.int64).contiguous()
        n, seq = ids.shape
        if seq != m.context_length:
            raise ValueError(f"expected token ids [N,{m.context_length}], got {tuple(ids.shape)}")
        ids, seq = self._effective_ids(ids)
        x = ops.text_embed(ids, m.token_embedding.weight.data, m.positional_embedding.data,
                           None if prompt_ctx is None else prompt_ctx.data)
        # only the EOT row of each caption is read below (jclip/model.py:213-214)
        one_row = bool(self.sparse_backward)
        # live rows (clipfs_tower_bwd_packed / clipfs_tower_fwd_packed): the plan is cached per caption table, so a
        # steady-state step builds nothing; the first check at R = n skips the plan for geometries that never pack
        # (one descriptor serves the checks and the forward)
        desc = self.txt.descriptor(train, seed, seq, row0, lo if train else 0)
        pack, pack_fwd = None, False
        if one_row and self.pack_text_backward and self.txt.pack_modes(desc, n, n)[0]:
            plan, R = self._pack_plan(ids, ids_host)
            bwd, fwd = self.txt.pack_modes(desc, n, R)
            if bwd:
                pack = (plan, R)
                pack_fwd = self.pack_text_forward and fwd
        saved = self.txt.forward(x, n, train, seed, seq, own_saved=own_saved, row0=row0,
                                 rows=ops.eot_index(ids) if one_row else None, grad_lo=lo,
                                 pack=pack if pack_fwd else None, desc=desc)
        rows, idx = ops.gather_eot(x, ids)
        if train:
            y, mean, rstd = ops.layernorm_fwd(rows, m.ln_final.weight.data, m.ln_final.bias.data, save_stats=True)
        else:
            y = ops.layernorm_fwd(rows, m.ln_final.weight.data, m.ln_final.bias.data)
            mean = rstd = None
        feat = ops.gemm_nt(y, self.tproj_t)
        ctx = None
        if train:
            ctx = dict(n=n, seq=seq, rows=rows, idx=idx, stats=(mean, rstd), saved=saved, seed=seed, row0=row0,
                       one_row=one_row, has_ctx=prompt_ctx is not None, lo=lo, pack=pack, pack_fwd=pack_fwd)
        return feat, ctx

    def text_backward(self, ctx: dict, dfeat: torch.Tensor, dctx_slot: Optional[torch.Tensor] = None) -> None:
        m = self.model
        n, seq = ctx["n"], ctx["seq"]
        dy = ops.gemm_nt(dfeat.contiguous(), m.text_projection.data)
        g_final = _bias_slot(m.ln_final.bias)
        if g_final is not None:
            ops.bias_grad(dy, g_final)
        mean, rstd = ctx["stats"]
        drows = ops.layernorm_bwd(dy, ctx["rows"], m.ln_final.weight.data, mean, rstd)
        # only the EOT row of each caption carries gradient (jclip/model.py:213-214)
        if ctx.get("pack") is not None:
            plan, R = ctx["pack"]
            dx = self.txt.backward_packed(drows, ctx["idx"], plan, R, n, ctx["saved"], ctx["seed"],
                                          stop_at_input=not ctx["has_ctx"], seq=seq, row0=ctx["row0"], grad_lo=ctx["lo"],
                                          saved_packed=ctx["pack_fwd"])
        elif ctx["one_row"]:
            dx = self.txt.backward_sparse(drows, ctx["idx"], n, ctx["saved"], ctx["seed"], stop_at_input=not ctx["has_ctx"],
                                          seq=seq, row0=ctx["row0"], grad_lo=ctx["lo"])
        else:
            dx = ops.scatter_rows(drows, ctx["idx"], seq)
            self.txt.backward(dx, n, ctx["saved"], ctx["seed"], stop_at_input=not ctx["has_ctx"], seq=seq, row0=ctx["row0"],
                              grad_lo=ctx["lo"])
        if ctx["has_ctx"]:
            assert dctx_slot is not None
            ops.token_rows_grad(dx, dctx_slot, n, seq, 1)


# ------------------------------------------------------------------------------------------------
# autograd plumbing for the drop-in API (encode_image / encode_text return differentiable tensors)
# ------------------------------------------------------------------------------------------------

def _tower_trainables(tower_mod) -> List[Tuple[torch.nn.Parameter, torch.Tensor]]:
    """(parameter, gradient-slot view) pairs of the LoRA adapters of one tower."""
    out = []
    for blk in tower_mod.resblocks:
        a = blk.attn
        if getattr(a, "is_lora_mha", False):
            out.extend(a.trainable_pairs())
        for _, m in _mlp_adapters(blk):
            for q in (m.w_lora_A, m.w_lora_B):
                if q.requires_grad:
                    _ensure_slot(q)
                    out.append((q, q.grad_slot))
    return out


def _block_biases(tower_mod) -> List[torch.nn.Parameter]:
    """Every bias parameter of a tower's blocks (LoRA blocks: the q / k / v views of the packed in-projection bias)."""
    return [p for blk in tower_mod.resblocks for p in _blk_biases(blk)]


def _is_resnet(visual) -> bool:
    return bool(getattr(visual, "is_modified_resnet", False))


def image_biases(model) -> List[torch.nn.Parameter]:
    v = model.visual
    if _is_resnet(v):  # a frozen trunk: none of its biases is reachable by the fused backward
        return []
    return [v.ln_pre.bias] + _block_biases(v.transformer) + [v.ln_post.bias]


def text_biases(model) -> List[torch.nn.Parameter]:
    return _block_biases(model.transformer) + [model.ln_final.bias]


def _bias_pairs(biases) -> List[Tuple[torch.nn.Parameter, torch.Tensor]]:
    """(bias, gradient slot) of the trainable ones; a slot is attached where none is yet (autograd route)."""
    out = []
    for p in biases:
        if p is not None and p.requires_grad:
            _ensure_slot(p)
            out.append((p, p.grad_slot))
    return out


def deep_prompts(tower_mod) -> List[torch.nn.Parameter]:
    """The deep prompts of a tower's blocks (``resblocks[i].VPT_shallow``), block order."""
    return [blk.VPT_shallow for blk in tower_mod.resblocks if getattr(blk, "VPT_shallow", None) is not None]


def _image_trainables(model):
    if _is_resnet(model.visual):
        return []
    return (_tower_trainables(model.visual.transformer) + _bias_pairs(image_biases(model))
            + _bias_pairs(deep_prompts(model.visual.transformer)))


def _text_trainables(model):
    return (_tower_trainables(model.transformer) + _bias_pairs(text_biases(model))
            + _bias_pairs(deep_prompts(model.transformer)))


def _zero_slots(pairs):
    for _, g in pairs:
        g.zero_()


class _EncodeImage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, images, *params):
        eng = model.engine
        train = model.training
        seed = eng.next_seed() if train else 0
        feat, c = eng.vit_forward(images, True, seed, own_saved=True)
        ctx.model, ctx.c = model, c
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        model = ctx.model
        pairs = _image_trainables(model)
        _zero_slots(pairs)
        v = model.visual
        if v.VPT is not None:
            v.VPT.grad_slot.zero_()
        model.engine.vit_backward(ctx.c, dfeat.contiguous())
        grads = [g.clone() for _, g in pairs]
        if v.VPT is not None:
            grads.append(v.VPT.grad_slot.clone())
        return (None, None, *grads)


class _EncodeText(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, ids, prompt_ctx, *params):
        eng = model.engine
        seed = eng.next_seed() if model.training else 0
        feat, c = eng.text_forward(ids, prompt_ctx, True, seed, own_saved=True)
        ctx.model, ctx.c, ctx.prompt = model, c, prompt_ctx
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        model = ctx.model
        pairs = _text_trainables(model)
        _zero_slots(pairs)
        slot = None
        if ctx.prompt is not None:
            slot = torch.zeros_like(ctx.prompt.data)
        model.engine.text_backward(ctx.c, dfeat.contiguous(), slot)
        return (None, None, slot, *[g.clone() for _, g in pairs])


def encode_image(model, images: torch.Tensor) -> torch.Tensor:
    """Image features; differentiable with respect to the image tower's adapters / prompts where it has any.  A
    ModifiedResNet tower has none: its features come from the no-grad route, without a graph."""
    images = images.to(device=model.device, dtype=torch.float32)
    pairs = _image_trainables(model)
    params = [p for p, _ in pairs]
    if model.visual.VPT is not None:
        _ensure_slot(model.visual.VPT)
        params.append(model.visual.VPT)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        model.engine.refuse_merged("encode_image with trainable parameters")
        return _EncodeImage.apply(model, images, *params)
    # no-grad route: dropout still follows model.training (reference: a second encode_image under jt.no_grad() in
    # train mode, slow_pace.py:1612,1659-1661, is dropout-on)
    feat, _ = model.engine.vit_forward(images, False, model.engine.next_seed() if model.training else 0)
    return feat


@torch.no_grad()
def encode_image_tokens(model, images: torch.Tensor, with_class: bool = False):
    """Local image features [B, P, embed]: every patch row of a ViT tower through ln_post and proj (the class row and
    the VPT rows are dropped), without a graph, in any precision mode.  ``with_class``: (tokens, class-row feature
    [B, embed]) -- the feature ``encode_image`` returns.  Dropout follows model.training, as in ``encode_image``'s no-grad
    route.  A ModifiedResNet tower is refused."""
    images = images.to(device=model.device, dtype=torch.float32)
    tokens, cls = model.engine.vit_tokens(images, model.engine.next_seed() if model.training else 0)
    return (tokens, cls) if with_class else tokens


def encode_text(model, ids: torch.Tensor, prompt_ctx: Optional[torch.Tensor] = None) -> torch.Tensor:
    pairs = _text_trainables(model)
    params = [p for p, _ in pairs]
    needs = any(p.requires_grad for p in params) or (prompt_ctx is not None and prompt_ctx.requires_grad)
    if torch.is_grad_enabled() and needs:
        model.engine.refuse_merged("encode_text with trainable parameters")
        return _EncodeText.apply(model, ids, prompt_ctx, *params)
    feat, _ = model.engine.text_forward(ids, prompt_ctx, False, model.engine.next_seed() if model.training else 0)
    return feat


def _ensure_slot(p: torch.nn.Parameter) -> None:
    if getattr(p, "grad_slot", None) is None or p.grad_slot.shape != p.shape:
        p.grad_slot = torch.zeros_like(p.data)


@torch.no_grad()
def clip_logits(model, image, text):
    """CLIP.execute (jclip/model.py:217-232): logit_scale.exp() * norm(img) @ norm(txt)^T."""
    fi = ops.l2norm_fwd(encode_image(model, image))
    ft = ops.l2norm_fwd(encode_text(model, text))
    li = ops.gemm_nt(fi, ft, alpha=float(model.logit_scale.data.exp().item()))
    return li, li.t()


# ------------------------------------------------------------------------------------------------
# differentiable head ops (each backed by a HIP kernel pair)
# ------------------------------------------------------------------------------------------------

class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y, inv = ops.l2norm_fwd(x.contiguous(), save_inv=True)
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        return ops.l2norm_bwd(dy.contiguous(), y, inv)


class _CosineLogits(torch.autograd.Function):
    """scale * a @ b^T, a [M,d], b [C,d]."""

    @staticmethod
    def forward(ctx, a, b, scale):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        ctx.scale = scale
        return ops.gemm_nt(a, b, alpha=scale)

    @staticmethod
    def backward(ctx, dl):
        a, b = ctx.saved_tensors
        dl = dl.contiguous()
        M, d = a.shape
        Cn = b.shape[0]
        da = ops.matmul_small(dl, b, M, d, Cn, Cn, 1, d, 1, ctx.scale)
        db = ops.matmul_small(dl, a, Cn, d, M, 1, Cn, d, 1, ctx.scale)
        return da, db, None


class _ClassMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, classes, templates):
        emb = emb.contiguous()
        ctx.save_for_backward(emb)
        ctx.dims = (classes, templates)
        return ops.class_mean_fwd(emb, classes, templates)

    @staticmethod
    def backward(ctx, dout):
        (emb,) = ctx.saved_tensors
        return ops.class_mean_bwd(emb, dout.contiguous(), *ctx.dims), None, None


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss_sum, dl, _ = ops.cross_entropy(logits.contiguous(), target, True, 1.0)
        ctx.save_for_backward(dl)
        return (loss_sum / logits.shape[0]).reshape(())

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None


def l2_normalize(x):
    return _L2Norm.apply(x)


def cosine_logits(a, b, scale=100.0):
    return _CosineLogits.apply(a, b, scale)


def class_mean(emb, classes, templates):
    return _ClassMean.apply(emb, classes, templates)


def cross_entropy_loss(logits, target):
    return _CrossEntropy.apply(logits, target.to(logits.device).long())
