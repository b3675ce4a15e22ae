"""Frozen ResNet-50 feature extractor of the MoCo-v3 auxiliary branch (reference: ``load_moco`` slow_pace.py:1237-1271,
which builds ``jittor.models.resnet.resnet50`` -- torchvision's ResNet-50 v1.5, stride on the 3x3 convolution -- loads the
MoCo-v3 ``base_encoder.*`` weights and replaces ``fc`` by Identity; used forward-only at :1158,1677,1013,1099).

Execution on the HIP engine: activations NHWC; every convolution is one fp32-MFMA GEMM (csrc/gemm.hip) -- a 1x1 /
stride-1 convolution directly on the activation tensor, the others on an im2col matrix (csrc/resnet.hip) -- with the
BatchNorm of inference mode folded into weight and bias ONCE at load time and bias + residual + ReLU in the GEMM epilogue.

Flagged deviation: BatchNorm always uses the RUNNING statistics (a frozen feature extractor; ``moco_model.eval()`` is what
test.py:1828 and evaluate_lora :950 set).  The reference's training script never calls ``moco_model.eval()`` before its
first epoch, so there Jittor's default training flag makes the first epoch (and pre_load_features_moco) use batch
statistics -- an accident of the script, not reproduced.  Pretrained weights (r-50-1000ep.pkl) are not available
offline: parity is the oracle's (oracle/clip_oracle.py: resnet50_forward) on synthetic weights, i.e. unpinned against
Jittor like the rest of the path.

``ClipResNet`` below is the image tower of CLIP's own RN50 family (``ModifiedResNet``) on the same machinery; its
docstring lists what differs, and flags the same BatchNorm deviation: running statistics, folded once at load, although
the reference calls ``clip_model.train()`` every epoch.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from . import _lib, ops
from ._lib import check

LAYERS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def fold_conv_bn(sd: Dict[str, torch.Tensor], conv: str, bn: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inference-mode BatchNorm folded into its convolution, in fp64: (weight [Cout, Kp] in (ky, kx, cin) column order with
    Kp = kh * kw * cin rounded up to a multiple of 4 and the tail zero, bias [Cout]), so that bn(conv(x)) = col(x) @ weight.T
    + bias for the im2col matrix of csrc/resnet.hip."""
    w = sd[conv + ".weight"].to(torch.float64)
    cout, cin, kh, kw = w.shape
    g, b = sd[bn + ".weight"].double(), sd[bn + ".bias"].double()
    mu, var = sd[bn + ".running_mean"].double(), sd[bn + ".running_var"].double()
    scale = g / torch.sqrt(var + BN_EPS)
    w = (w * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(cout, kh * kw * cin)
    k = kh * kw * cin
    kp = (k + 3) // 4 * 4
    if kp != k:
        w = torch.cat([w, torch.zeros(cout, kp - k, dtype=w.dtype, device=w.device)], dim=1)
    return w, b - mu * scale


class _Conv:
    """One convolution + folded BatchNorm as a GEMM operand: weight [Cout, Kp] in (ky, kx, cin) column order."""

    def __init__(self, sd: Dict[str, torch.Tensor], conv: str, bn: str, stride: int, pad: int, device):
        cout, cin, kh, kw = sd[conv + ".weight"].shape
        w, b = fold_conv_bn(sd, conv, bn)
        self.kp = w.shape[1]
        self.weight = w.float().contiguous().to(device)
        self.bias = b.float().contiguous().to(device)
        self.cin, self.cout, self.kh, self.kw, self.stride, self.pad = cin, cout, kh, kw, stride, pad

    def __call__(self, x: torch.Tensor, shape: Tuple[int, int, int], relu: bool, residual=None):
        """x [N*H*W, cin] (NHWC rows), shape = (N, H, W) -> (y [N*Ho*Wo, cout], (N, Ho, Wo))"""
        n, h, w = shape
        ho = (h + 2 * self.pad - self.kh) // self.stride + 1
        wo = (w + 2 * self.pad - self.kw) // self.stride + 1
        if self.kh == 1 and self.kw == 1 and self.stride == 1 and self.pad == 0:
            a = x
        else:
            a = torch.empty(n * ho * wo, self.kp, device=x.device, dtype=torch.float32)
            check(_lib.load().clipfs_im2col_nhwc(x.data_ptr(), a.data_ptr(), n, h, w, self.cin, self.kh, self.kw, self.stride,
                                                 self.pad, self.kp, _stream()), "im2col_nhwc")
        y = ops.gemm_nt(a, self.weight, bias=self.bias, residual=residual, act=3 if relu else 0)
        return y, (n, ho, wo)


class MocoResNet50:
    """``model, feat_dim = load_moco(path)``: callable on NORMALISED images [B, 3, H, W] (``tfm_moco``), returns the
    2048-d pooled features (``model.fc`` = Identity, slow_pace.py:1269-1270).  Forward only (the branch is frozen)."""

    feat_dim = 2048

    def __init__(self, state_dict: Dict[str, torch.Tensor], device):
        self.device = torch.device(device)
        sd = state_dict
        self.conv1 = _Conv(sd, "conv1", "bn1", 2, 3, self.device)
        self.blocks: List[dict] = []
        inplanes = 64
        for li, (nb, planes) in enumerate(zip(LAYERS, PLANES)):
            for bi in range(nb):
                stride = 2 if (bi == 0 and li > 0) else 1
                p = f"layer{li + 1}.{bi}"
                blk = {"c1": _Conv(sd, p + ".conv1", p + ".bn1", 1, 0, self.device),
                       "c2": _Conv(sd, p + ".conv2", p + ".bn2", stride, 1, self.device),
                       "c3": _Conv(sd, p + ".conv3", p + ".bn3", 1, 0, self.device), "down": None}
                if bi == 0:
                    blk["down"] = _Conv(sd, p + ".downsample.0", p + ".downsample.1", stride, 0, self.device)
                self.blocks.append(blk)
                inplanes = planes * 4
        self.training = False

    def eval(self):
        return self

    def train(self, mode: bool = True):  # BatchNorm statistics are frozen (module docstring)
        return self

    @torch.no_grad()
    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        x = images.to(self.device, torch.float32).contiguous()
        assert x.dim() == 4 and x.shape[1] == 3, "images: [B, 3, H, W]"
        n, _, h, w = x.shape
        lib = _lib.load()
        xh = torch.empty(n * h * w, 3, device=self.device, dtype=torch.float32)
        check(lib.clipfs_nchw_to_nhwc(x.data_ptr(), xh.data_ptr(), n, 3, h, w, _stream()), "nchw_to_nhwc")
        y, shp = self.conv1(xh, (n, h, w), relu=True)
        n, h, w = shp
        ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        p = torch.empty(n * ho * wo, 64, device=self.device, dtype=torch.float32)
        check(lib.clipfs_maxpool3x3s2_nhwc(y.data_ptr(), p.data_ptr(), n, h, w, 64, _stream()), "maxpool")
        x, shp = p, (n, ho, wo)
        for blk in self.blocks:
            idn = x
            y, s1 = blk["c1"](x, shp, relu=True)
            y, s2 = blk["c2"](y, s1, relu=True)
            if blk["down"] is not None:
                idn, _ = blk["down"](x, shp, relu=False)
            x, shp = blk["c3"](y, s2, relu=True, residual=idn)  # relu(bn3(conv3) + identity)
        n, h, w = shp
        out = torch.empty(n, x.shape[1], device=self.device, dtype=torch.float32)
        check(lib.clipfs_global_avgpool_nhwc(x.data_ptr(), out.data_ptr(), n, h * w, x.shape[1], _stream()), "avgpool")
        return out

    forward = execute = __call__


class ClipResNet:
    """The image tower of CLIP's RN50 family (``ModifiedResNet``, jclip/model_res.py:84-170 = the published CLIP class) on
    the same machinery as ``MocoResNet50``: NHWC activations, every convolution one fp32-MFMA GEMM with the BatchNorm folded
    at load and bias + residual + ReLU in the epilogue.  What differs from torchvision's ResNet:

    * a three-convolution stem (3x3 stride 2, 3x3, 3x3; each BN + ReLU) followed by a 2x2 MEAN pool;
    * no strided convolution after the stem: a bottleneck with stride s > 1 mean-pools s x s before ``conv3`` and before the
      1x1 convolution of its identity branch (csrc/resnet.hip: avgpool_nhwc; sizes floored, no padding).  The pooled tensor
      IS the A operand of the 1x1 GEMM -- no im2col;
    * the attention-pool head instead of the global mean: tokens ``[mean over HW ; x] + positional_embedding``, one
      multi-head attention (head width 64, scale 1/8) whose ONLY query is token 0, then ``c_proj``.  Here: one kernel builds
      the tokens in a single pass, one GEMM gives k | v for every token (``k_proj`` / ``v_proj`` stacked once at load), one
      GEMM gives q for token 0 alone, one wave per (image, head) attends, one GEMM applies ``c_proj``.  Queries of the
      other tokens are never computed.

    ``state_dict``: the ``visual.*`` tensors of a CLIP checkpoint under their published names, with or without the
    ``visual.`` prefix; ``num_batches_tracked`` entries are ignored.  Layer counts, width and grid come from the shapes.

    Forward only, under ``torch.no_grad()``; fp32 in EVERY engine precision mode (the trunk is frozen and there is no
    bf16x3 / fp16 path for the convolutions: ``Engine.precision`` touches the text tower only).

    Flagged deviations.  (1) BatchNorm always uses the RUNNING statistics, folded once at load -- the same deviation as the
    MoCo branch (module docstring): the reference calls ``clip_model.train()`` every epoch, which would put a frozen trunk's
    BatchNorm on batch statistics.  (2) The reference's port of the head (model_res.py:65-82) feeds the three projected
    tensors into a second ``jittor.attention.MultiheadAttention`` whose in / out projections no checkpoint carries; this is
    the published semantics (what the checkpoints' weights mean), not that quirk."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device):
        self.device = torch.device(device)
        sd = strip_visual_prefix(state_dict)
        self.layers = clip_resnet_layers(sd)
        self.width = int(sd["layer1.0.conv1.weight"].shape[0])
        pos = sd["attnpool.positional_embedding"]
        self.grid = round((pos.shape[0] - 1) ** 0.5)
        if self.grid * self.grid + 1 != pos.shape[0]:
            raise ValueError(f"attnpool.positional_embedding has {pos.shape[0]} rows: not a square grid plus the mean token")
        self.input_resolution = 32 * self.grid
        self.embed = int(pos.shape[1])
        if self.embed != 32 * self.width or self.embed % 64:
            raise ValueError(f"attention pool width {self.embed} is not 32 x the trunk width {self.width} (heads of 64)")
        self.heads = self.embed // 64
        self.stem = [_Conv(sd, "conv1", "bn1", 2, 1, self.device), _Conv(sd, "conv2", "bn2", 1, 1, self.device),
                     _Conv(sd, "conv3", "bn3", 1, 1, self.device)]
        self.blocks: List[dict] = []
        for li, nb in enumerate(self.layers):
            for bi in range(nb):
                p = f"layer{li + 1}.{bi}"
                blk = {"c1": _Conv(sd, p + ".conv1", p + ".bn1", 1, 0, self.device),
                       "c2": _Conv(sd, p + ".conv2", p + ".bn2", 1, 1, self.device),
                       "c3": _Conv(sd, p + ".conv3", p + ".bn3", 1, 0, self.device),
                       "stride": 2 if (bi == 0 and li > 0) else 1, "down": None}
                if p + ".downsample.0.weight" in sd:  # stride > 1 or a change of width (model_res.py:101-106)
                    blk["down"] = _Conv(sd, p + ".downsample.0", p + ".downsample.1", 1, 0, self.device)
                self.blocks.append(blk)

        def dev(name):
            return sd[name].detach().to(self.device, torch.float32).contiguous()

        self.pos = dev("attnpool.positional_embedding")
        self.q_w, self.q_b = dev("attnpool.q_proj.weight"), dev("attnpool.q_proj.bias")
        self.kv_w = torch.cat([dev("attnpool.k_proj.weight"), dev("attnpool.v_proj.weight")], dim=0).contiguous()
        self.kv_b = torch.cat([dev("attnpool.k_proj.bias"), dev("attnpool.v_proj.bias")], dim=0).contiguous()
        self.c_w, self.c_b = dev("attnpool.c_proj.weight"), dev("attnpool.c_proj.bias")
        self.output_dim = int(self.c_w.shape[0])
        self.training = False

    def eval(self):
        return self

    def train(self, mode: bool = True):  # BatchNorm statistics are frozen (class docstring)
        return self

    def _pool(self, x: torch.Tensor, shape: Tuple[int, int, int], k: int):
        n, h, w = shape
        c = x.shape[1]
        y = torch.empty(n * (h // k) * (w // k), c, device=self.device, dtype=torch.float32)
        check(_lib.load().clipfs_avgpool_nhwc(x.data_ptr(), y.data_ptr(), n, h, w, c, k, _stream()), "avgpool_nhwc")
        return y, (n, h // k, w // k)

    def trunk(self, images: torch.Tensor):
        """images [B, 3, R, R] -> (x [B * g * g, 32 * width] NHWC rows, (B, g, g))"""
        x = images.to(self.device, torch.float32).contiguous()
        assert x.dim() == 4 and x.shape[1] == 3, "images: [B, 3, H, W]"
        n, _, h, w = x.shape
        if h != self.input_resolution or w != self.input_resolution:  # the positional embedding fixes the grid
            raise ValueError(f"expected images [B,3,{self.input_resolution},{self.input_resolution}], got {tuple(x.shape)}")
        xh = torch.empty(n * h * w, 3, device=self.device, dtype=torch.float32)
        check(_lib.load().clipfs_nchw_to_nhwc(x.data_ptr(), xh.data_ptr(), n, 3, h, w, _stream()), "nchw_to_nhwc")
        x, shp = xh, (n, h, w)
        for conv in self.stem:
            x, shp = conv(x, shp, relu=True)
        x, shp = self._pool(x, shp, 2)
        for blk in self.blocks:
            s = blk["stride"]
            y, s1 = blk["c1"](x, shp, relu=True)
            y, s2 = blk["c2"](y, s1, relu=True)
            if s > 1:
                y, s2 = self._pool(y, s2, s)
            idn = x
            if blk["down"] is not None:
                xi, si = self._pool(x, shp, s) if s > 1 else (x, shp)
                idn, _ = blk["down"](xi, si, relu=False)
            x, shp = blk["c3"](y, s2, relu=True, residual=idn)  # relu(bn3(conv3) + identity)
        return x, shp

    def head(self, x: torch.Tensor, shape: Tuple[int, int, int]) -> torch.Tensor:
        """x [N * HW, C] -> [N, output_dim]: the attention pool (class docstring)."""
        n, h, w = shape
        hw, c = h * w, self.embed
        ln = hw + 1
        assert ln == self.pos.shape[0] and x.shape[1] == c
        lib = _lib.load()
        tok = torch.empty(n * ln, c, device=self.device, dtype=torch.float32)
        check(lib.clipfs_attnpool_tokens(x.data_ptr(), self.pos.data_ptr(), tok.data_ptr(), n, hw, c, _stream()),
              "attnpool_tokens")
        kv = ops.gemm_nt(tok, self.kv_w, bias=self.kv_b)
        q = _gemm_nt_rows(tok, n, ln * c, self.q_w, self.q_b)  # token 0 of every image: rows ln * c floats apart
        o = torch.empty(n, c, device=self.device, dtype=torch.float32)
        check(lib.clipfs_attnpool_attend(q.data_ptr(), kv.data_ptr(), o.data_ptr(), n, ln, self.heads, _stream()),
              "attnpool_attend")
        return ops.gemm_nt(o, self.c_w, bias=self.c_b)

    @torch.no_grad()
    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        return self.head(*self.trunk(images))

    forward = execute = __call__


def _gemm_nt_rows(a: torch.Tensor, rows: int, lda: int, b: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """out [rows, N] = A @ b.T + bias where row i of A is the first K floats at ``a + i * lda`` (``ops.gemm_nt`` takes
    dense operands only; the GEMM itself takes any leading dimension)."""
    import ctypes as C
    nn_, k = b.shape
    assert a.dtype == torch.float32 and a.is_contiguous() and a.numel() >= (rows - 1) * lda + k
    out = torch.empty(rows, nn_, device=b.device, dtype=torch.float32)
    g = _lib.new_gemm_args()
    g.A, g.B, g.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    g.M, g.N, g.K = rows, nn_, k
    g.lda, g.ldb, g.ldc = lda, k, nn_
    g.alpha = 1.0
    g.bias = bias.data_ptr()
    g.ldres = nn_
    check(_lib.load().clipfs_gemm_nt(C.byref(g), _stream()), "gemm_nt")
    return out


def strip_visual_prefix(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The image tower's tensors of a CLIP state dict without their ``visual.`` prefix (a dict that has no such key is
    taken to be the tower's own); BatchNorm's ``num_batches_tracked`` counters are dropped."""
    if any(k.startswith("visual.") for k in state_dict):
        state_dict = {k[len("visual."):]: v for k, v in state_dict.items() if k.startswith("visual.")}
    return {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}


def clip_resnet_layers(sd: Dict[str, torch.Tensor], prefix: str = "") -> Tuple[int, int, int, int]:
    """Blocks per stage from the ``layer{b}.{i}.*`` keys (model_res.py:316-319)."""
    return tuple(len({k[len(prefix):].split(".")[1] for k in sd if k.startswith(f"{prefix}layer{b}.")}) for b in (1, 2, 3, 4))


def synth_clip_resnet_state_dict(layers=(3, 4, 6, 3), width: int = 64, resolution: int = 224, embed_dim: int = 1024,
                                 seed: int = 7, text=None) -> Dict[str, torch.Tensor]:
    """Random ModifiedResNet weights under the published CLIP key names (``visual.conv1.weight`` ...
    ``visual.attnpool.c_proj.bias``): kaiming-normal convolutions, perturbed BatchNorm affine and running statistics so that
    the folding is exercised, an int64 ``num_batches_tracked`` per BatchNorm (published checkpoints carry it; the loader
    ignores it), attention-pool weights with the statistics of CLIP.initialize_parameters (std = C ** -0.5) and small random
    biases.  ``text``: a ``synth.ClipConfig`` whose text tower (``embed_dim`` must agree) is added to make a whole CLIP
    state dict; None = the ``visual.*`` keys alone."""
    if resolution % 32:
        raise ValueError("resolution must be a multiple of 32")
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, cout, cin, k):
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5

    def bn(name, c):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.05 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 1.0 + 0.2 * torch.rand(c, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(1000, dtype=torch.int64)

    v = "visual."
    conv(v + "conv1", width // 2, 3, 3)
    bn(v + "bn1", width // 2)
    conv(v + "conv2", width // 2, width // 2, 3)
    bn(v + "bn2", width // 2)
    conv(v + "conv3", width, width // 2, 3)
    bn(v + "bn3", width)
    inplanes = width
    for li, nb in enumerate(layers):
        planes = width << li
        for bi in range(nb):
            p = f"{v}layer{li + 1}.{bi}"
            stride = 2 if (bi == 0 and li > 0) else 1
            conv(p + ".conv1", planes, inplanes, 1)
            bn(p + ".bn1", planes)
            conv(p + ".conv2", planes, planes, 3)
            bn(p + ".bn2", planes)
            conv(p + ".conv3", planes * 4, planes, 1)
            bn(p + ".bn3", planes * 4)
            if stride > 1 or inplanes != planes * 4:
                conv(p + ".downsample.0", planes * 4, inplanes, 1)
                bn(p + ".downsample.1", planes * 4)
            inplanes = planes * 4
    c = width * 32
    grid = resolution // 32
    sd[v + "attnpool.positional_embedding"] = torch.randn(grid * grid + 1, c, generator=g) / c ** 0.5
    for name, out in (("q_proj", c), ("k_proj", c), ("v_proj", c), ("c_proj", embed_dim)):
        sd[f"{v}attnpool.{name}.weight"] = torch.randn(out, c, generator=g) * c ** -0.5
        sd[f"{v}attnpool.{name}.bias"] = 0.02 * torch.randn(out, generator=g)
    if text is not None:
        from . import synth
        if text.embed_dim != embed_dim:
            raise ValueError(f"text tower embeds to {text.embed_dim}, the image tower to {embed_dim}")
        sd.update({k: t for k, t in synth.synth_state_dict(text, seed=seed + 1, perturb=True).items()
                   if not k.startswith("visual.")})
    return sd


def strip_moco_prefix(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """slow_pace.py:1246-1261: ``base_encoder.X`` -> ``X`` (except ``base_encoder.fc*``); also accepts the
    ``module.base_encoder.`` prefix of the original MoCo-v3 checkpoints (moco.py:17-20)."""
    out = {}
    for k, v in state_dict.items():
        for pre in ("module.base_encoder.", "base_encoder."):
            if k.startswith(pre) and not k.startswith(pre + "fc"):
                out[k[len(pre):]] = v
                break
        else:
            out[k] = v
    return out


def synth_resnet50_state_dict(seed: int = 7) -> Dict[str, torch.Tensor]:
    """Random ResNet-50 weights with torchvision key names (kaiming-normal convolutions, perturbed BatchNorm affine and
    running statistics so that the folding is exercised).  The MoCo-v3 checkpoint is not available offline."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, cout, cin, k):
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5

    def bn(name, c):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.05 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 1.0 + 0.2 * torch.rand(c, generator=g)

    conv("conv1", 64, 3, 7)
    bn("bn1", 64)
    inplanes = 64
    for li, (nb, planes) in enumerate(zip(LAYERS, PLANES)):
        for bi in range(nb):
            p = f"layer{li + 1}.{bi}"
            conv(p + ".conv1", planes, inplanes, 1)
            bn(p + ".bn1", planes)
            conv(p + ".conv2", planes, planes, 3)
            bn(p + ".bn2", planes)
            conv(p + ".conv3", planes * 4, planes, 1)
            bn(p + ".bn3", planes * 4)
            if bi == 0:
                conv(p + ".downsample.0", planes * 4, inplanes, 1)
                bn(p + ".downsample.1", planes * 4)
            inplanes = planes * 4
    return sd
