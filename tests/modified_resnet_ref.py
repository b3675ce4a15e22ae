"""fp64 restatement of CLIP's ModifiedResNet image tower in plain ``torch.nn.functional`` (test infrastructure, like
oracle/clip_oracle.py for the rest of the model; the text side keeps using that oracle).

Restated from the reference's jclip/model_res.py -- Bottleneck :84-121, ModifiedResNet :123-170, hyper-parameters from
shapes :316-331 -- which equals the published CLIP class.  Two deliberate differences from what the reference executes,
both flagged in clipfs/resnet.py (ClipResNet):

* BatchNorm uses the running statistics (inference mode);
* the attention pool is the PUBLISHED one (tokens [mean ; x] + positional_embedding, one multi-head attention with
  q_proj / k_proj / v_proj / c_proj, head width 64, the output at token 0), not the port of model_res.py:65-82, which
  runs a second MultiheadAttention with projections no checkpoint carries.

The geometries of the tests live here too, so that the CPU and the GPU tests share them."""
from collections import namedtuple

import torch
import torch.nn.functional as F

Geometry = namedtuple("Geometry", "layers width resolution embed text")

BN_EPS = 1e-5


def geometries():
    from clipfs import synth
    return {"RN_TINY": Geometry((1, 1, 1, 1), 16, 64, 64, synth.TINY),
            "RN_SMALL": Geometry((2, 1, 2, 1), 32, 96, 128, synth.SMALL)}


def synth_sd(geo: Geometry, seed: int = 7):
    from clipfs import resnet
    return resnet.synth_clip_resnet_state_dict(geo.layers, geo.width, geo.resolution, geo.embed, seed=seed, text=geo.text)


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def layer_counts(sd):
    """model_res.py:316-319"""
    return tuple(len({k.split(".")[2] for k in sd if k.startswith(f"visual.layer{b}.")}) for b in (1, 2, 3, 4))


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                        training=False, eps=BN_EPS)


def bottleneck(sd, p, x, stride):
    """model_res.py:108-121"""
    out = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"])))
    out = F.relu(_bn(sd, p + ".bn2", F.conv2d(out, sd[p + ".conv2.weight"], padding=1)))
    if stride > 1:
        out = F.avg_pool2d(out, stride)
    out = _bn(sd, p + ".bn3", F.conv2d(out, sd[p + ".conv3.weight"]))
    identity = x
    if p + ".downsample.0.weight" in sd:
        if stride > 1:
            identity = F.avg_pool2d(identity, stride)
        identity = _bn(sd, p + ".downsample.1", F.conv2d(identity, sd[p + ".downsample.0.weight"]))
    return F.relu(out + identity)


def trunk(sd, x):
    """model_res.py:156-167: x [B, 3, R, R] -> [B, 32 w, R/32, R/32]"""
    v = "visual."
    x = F.relu(_bn(sd, v + "bn1", F.conv2d(x, sd[v + "conv1.weight"], stride=2, padding=1)))
    x = F.relu(_bn(sd, v + "bn2", F.conv2d(x, sd[v + "conv2.weight"], padding=1)))
    x = F.relu(_bn(sd, v + "bn3", F.conv2d(x, sd[v + "conv3.weight"], padding=1)))
    x = F.avg_pool2d(x, 2)
    for li, nb in enumerate(layer_counts(sd)):
        for bi in range(nb):
            x = bottleneck(sd, f"{v}layer{li + 1}.{bi}", x, 2 if (bi == 0 and li > 0) else 1)
    return x


def attention(q, k, v):
    """q [N, H, 64], k / v [N, L, H, 64] -> [N, H, 64]: softmax(q . k / 8) . v per (image, head)"""
    s = torch.einsum("nhd,nlhd->nhl", q, k) / 8.0
    return torch.einsum("nhl,nlhd->nhd", torch.softmax(s, dim=-1), v)


def attnpool_tokens(x, pos):
    """x [N, HW, C] -> [N, HW + 1, C]"""
    return torch.cat([x.mean(dim=1, keepdim=True), x], dim=1) + pos[None]


def attnpool(sd, x):
    """x [B, C, g, g] -> [B, embed]; heads = C / 64 (model_res.py:228 with C = 32 w)"""
    p = "visual.attnpool."
    n, c = x.shape[:2]
    tok = attnpool_tokens(x.flatten(2).permute(0, 2, 1), sd[p + "positional_embedding"])
    heads = c // 64
    q = F.linear(tok[:, 0], sd[p + "q_proj.weight"], sd[p + "q_proj.bias"]).reshape(n, heads, 64)
    k = F.linear(tok, sd[p + "k_proj.weight"], sd[p + "k_proj.bias"]).reshape(n, -1, heads, 64)
    v = F.linear(tok, sd[p + "v_proj.weight"], sd[p + "v_proj.bias"]).reshape(n, -1, heads, 64)
    o = attention(q, k, v).reshape(n, c)
    return F.linear(o, sd[p + "c_proj.weight"], sd[p + "c_proj.bias"])


def image_features(sd, images):
    """sd: fp64 state dict with the ``visual.*`` keys; images [B, 3, R, R] fp64"""
    return attnpool(sd, trunk(sd, images))
