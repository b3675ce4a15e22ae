"""Inputs far from the unit range, a plain torch yardstick and the acceptance rule of the range suites
(test_range_cases_cpu.py, test_attention_range_gpu.py, test_softmax_range_gpu.py).  torch only, no clipfs: this imports
and runs on a machine without a GPU.

Every other attention test draws qkv from a unit normal: with 64-wide heads and the 1/8 scale its scores are N(0, 1), the
largest near 4, the log-sum-exp near 5 -- a range at which a softmax without the row maximum, a running maximum that
starts at 0 or a forgotten online rescale are all right to the last bit of the fixed budgets.  The regimes here put the
scores where the product runs: tens to hundreds.

Acceptance follows the conditioning of the input instead of a fixed number: budget(floor, yard_err, want) is the family's
existing budget (the floor) or 8 x the error the SAME operation makes in plain fp32 torch against fp64 on these very
inputs, whichever is larger.  The 8 covers the kernels' other summation order and the 1-ulp hardware exp2; it is a margin
over the reference, never over the code under test, and it is capped at 1e-2 of the largest expected value so that it
cannot hide a failure: past the cap budget() raises."""
import functools

import torch

HD = 64  # head width of every attention kernel
ATTENTION_REGIMES = ("peaked", "shifted", "stairs")
LOGIT_REGIMES = ("peaked", "shifted", "confident")
MARGIN, CAP = 8.0, 1e-2


# ---- attention ----------------------------------------------------------------------------------------------------------
def attention_inputs(B, L, H, regime, seed):
    """(qkv [B*L, 3*H*64], dout [B*L, H*64]) in fp64, every value an f16 number, so the same tensors serve the fp32 and the
    f16 kernels exactly.  Feature 0 of a head is the carrier; everything else is a seeded unit normal.
      unit     nothing else: the inputs of the existing suites
      peaked   q, k x 4.5: scores of standard deviation ~20, lse 75 .. 100, a nearly one-hot softmax
      shifted  k[..., 0] += 100, q[..., 0] = +16 on even / -16 on odd query tokens: every score of a row moves by ~ +-200
      stairs   k[..., 0] = 0.5 j for key token j, q[..., 0] = +-8 as above: scores 0.5 j + noise, a new maximum in every
               later key tile on the even rows, the first tile holding it on the odd ones"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, 3, H, HD, generator=g, dtype=torch.float64)
    dout = torch.randn(B * L, H * HD, generator=g, dtype=torch.float64)
    sign = torch.where(torch.arange(L) % 2 == 0, 1.0, -1.0).double()[None, :, None]  # [1, L, 1]
    if regime == "peaked":
        x[:, :, :2] *= 4.5
    elif regime == "shifted":
        x[:, :, 1, :, 0] += 100.0
        x[:, :, 0, :, 0] = 16.0 * sign
    elif regime == "stairs":
        x[:, :, 1, :, 0] = 0.5 * torch.arange(L, dtype=torch.float64)[None, :, None]
        x[:, :, 0, :, 0] = 8.0 * sign
    elif regime != "unit":
        raise ValueError(regime)
    return x.reshape(B * L, 3 * H * HD).half().double(), dout.half().double()


def split_heads(qkv, B, L, H):
    """q, k, v as [B, H, L, 64] views of a [B*L, 3*H*64] tensor"""
    x = qkv.reshape(B, L, 3, H, HD)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def scores(qkv, B, L, H, causal):
    """masked scaled scores [B, H, L, L] in qkv's dtype"""
    q, k, _ = split_heads(qkv, B, L, H)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=s.dtype).triu(1)
    return s


def attention_ref(qkv, dout, B, L, H, causal, dtype, round_p=None):
    """(out [B*L, H*64], lse [B*H*L], dqkv) of plain attention evaluated in `dtype`: masked scores, lse = logsumexp,
    P = exp(s - lse), out = P v, gradients by autograd.  At fp64 it is the expected value, at fp32 the yardstick.
    round_p=torch.float16 rounds P to f16 with a straight-through gradient: the dominant rounding of the f16 kernels."""
    x = qkv.to(dtype).clone().requires_grad_()
    _, _, v = split_heads(x, B, L, H)
    s = scores(x, B, L, H, causal)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    if round_p is not None:
        p = p + (p.detach().to(round_p).to(dtype) - p.detach())
    out = (p @ v).permute(0, 2, 1, 3).reshape(B * L, H * HD)
    out.backward(dout.to(dtype))
    return out.detach(), lse.detach().reshape(-1), x.grad


def visible_value_range(qkv, B, L, H, causal):
    """(lo, hi) [B*L, H*64]: per feature the smallest and largest v among the rows each query sees.  out is a convex
    combination of those rows, whatever the scores."""
    v = qkv.reshape(B, L, 3, H * HD)[:, :, 2]
    if causal:
        lo, hi = torch.cummin(v, 1).values, torch.cummax(v, 1).values
    else:
        lo, hi = v.amin(1, keepdim=True).expand_as(v), v.amax(1, keepdim=True).expand_as(v)
    return lo.reshape(B * L, -1), hi.reshape(B * L, -1)


@functools.lru_cache(maxsize=None)
def attention_case(B, L, H, causal, regime, lens=None, round_p=None):
    """(qkv, dout, want, yard_err): the inputs, the fp64 (out, lse, dqkv) and the max abs errors of the fp32 yardstick on
    them (with P rounded to `round_p` if given); computed once per case, shared, never modified.  With `lens`, dout is
    zero on the dead rows of each caption (token t of caption c is dead iff t >= lens[c])."""
    qkv, dout = attention_inputs(B, L, H, regime, shape_seed(B, L, H, causal))
    if lens is not None:
        dout = dout * live_rows(L, lens)[:, None]
    want = attention_ref(qkv, dout, B, L, H, causal, torch.float64)
    yard = attention_ref(qkv, dout, B, L, H, causal, torch.float32, round_p)
    return qkv, dout, want, tuple(max_err(y, w) for y, w in zip(yard, want))


# ---- acceptance ---------------------------------------------------------------------------------------------------------
def max_err(got, want):
    """max abs error in fp64; inf if anything is not finite (NaN compares false everywhere, so it must not reach max())"""
    got = got.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float("inf")
    return (got - want.double()).abs().max().item()


def budget(floor, yard_err, want):
    """max(floor, 8 * yard_err): `floor` the existing budget of the family, `yard_err` the max abs error of the fp32 yardstick
    against fp64 on these very inputs.  Raises if the widened budget passes 1e-2 of the largest expected value.  Where
    8 * yard_err stays within the floor nothing is widened and the cap has nothing to limit: an expected tensor that is
    zero but for underflow (softmax - onehot of a row whose other classes are e^-120) has no scale to be 1e-2 of, and is
    held to the floor as before."""
    wide = MARGIN * yard_err
    top = want.abs().max().item()
    if not (wide <= floor or wide <= CAP * top):
        raise AssertionError(f"the yardstick itself is off by {yard_err:.3e}: 8 x that is past {CAP:g} of max |want| = {top:.3e}, "
                             "a budget that wide would hide a failure")
    return max(floor, wide)


def accepts(got, want, floor, yard_err):
    return max_err(got, want) <= budget(floor, yard_err, want)


# ---- row-softmax kernels ------------------------------------------------------------------------------------------------
def logit_inputs(rows, C, regime, seed, winner_shift=0):
    """logits [rows, C] in fp64, every value an fp32 number.
      peaked     standard deviation 30
      shifted    unit normal + 300 on even rows, - 300 on odd rows
      confident  unit normal, class (3 r + 1 + winner_shift) % C of row r is 120 above its value: every other probability
                 underflows to 0 in fp32"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, C, generator=g, dtype=torch.float64)
    if regime == "peaked":
        z = z * 30.0
    elif regime == "shifted":
        z = z + torch.where(torch.arange(rows) % 2 == 0, 300.0, -300.0).double()[:, None]
    elif regime == "confident":
        z[torch.arange(rows), confident_winner(rows, C, winner_shift)] += 120.0
    elif regime != "unit":
        raise ValueError(regime)
    return z.float().double()


def confident_winner(rows, C, winner_shift=0):
    return (3 * torch.arange(rows) + 1 + winner_shift) % C


# ---- the shapes of test_attention_range_gpu.py: (B, L, H, causal), the smallest that reach each kernel instance ----------
MFMA16_SHAPES = [((2, 16, 1, True), 1), ((2, 50, 2, False), 4), ((2, 77, 2, True), 5), ((1, 96, 2, False), 6)]  # with nt
MFMA32_SHAPES = [(1, 97, 1, False), (1, 130, 1, True), (1, 288, 1, True)]
MFMA_LONG_SHAPES = [(1, 289, 1, True), (1, 330, 2, False)]
STREAM_MISALIGNED_SHAPES = [(2, 50, 2, True), (1, 130, 1, False)]
STREAM_DEFAULT_SHAPE = (1, 1025, 1, True)
RECOMPUTE_SHAPES = [((3, 31, 1, True), 64), ((1, 65, 2, False), 80), ((2, 96, 2, True), 96)]  # with lmax
F16_SHORT_SHAPES = [(3, 50, 2, False), (3, 77, 2, True), (1, 288, 1, False)]
F16_LONG_SHAPES = [(1, 289, 1, True), (1, 330, 2, False)]
PACKED_SEQ, PACKED_HEADS, PACKED_LENS = 77, 2, (2, 17, 40, 77)  # one batch of four captions, causal
FP32_SHAPES = sorted(set([s for s, _ in MFMA16_SHAPES] + MFMA32_SHAPES + MFMA_LONG_SHAPES + STREAM_MISALIGNED_SHAPES
                         + [STREAM_DEFAULT_SHAPE] + [s for s, _ in RECOMPUTE_SHAPES]))
F16_SHAPES = F16_SHORT_SHAPES + F16_LONG_SHAPES


def shape_seed(B, L, H, causal):
    return 1000 * L + 10 * H + B + (500 if causal else 0)


def live_rows(seq=PACKED_SEQ, lens=PACKED_LENS):
    """bool [len(lens) * seq]: token t of caption c is live iff t < lens[c]"""
    return (torch.arange(seq)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
