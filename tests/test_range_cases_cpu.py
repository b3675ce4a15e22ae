"""The range suites have teeth (CPU only): the acceptance rule of range_cases.py, applied to deliberately wrong fp32
restatements of attention written in torch, rejects each of them in at least one regime -- and the existing fixed budgets
on unit-normal inputs accept the first two, which is the proof that the suites before this one cannot see them.

  1. a softmax without the row maximum, exp(s) / sum exp(s);
  2. an online softmax over 32-key tiles whose running maximum starts at 0;
  3. an online softmax that rescales l but not the accumulated out when the maximum grows;
  4. a backward that rebuilds P as exp2(s c - lse) with lse left in natural-log units.

The inputs are what they claim, and the cap of budget() holds for the correct yardstick on every shape and regime of
test_attention_range_gpu.py.

Measured here (fp32 yardstick against fp64, worst over the fp32 shapes of that table; 8 x this is the widened budget):
  regime    out       lse       dqkv      dqkv / max |grad|   the case nearest the cap of budget()
  peaked    2.7e-05   3.2e-05   1.1e-04   8.8e-06             8 x 7.7e-05 of a cap of 8.7e-02 (dqkv, 97 tokens): 140x inside
  shifted   1.5e-04   8.7e-05   2.6e-03   1.2e-04             8 x 1.7e-03 of a cap of 1.4e-01 (dqkv, 16 tokens): 10x inside
  stairs    2.1e-04   1.2e-04   1.1e-02   1.2e-04             8 x 1.1e-02 of a cap of 9.0e-01 (dqkv, 1025 tokens): 11x inside
With P rounded to f16 the nearest case is out at 330 tokens: 8 x 6.2e-04 .. 9.5e-04 of a cap of 2.0e-02 .. 4.0e-02, 4x inside.
Mistakes 1 and 2 are rejected by `shifted` alone (every figure non-finite) and are accepted on `peaked` and `stairs`, whose
scores stay below exp's overflow at 88; mistake 3 misses out and dqkv by 3 .. 120 in every regime, mistake 4 dqkv by 1e5 ..
1e28.  On unit-normal inputs mistakes 1 and 2 are within 1.7e-06 of fp64 everywhere.
The stairs input at 130 tokens leaves the first 32-key tile a mass of at most 2.6e-21 on the even rows (exp(-45): far
below half an ulp of the out it is added to, not yet an exact 0 in fp32); from 289 tokens on it is exactly 0."""
import functools
import math

import pytest
import torch

import range_cases as R

FWD_TOL, BWD_TOL = 2e-5, 5e-5  # test_kernels_gpu.py::test_attention and every fp32 attention suite since
SHAPES = [(2, 77, 2, True), (1, 130, 1, False)]
TILE = 32


_case = R.attention_case


def _floors(want):
    return FWD_TOL, FWD_TOL, BWD_TOL * max(1.0, want[2].abs().max().item())


def _accepted(got, want, yard_err):
    """by the range rule: every one of out, lse, dqkv within budget(floor, yard_err, want)"""
    return all(R.accepts(g, w, f, y) for g, w, f, y in zip(got, want, _floors(want), yard_err))


def _accepted_by_fixed_budgets(got, want):
    return all(R.max_err(g, w) <= f for g, w, f in zip(got, want, _floors(want)))


# ---- the planted mistakes, all in fp32 -----------------------------------------------------------------------------------
def _finish(x, out, lse, dout, B, L, H):
    out = out.permute(0, 2, 1, 3).reshape(B * L, H * R.HD)
    out.backward(dout.float())
    return out.detach(), lse.detach().reshape(-1), x.grad


def no_row_max(qkv, dout, B, L, H, causal):
    x = qkv.float().requires_grad_()
    e = torch.exp(R.scores(x, B, L, H, causal))
    l = e.sum(-1, keepdim=True)
    return _finish(x, (e / l) @ R.split_heads(x, B, L, H)[2], torch.log(l[..., 0]), dout, B, L, H)


def online(qkv, dout, B, L, H, causal, m0=-math.inf, rescale_out=True):
    """flash-style: m, l and the accumulator carried over 32-key tiles, out = acc / l, lse = m + log l.  With the defaults
    it is correct."""
    x = qkv.float().requires_grad_()
    s = R.scores(x, B, L, H, causal)
    v = R.split_heads(x, B, L, H)[2]
    m = torch.full(s.shape[:-1] + (1,), m0)
    l = torch.zeros_like(m)
    acc = torch.zeros(s.shape[:-1] + (R.HD,))
    for j in range(0, L, TILE):
        st = s[..., j:j + TILE]
        mn = torch.maximum(m, st.amax(-1, keepdim=True).detach())
        f = torch.exp(m - mn)
        p = torch.exp(st - mn)
        l = l * f + p.sum(-1, keepdim=True)
        acc = (acc * f if rescale_out else acc) + p @ v[..., j:j + TILE, :]
        m = mn
    return _finish(x, acc / l, (m + torch.log(l))[..., 0], dout, B, L, H)


def lse_in_wrong_units(qkv, dout, B, L, H, causal):
    """a correct forward; the backward of the kernels (P from lse, D = dO . O, dS = P (dP - D)) with lse not multiplied by
    log2(e)"""
    c = math.log2(math.e)
    x = qkv.float()
    q, k, v = R.split_heads(x, B, L, H)
    s = R.scores(x, B, L, H, causal)
    lse = torch.logsumexp(s, -1)
    o = torch.exp(s - lse[..., None]) @ v
    do = dout.float().reshape(B, L, H, R.HD).permute(0, 2, 1, 3)
    p = torch.exp2(s * c - lse[..., None])
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    dq, dk, dv = ds @ k * 0.125, ds.transpose(-1, -2) @ q * 0.125, p.transpose(-1, -2) @ do
    dqkv = torch.stack([t.permute(0, 2, 1, 3) for t in (dq, dk, dv)], 2).reshape(B * L, 3 * H * R.HD)
    return o.permute(0, 2, 1, 3).reshape(B * L, H * R.HD), lse.reshape(-1), dqkv


MISTAKES = {
    "no_row_max": no_row_max,
    "running_max_starts_at_0": functools.partial(online, m0=0.0),
    "out_not_rescaled": functools.partial(online, rescale_out=False),
    "lse_in_wrong_units": lse_in_wrong_units,
}


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_planted_mistake_is_rejected(mistake, shape):
    verdict = {}
    for regime in R.ATTENTION_REGIMES:
        qkv, dout, want, yard_err = _case(*shape, regime)
        got = MISTAKES[mistake](qkv, dout, *shape)
        verdict[regime] = _accepted(got, want, yard_err)
        print(f"{mistake} {shape} {regime}: errors {[f'{R.max_err(g, w):.2e}' for g, w in zip(got, want)]}, "
              f"{'accepted' if verdict[regime] else 'rejected'}")
    assert not all(verdict.values()), f"{mistake} passes every regime at {shape}"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("mistake", ["no_row_max", "running_max_starts_at_0"])
def test_todays_suite_cannot_see_it(mistake, shape):
    """unit-normal inputs and the fixed budgets of the existing tests: accepted"""
    qkv, dout, want, _ = _case(*shape, "unit")
    got = MISTAKES[mistake](qkv, dout, *shape)
    print(f"{mistake} {shape} unit: errors {[f'{R.max_err(g, w):.2e}' for g, w in zip(got, want)]}")
    assert _accepted_by_fixed_budgets(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("regime", R.ATTENTION_REGIMES + ("unit",))
def test_correct_online_softmax_is_accepted(regime, shape):
    """the rule rejects the mistakes, not tiling: the same loop with m from -inf and the rescale passes everywhere"""
    qkv, dout, want, yard_err = _case(*shape, regime)
    assert _accepted(online(qkv, dout, *shape), want, yard_err)


# ---- the inputs are what they claim ---------------------------------------------------------------------------------------
def test_every_value_is_an_f16_number():
    for regime in R.ATTENTION_REGIMES:
        qkv, dout = R.attention_inputs(2, 77, 2, regime, 1)
        assert qkv.dtype == dout.dtype == torch.float64 and qkv.shape == (154, 384) and dout.shape == (154, 128)
        assert torch.equal(qkv.half().double(), qkv) and torch.equal(dout.half().double(), dout)
        again = R.attention_inputs(2, 77, 2, regime, 1)
        assert torch.equal(again[0], qkv) and torch.equal(again[1], dout)


def test_peaked_scores():
    qkv, _ = R.attention_inputs(1, 130, 1, "peaked", 3)
    s = R.scores(qkv, 1, 130, 1, False)
    lse = torch.logsumexp(s, -1)
    assert 15 < s.std().item() < 25
    assert 50 < lse.median().item() < 110 and lse.max().item() > 75
    assert torch.softmax(s, -1).amax(-1).median().item() > 0.9  # nearly one-hot


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shifted_rows_overflow_and_underflow_exp(shape):
    B, L, H, causal = shape
    qkv, _ = R.attention_inputs(B, L, H, "shifted", R.shape_seed(*shape))
    s = R.scores(qkv, B, L, H, causal)
    smallest = torch.where(torch.isinf(s), torch.full_like(s, math.inf), s).amin(-1)
    largest = s.amax(-1)
    assert (smallest[..., 0::2] > 89).all(), "even rows: exp() of every visible score overflows fp32"
    assert (largest[..., 1::2] < -89).all(), "odd rows: exp() of every score underflows, l = 0 if m starts at 0"
    p = torch.softmax(s, -1)  # and the softmax of a row stays O(1)-conditioned: no one-hot rows past the first few
    assert p[..., 8:, :].amax(-1).median().item() < 0.9


@pytest.mark.parametrize("L,exact", [(130, False), (289, True), (330, True)])
def test_stairs_first_tile_ends_with_no_weight(L, exact):
    qkv, _ = R.attention_inputs(1, L, 1, "stairs", L)
    s = R.scores(qkv.float(), 1, L, 1, False)
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    first = p[0, 0, :, :TILE].sum(-1)
    assert first.dtype == torch.float32
    print(f"stairs {L}: first-tile mass on the even rows at most {first[0::2].max().item():.2e}")
    if exact:
        assert (first[0::2] == 0).all()
    else:
        assert first[0::2].max().item() < 2.0 ** -25  # below half an ulp of anything it is added to
    assert (first[1::2] > 0.99).all(), "odd rows: the first tile holds the maximum and nearly all the mass"
    assert (p[0, 0, 1::2, -TILE:].sum(-1) == 0).all() or L < 289
    # a new running maximum in every later whole key tile on the even rows
    tile_max = torch.stack([s[0, 0, 0::2, j:j + TILE].amax(-1) for j in range(0, L - TILE + 1, TILE)], -1)
    assert (tile_max[:, 1:] > tile_max[:, :-1]).all()


def test_stairs_causal_peak_sits_on_the_diagonal():
    qkv, _ = R.attention_inputs(1, 130, 1, "stairs", 130)
    s = R.scores(qkv, 1, 130, 1, True)[0, 0]
    even = torch.arange(32, 130, 2)
    assert ((even - s[even].argmax(-1)) < 16).all()


def test_logit_regimes():
    for C in (5, 64, 65, 403):
        z = R.logit_inputs(7, C, "peaked", C)
        assert torch.equal(z.float().double(), z) and 20 < z.std().item() < 40
        z = R.logit_inputs(7, C, "shifted", C)
        assert (z[0::2] > 290).all() and (z[1::2] < -290).all()
        z = R.logit_inputs(7, C, "confident", C)
        p = torch.softmax(z.float(), -1)
        win = R.confident_winner(7, C)
        assert torch.equal(p.argmax(-1), win) and (p.sum(-1) == 1).all() and (p.sum(-1) - p.amax(-1) == 0).all()
        assert not torch.equal(R.confident_winner(7, C, 1), win)


# ---- the cap never triggers for the correct yardstick -----------------------------------------------------------------------
def _assert_inside_the_cap(what, want, yard_err):
    for name, w, f, y in zip(("out", "lse", "dqkv"), want, _floors(want), yard_err):
        b = R.budget(f, y, w)  # raises past the cap
        print(f"{what} {name}: yardstick {y:.2e}, budget {b:.2e}, cap {R.CAP * w.abs().max().item():.2e}")
        assert math.isfinite(y)


@pytest.mark.parametrize("shape", R.FP32_SHAPES, ids=str)
@pytest.mark.parametrize("regime", R.ATTENTION_REGIMES)
def test_cap_holds_for_the_fp32_yardstick(regime, shape):
    _, _, want, yard_err = _case(*shape, regime)
    _assert_inside_the_cap(f"{regime} {shape}", want, yard_err)


@pytest.mark.parametrize("shape", R.F16_SHAPES, ids=str)
@pytest.mark.parametrize("regime", R.ATTENTION_REGIMES)
def test_cap_holds_for_the_f16_yardstick(regime, shape):
    _, _, want, yard_err = _case(*shape, regime, None, torch.float16)
    _assert_inside_the_cap(f"{regime} {shape} f16", want, yard_err)


@pytest.mark.parametrize("round_p", [None, torch.float16], ids=["fp32", "f16"])
@pytest.mark.parametrize("regime", R.ATTENTION_REGIMES)
def test_cap_holds_for_the_packed_batch(regime, round_p):
    shape = (len(R.PACKED_LENS), R.PACKED_SEQ, R.PACKED_HEADS, True)
    _, _, want, yard_err = _case(*shape, regime, R.PACKED_LENS, round_p)
    _assert_inside_the_cap(f"{regime} packed", want, yard_err)


def test_budget_rule():
    want = torch.tensor([10.0, -30.0])
    assert R.budget(2e-5, 1e-7, want) == 2e-5  # the floor, unchanged
    assert R.budget(2e-5, 1e-3, want) == 8e-3
    with pytest.raises(AssertionError):
        R.budget(2e-5, 0.05, want)  # 0.4 > 1e-2 * 30
    with pytest.raises(AssertionError):
        R.budget(2e-5, float("nan"), want)
    with pytest.raises(AssertionError):
        R.budget(2e-5, 1e-5, torch.tensor([1e-3]))  # widened to 8e-5, past 1e-2 of 1e-3
    # nothing widened, nothing to cap: an expected value of zero but for underflow is held to the floor
    assert R.budget(1e-6, 6e-52, torch.tensor([6e-52])) == 1e-6
    assert R.max_err(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 1.0])) == math.inf
