"""clipfs_adamw_tail on the MI355X: the one AdamW launch with a tail that has its own weight decay and a clamp.
tail_n = 0 is bitwise ops.adamw_ext; with a tail the body is bitwise adamw_ext's and the tail is bitwise adamw_ext's at
the tail's decay, then clamped (and within fp32 rounding of the torch formula); a clamp that binds; a skipped step; the
EMA shadow sees the clamped value; the refusals that need device pointers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, TAIL = 1027, 3
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _state(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    p, grad = torch.randn(N, generator=g), torch.randn(N, generator=g)
    m, v = 0.1 * torch.randn(N, generator=g), 0.01 * torch.rand(N, generator=g)
    return [t.to(dev) for t in (p, grad, m, v)]


def _ext(dev, step=3, seed=0, **kw):
    from clipfs import ops
    p, g, m, v = _state(dev, seed)
    ops.adamw_ext(p, g, m, v, step, **{**HYPER, **kw})
    return p, m, v


def _tail(dev, step=3, seed=0, **kw):
    from clipfs import ops
    p, g, m, v = _state(dev, seed)
    ops.adamw_tail(p, g, m, v, step, **{**HYPER, **kw})
    return p, m, v


def test_tail_zero_is_bitwise_adamw_ext(dev):
    from clipfs import ops
    for a, b in zip(_ext(dev), _tail(dev, tail_n=0, tail_weight_decay=0.7, tail_min=-1e-3, tail_max=1e-3)):
        assert torch.equal(a, b)
    # ... with every record on
    outs = []
    for fn in (ops.adamw_ext, ops.adamw_tail):
        p, g, m, v = _state(dev)
        shadow = p.clone() + 1.0
        scale, clip = ops.new_scaler_state(1024.0, dev), ops.new_clip_state(dev)
        ops.grads_nonfinite(g, scale)
        ops.scaler_decide(scale, HYPER["lr"], HYPER["betas"])
        work = ops.grad_sumsq(g)
        ops.clip_decide(work, N, 1.0, clip, scale)
        fn(p, g, m, v, 1, **HYPER, scale_state=scale, clip_state=clip, ema_shadow=shadow, ema_decay=0.9)
        outs.append((p, m, v, shadow))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_body_is_adamw_ext_and_the_tail_has_its_own_decay_then_the_clamp(dev):
    lo, hi = -0.25, 0.4
    body = _ext(dev)
    own = _ext(dev, weight_decay=0.0)  # the same kernel at the tail's decay
    got = _tail(dev, tail_n=TAIL, tail_weight_decay=0.0, tail_min=lo, tail_max=hi)
    for a, b, c in zip(body, own, got):
        assert torch.equal(c[:-TAIL], a[:-TAIL])
    assert torch.equal(got[0][-TAIL:], own[0][-TAIL:].clamp(lo, hi))
    assert torch.equal(got[1][-TAIL:], own[1][-TAIL:]) and torch.equal(got[2][-TAIL:], own[2][-TAIL:])
    assert not torch.equal(body[0][-TAIL:], own[0][-TAIL:])  # the decay shows
    # the torch formula, fp64: p (1 - lr wd) - step_size m' / (sqrt(v') / sqrt(bc2) + eps)
    p, g, m, v = (t.double().cpu() for t in _state(dev))
    b1, b2 = HYPER["betas"]
    step = 3
    m1, v1 = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
    want = p - HYPER["lr"] / (1 - b1 ** step) * m1 / (v1.sqrt() / (1 - b2 ** step) ** 0.5 + HYPER["eps"])  # decay 0
    want = want[-TAIL:].clamp(lo, hi)
    err = float((got[0][-TAIL:].double().cpu() - want).abs().max())
    print("tail against the torch formula:", err, got[0][-TAIL:].tolist(), want.tolist())
    assert err <= 4 * 2.0 ** -24 * max(1.0, float(p[-TAIL:].abs().max()))


def test_a_clamp_that_binds_and_infinite_bounds(dev):
    free = _tail(dev, tail_n=TAIL, tail_weight_decay=0.0)  # -inf, +inf: no bound
    own = _ext(dev, weight_decay=0.0)
    assert torch.equal(free[0][-TAIL:], own[0][-TAIL:])
    top = float(own[0][-TAIL:].min()) - 0.5  # below every entry: all three are held at it
    held = _tail(dev, tail_n=TAIL, tail_weight_decay=0.0, tail_max=top)
    assert bool((held[0][-TAIL:] == torch.tensor(top, dtype=torch.float32).item()).all())
    assert torch.equal(held[0][:-TAIL], free[0][:-TAIL])
    whole = _tail(dev, tail_n=N, tail_weight_decay=HYPER["weight_decay"], tail_min=-0.5, tail_max=0.5)  # the tail may be everything
    assert torch.equal(whole[0], _ext(dev)[0].clamp(-0.5, 0.5))


def test_a_skipped_step_leaves_the_tail_untouched(dev):
    from clipfs import ops
    p, g, m, v = _state(dev)
    g[5] = float("inf")
    shadow = p.clone() + 1.0
    keep = [t.clone() for t in (p, m, v, shadow)]
    scale = ops.new_scaler_state(1024.0, dev)
    ops.grads_nonfinite(g, scale)
    ops.scaler_decide(scale, HYPER["lr"], HYPER["betas"])
    ops.adamw_tail(p, g, m, v, 1, **HYPER, scale_state=scale, ema_shadow=shadow, ema_decay=0.9, tail_n=TAIL,
                   tail_weight_decay=0.0, tail_min=-1e-3, tail_max=1e-3)  # a clamp that would bind
    for a, b in zip((p, m, v, shadow), keep):
        assert torch.equal(a, b)


def test_the_ema_shadow_holds_the_clamped_value(dev):
    from clipfs import ops
    p, g, m, v = _state(dev)
    shadow = torch.zeros_like(p)
    decay = 0.75
    ops.adamw_tail(p, g, m, v, 3, **HYPER, ema_shadow=shadow, ema_decay=decay, tail_n=TAIL, tail_weight_decay=0.0,
                   tail_min=-1e-3, tail_max=1e-3)
    assert bool((p[-TAIL:].abs() <= 1e-3).all()) and bool((p[-TAIL:].abs() == torch.tensor(1e-3).item()).any())
    want = torch.tensor(1.0 - decay, dtype=torch.float32).item() * p  # fmaf(decay, 0, (1 - decay) p_new)
    assert torch.equal(shadow, want)


def test_refusals(dev):
    from clipfs import _lib, ops
    p, g, m, v = _state(dev)
    keep = p.clone()
    for kw, word in ((dict(tail_n=N + 1), "tail_n = 1028 exceeds n = 1027"), (dict(tail_n=1, tail_min=1.0, tail_max=0.0), "exceeds tail_max"),
                     (dict(tail_n=1, tail_min=float("nan")), "NaN"), (dict(tail_n=1, tail_max=float("nan")), "NaN")):
        with pytest.raises(_lib.ClipfsError, match=word):
            ops.adamw_tail(p, g, m, v, 1, **HYPER, **kw)
    with pytest.raises(_lib.ClipfsError, match="step 0"):
        ops.adamw_tail(p, g, m, v, 0, **HYPER, tail_n=1)
    torch.cuda.synchronize()
    assert torch.equal(p, keep)
