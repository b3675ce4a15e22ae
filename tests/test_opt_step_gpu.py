"""The optimiser step's options on the GPU: the deterministic sum of squares and the clip decision against float64, the
extended AdamW's bitwise identities with the two existing AdamW entry points, the EMA shadow against a float64
restatement, and the trainers (LoRATrainer on TINY / SMALL with dropout 0.25, the fused stage-2 trainer, two
data-parallel ranks): clipping, averaged weights, and resuming from ``state_dict()`` bit for bit."""
import io
import os
import time
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, WD = 2e-4, (0.9, 0.999), 1e-8, 1e-2
CHUNK = 4096  # elements per pass-1 workgroup below 512 workgroups (csrc/elem.hip: kSumsqMinChunk)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _norm64(g):
    return torch.linalg.vector_norm(g.detach().double().cpu()).item()


def _two_ulp(want):
    """2 ulp of fp32 at the result: the double sums are exact to about n * 2^-53, the one rounding is the store."""
    return 2.0 * float(np.spacing(np.float32(want)))


def _clip_record(st):
    from clipfs import _lib as K
    f = st.cpu()
    return dict(norm=f[K.CLIP_NORM].item(), coef=f[K.CLIP_COEF].item(), mult=f[K.CLIP_MULT].item(),
                rest=f[K.CLIP_MULT + 1:].tolist())


def _measure(g, max_norm=1.0, scale_state=None):
    """grad_sumsq + clip_decide on a fresh work buffer and record -> (record dict, work buffer, record tensor)."""
    from clipfs import ops
    work = ops.grad_sumsq(g)
    st = ops.new_clip_state(g.device)
    ops.clip_decide(work, g.numel(), max_norm, st, scale_state)
    return _clip_record(st), work, st


# ------------------------------------------------------------------------------------------------------- 1. the norm
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 370689]


def _inputs(n):
    """name -> host fp32 [n]"""
    gen = torch.Generator().manual_seed(n)
    rnd = torch.randn(n, generator=gen)
    big = rnd.clone()
    big[torch.randint(0, n, (min(n, 5),), generator=gen)] = 1e19  # squares overflow fp32, the double sum must not
    big[n - 1] = -1e19
    out = {"random": rnd, "zeros": torch.zeros(n), "1e19": big}
    if n > CHUNK:  # the values on either side of the first boundary between two pass-1 workgroups carry the norm
        edge = rnd * 1e-3
        edge[CHUNK - 1], edge[CHUNK] = 3.0e3, -4.0e3
        out["chunk boundary"] = edge
    return out


@pytest.mark.parametrize("n", SIZES)
def test_norm(dev, n):
    from clipfs import ops
    for name, host in _inputs(n).items():
        want = _norm64(host)
        for off in range(4):
            base = torch.full((n + 8,), float("nan"), device=dev)  # poison on both sides: a read outside the slice shows
            lo = 4 + off
            g = base[lo:lo + n]
            assert g.data_ptr() % 16 == 4 * off
            g.copy_(host)
            rec, work, _ = _measure(g)
            rec2, work2, _ = _measure(g)
            err = abs(rec["norm"] - want)
            if off == 0:
                print(f"n={n} {name}: NORM {rec['norm']:.9g} float64 {want:.9g} |diff| {err:.3e} (bound {_two_ulp(want):.3e})")
            assert err <= _two_ulp(want), (n, name, off, rec["norm"], want)
            assert _same(work.view(torch.float32), work2.view(torch.float32)) and rec == rec2  # run to run, bit for bit
            assert rec["rest"] == [0.0] * 5
            if name == "zeros":
                assert rec["norm"] == 0.0 and rec["coef"] == 1.0 and rec["mult"] == 1.0
            # under a loss scale of 2^12 (exact in fp32 and in the double sum) NORM is still the unscaled norm
            if name != "1e19":
                sc = ops.new_scaler_state(2.0 ** 12, dev)
                keep = sc.clone()
                g.mul_(2.0 ** 12)
                rec_s, _, _ = _measure(g, scale_state=sc)
                assert abs(rec_s["norm"] - want) <= _two_ulp(want), (n, name, off, rec_s["norm"], want)
                assert rec_s["norm"] == rec["norm"]  # a power of two changes no bit
                assert _same(sc, keep)               # the scaler record is only read: its reserved words stay zero


def test_work_size_on_the_device_path(dev):
    """The buffer the query sizes is what the launches use: a guard value behind it survives both."""
    from clipfs import _lib, ops
    for n in (1, CHUNK, CHUNK + 1, 370689, 3934208):
        need = _lib.load().clipfs_grad_sumsq_work_doubles(n)
        assert need == min(512, -(-n // CHUNK))
        work = torch.full((need + 1,), -7.0, dtype=torch.float64, device=dev)
        g = torch.ones(n, device=dev)
        ops.grad_sumsq(g, work)
        st = ops.new_clip_state(dev)
        ops.clip_decide(work, n, 1.0, st)
        assert work[need].item() == -7.0
        assert work[:need].sum().item() == float(n)  # integers: exact in double
        assert abs(_clip_record(st)["norm"] - n ** 0.5) <= _two_ulp(n ** 0.5)


# --------------------------------------------------------------------------------------------------- 2. the decision
REL = 4 * 2.0 ** -24


@pytest.mark.parametrize("scale", [None, 2.0 ** 12, 1000.0])
def test_decision(dev, scale):
    from clipfs import _lib, ops
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(4099, generator=gen).to(dev)
    norm = _norm64(g)
    sc = None
    inv = 1.0
    if scale is not None:
        sc = ops.new_scaler_state(scale, dev)
        inv = sc[_lib.SCALER_INV_SCALE].item()
        norm *= inv
    for max_norm in (2.0 * norm, 0.5 * norm, norm / 7.3, 1e30):
        mx = float(np.float32(max_norm))  # the number the C ABI receives
        rec, _, st = _measure(g, mx, sc)
        want_coef = min(1.0, mx / (rec["norm"] + 1e-6))  # the float64 rule at the NORM the record holds
        want_mult = inv * want_coef
        print(f"scale {scale} max_norm {mx:.6g}: NORM {rec['norm']:.8g} COEF {rec['coef']:.9g} (float64 {want_coef:.9g}) "
              f"MULT {rec['mult']:.9g} (float64 {want_mult:.9g})")
        assert abs(rec["norm"] - norm) <= _two_ulp(norm)
        assert abs(rec["coef"] - want_coef) <= REL * want_coef
        assert abs(rec["mult"] - want_mult) <= REL * want_mult
        if rec["norm"] <= mx * (1 - 1e-3):  # clearly below: untouched gradients
            assert rec["coef"] == 1.0
            mult_bits = st.view(torch.int32)[_lib.CLIP_MULT].item()
            want_bits = (sc.view(torch.int32)[_lib.SCALER_INV_SCALE].item() if sc is not None
                         else torch.tensor(1.0).view(torch.int32).item())
            assert mult_bits == want_bits
        else:
            assert rec["coef"] < 1.0


def test_decision_of_a_non_finite_norm(dev):
    """Without a scaler: COEF = 0 (torch's clip_grad_norm_ with error_if_nonfinite=False gives 0 for an infinite norm)."""
    g = torch.ones(257, device=dev)
    for bad in (float("inf"), float("nan")):
        g[100] = bad
        rec, _, _ = _measure(g, 1.0)
        assert not np.isfinite(rec["norm"]) and rec["coef"] == 0.0 and rec["mult"] == 0.0


# ---------------------------------------------------------------------------------- 3. extended AdamW: exact identities
def _state(dev, n, seed):
    from test_loss_scale_gpu import _adam_state
    return _adam_state(dev, n, 4, seed)  # p, m, v after four plain steps, and the next gradient


@pytest.mark.parametrize("n", [1003, 4099])
def test_adamw_ext_without_options_is_adamw(dev, n):
    from clipfs import ops
    p, m, v, g = _state(dev, n, seed=7)
    want = [x.clone() for x in (p, m, v)]
    ops.adamw(want[0], g, want[1], want[2], 5, LR, BETAS, EPS, WD, 0.37)
    before = p.clone()
    ops.adamw_ext(p, g, m, v, 5, LR, BETAS, EPS, WD, 0.37)
    assert not _same(p, before)
    assert _same(p, want[0]) and _same(m, want[1]) and _same(v, want[2])


@pytest.mark.parametrize("n", [1003, 4099])
def test_adamw_ext_with_the_scaler_alone_is_adamw_scaled(dev, n):
    from clipfs import ops
    from test_loss_scale_gpu import _record
    p, m, v, g = _state(dev, n, seed=8)
    g = g * 2.0 ** 10
    st = _record(dev, 2.0 ** 10, step=4)
    ops.grads_nonfinite(g, st)
    ops.scaler_decide(st, LR, BETAS, 2.0, 0.5, 2000)
    want = [x.clone() for x in (p, m, v)]
    ops.adamw_scaled(want[0], g, want[1], want[2], st, LR, BETAS, EPS, WD)
    before = p.clone()
    ops.adamw_ext(p, g, m, v, 1, LR, BETAS, EPS, WD, 1.0, scale_state=st)  # step is ignored: the record says 5
    assert not _same(p, before)
    assert _same(p, want[0]) and _same(m, want[1]) and _same(v, want[2])


@pytest.mark.parametrize("n", [1003, 4099])
def test_adamw_ext_with_a_clip_record_uses_its_multiplier(dev, n):
    from clipfs import _lib, ops
    from test_loss_scale_gpu import _record
    p, m, v, g = _state(dev, n, seed=9)
    rec, _, cs = _measure(g, 0.25 * _norm64(g))
    assert 0.2 < rec["mult"] < 0.3 and rec["mult"] == rec["coef"]
    want = [x.clone() for x in (p, m, v)]
    ops.adamw(want[0], g, want[1], want[2], 5, LR, BETAS, EPS, WD, grad_scale=rec["mult"])
    got = [x.clone() for x in (p, m, v)]
    ops.adamw_ext(got[0], g, got[1], got[2], 5, LR, BETAS, EPS, WD, 1.0, clip_state=cs)
    for a, b in zip(got, want):
        assert _same(a, b)
    # with a scaler too: the corrections and the skip decision are the scaler's, the multiplier is MULT (which carries
    # INV_SCALE) -- the same as adamw_scaled on a record whose INV_SCALE word holds MULT
    gs = g * 1000.0
    st = _record(dev, 1000.0, step=4)
    ops.grads_nonfinite(gs, st)
    ops.scaler_decide(st, LR, BETAS, 2.0, 0.5, 2000)
    rec, _, cs = _measure(gs, 0.25 * _norm64(g), st)
    assert rec["coef"] < 1.0 and rec["mult"] < 1e-3
    forged = st.clone()
    forged[_lib.SCALER_INV_SCALE] = cs[_lib.CLIP_MULT]
    want = [x.clone() for x in (p, m, v)]
    ops.adamw_scaled(want[0], gs, want[1], want[2], forged, LR, BETAS, EPS, WD)
    got = [x.clone() for x in (p, m, v)]
    ops.adamw_ext(got[0], gs, got[1], got[2], 1, LR, BETAS, EPS, WD, 1.0, scale_state=st, clip_state=cs)
    for a, b in zip(got, want):
        assert _same(a, b)
    assert not _same(got[0], p)


@pytest.mark.parametrize("n", [1003, 4099])
def test_adamw_ext_skipped_step_writes_nothing(dev, n):
    from clipfs import _lib, ops
    from test_loss_scale_gpu import _record
    p, m, v, g = _state(dev, n, seed=10)
    g[n - 2] = float("inf")
    shadow = (p * 0.5).contiguous()
    keep = [x.clone() for x in (p, m, v, shadow)]
    st = _record(dev, 65536.0, tracker=7, step=4)
    ops.grads_nonfinite(g, st)
    ops.scaler_decide(st, LR, BETAS, 2.0, 0.5, 2000)
    assert st.view(torch.int32)[_lib.SCALER_SKIP].item() == 1
    rec, _, cs = _measure(g, 1.0, st)
    assert not np.isfinite(rec["norm"])  # the record still gets NORM
    ops.adamw_ext(p, g, m, v, 5, LR, BETAS, EPS, WD, 1.0, scale_state=st, clip_state=cs, ema_shadow=shadow, ema_decay=0.999)
    for got, want in zip((p, m, v, shadow), keep):
        assert _same(got, want)


# ------------------------------------------------------------------------------------------------ 4. EMA arithmetic
def _ema64(shadow64, p_dev, decay):
    """The float64 restatement of one shadow update from the parameter the device holds (fp32 values are exact in
    float64; decay crosses the C ABI as fp32)."""
    d = float(np.float32(decay))
    return d * shadow64 + (1.0 - d) * p_dev.detach().double().cpu()


@pytest.mark.parametrize("decay", [0.999, 0.9])
def test_ema_arithmetic(dev, decay):
    from clipfs import ops
    from oracle import clip_oracle as O
    n, k = 4099, 5
    gen = torch.Generator().manual_seed(21)
    p = (torch.randn(n, generator=gen) * 0.05).to(dev)  # adapter-sized values, as tests/test_glue_kernels_gpu.py uses
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    shadow = p.clone()
    assert shadow.data_ptr() != p.data_ptr()
    p64, m64, v64 = p.double().cpu(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    s64 = p64.clone()
    for t in range(1, k + 1):
        g = torch.randn(n, generator=gen)
        ops.adamw_ext(p, g.to(dev), m, v, t, LR, BETAS, EPS, WD, 1.0, ema_shadow=shadow, ema_decay=decay)
        p64, m64, v64 = O.jt_adamw_step(p64, g.double(), m64, v64, t, LR, BETAS, EPS, WD)
        s64 = _ema64(s64, p, decay)
        if t == 1:
            assert not torch.equal(shadow, p)  # the shadow is an average, not an alias of the parameters
    # the AdamW part against the oracle, as tests/test_engine_gpu.py holds the trainer's step
    assert (p.double().cpu() - p64).abs().max().item() < 1e-6
    # three fp32 roundings per step (1 - decay, its product with p, the fused multiply-add), k steps
    bound = k * 3 * 2.0 ** -24 * torch.maximum(s64.abs(), p.double().cpu().abs())
    err = (shadow.double().cpu() - s64).abs()
    print(f"decay {decay}: max shadow error {err.max().item():.3e}, largest error / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------- 5. LoRATrainer
def _make(dev, cfg_name, r=4, p=0.25):
    """tests/test_engine_gpu.py's geometry: rank-r q/k/v adapters in every block of both towers, LoRA dropout p, train mode."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = getattr(synth, cfg_name)
    backbone = cfg_name.lower()
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    model = build_model(sd, device=dev)
    args = types.SimpleNamespace(encoder="both", position="all", backbone=backbone, params=["q", "k", "v"], r=r, alpha=1,
                                 dropout_rate=p)
    saved_t, saved_v = L.INDEX_POSITIONS_TEXT["all"], L.INDEX_POSITIONS_VISION.get(backbone)
    L.INDEX_POSITIONS_TEXT["all"] = list(range(cfg.transformer_layers))
    L.INDEX_POSITIONS_VISION[backbone] = {"all": list(range(cfg.vision_layers))}
    try:
        layers = L.apply_lora(args, model)
    finally:
        L.INDEX_POSITIONS_TEXT["all"] = saved_t
        if saved_v is None:
            del L.INDEX_POSITIONS_VISION[backbone]
        else:
            L.INDEX_POSITIONS_VISION[backbone] = saved_v
    lw = synth.synth_lora(cfg, r, seed=5)
    names = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                mod = getattr(layer, names[pr])
                mod.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][names[pr]]["w_lora_A"]))
                mod.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][names[pr]]["w_lora_B"]))
    model.train(p > 0)
    return L, model, cfg


def _batch(dev, cfg, B=6, Cn=9):
    from clipfs import synth
    return (synth.synth_images(B, cfg.image_resolution, seed=3).to(dev),
            synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev),
            synth.synth_labels(B, Cn, seed=2).to(dev))


def _trainer(dev, cfg_name, r=4, **kw):
    L, model, cfg = _make(dev, cfg_name, r)
    return L.LoRATrainer(model, lr=LR, **kw), _batch(dev, cfg)


_PLAIN = {}


def _plain(dev, cfg_name):
    """Three steps without any option (computed once per model): the start, the first step's gradient and its float64
    norm, and parameters, moments and loss after each step."""
    if cfg_name not in _PLAIN:
        tr, batch = _trainer(dev, cfg_name)
        out = dict(p0=tr.flat.params.clone(), params=[], losses=[])
        for s in range(3):
            loss, _, _ = tr.step(*batch)
            if s == 0:
                out["grad"] = tr.flat.grads.clone()
                out["norm"] = _norm64(out["grad"])
            out["params"].append(tr.flat.params.clone())
            out["losses"].append(loss.clone())
        out["m"], out["v"] = tr.flat.m.clone(), tr.flat.v.clone()
        assert tr.last_grad_norm is None and tr.last_clip_coef is None and not tr.shadow_applied
        assert out["norm"] > 1e-4
        _PLAIN[cfg_name] = out
    return _PLAIN[cfg_name]


@pytest.mark.parametrize("cfg_name", ["TINY", "SMALL"])
def test_trainer_with_a_huge_max_norm_is_the_plain_trainer(dev, cfg_name):
    plain = _plain(dev, cfg_name)
    tr, batch = _trainer(dev, cfg_name, max_grad_norm=1e30)
    for s in range(3):
        loss, _, _ = tr.step(*batch)
        assert tr.last_clip_coef == 1.0
        assert _same(loss, plain["losses"][s]) and _same(tr.flat.params, plain["params"][s]), s
    assert _same(tr.flat.m, plain["m"]) and _same(tr.flat.v, plain["v"])
    assert abs(tr.last_grad_norm - _norm64(tr.flat.grads)) <= _two_ulp(tr.last_grad_norm)


@pytest.mark.parametrize("cfg_name", ["TINY", "SMALL"])
def test_trainer_clipped_step(dev, cfg_name):
    from oracle import clip_oracle as O
    from test_glue_kernels_gpu import _adamw_f32
    plain = _plain(dev, cfg_name)
    max_norm = float(np.float32(0.5 * plain["norm"]))
    tr, batch = _trainer(dev, cfg_name, max_grad_norm=max_norm)
    tr.step(*batch)
    got_norm, got_coef = tr.last_grad_norm, tr.last_clip_coef
    print(f"{cfg_name}: last_grad_norm {got_norm:.9g} float64 {plain['norm']:.9g} (bound {_two_ulp(plain['norm']):.3e}) "
          f"coef {got_coef:.9g}")
    assert abs(got_norm - plain["norm"]) <= _two_ulp(plain["norm"])
    coef = min(1.0, max_norm / (plain["norm"] + 1e-6))
    assert abs(got_coef - coef) <= REL * coef and 0.49 < got_coef < 0.51
    p0, g = plain["p0"].cpu(), plain["grad"].cpu()
    zero = torch.zeros_like(p0)
    want, _, _ = O.jt_adamw_step(p0.double(), g.double() * coef, zero.double(), zero.double(), 1, LR, BETAS, EPS, WD)
    r32, _, _ = _adamw_f32(p0, g, zero, zero.clone(), 1, LR, BETAS[0], BETAS[1], EPS, WD, float(np.float32(coef)))
    e32 = (r32.double() - want).abs().max().item()
    err = (tr.flat.params.double().cpu() - want).abs().max().item()
    moved = (want - plain["params"][0].double().cpu()).abs().max().item()
    print(f"{cfg_name}: max |param - float64| = {err:.3e}; fp32 restatement {e32:.3e} -> bound {4 * e32:.3e}; "
          f"clipped and unclipped steps differ by {moved:.3e}")
    assert err <= 4 * e32
    assert not _same(tr.flat.params, plain["params"][0])


@pytest.mark.parametrize("cfg_name", ["TINY", "SMALL"])
def test_trainer_clipping_under_a_power_of_two_loss_scale(dev, cfg_name):
    """Scaling by 2^12 is exact, NORM is the unscaled norm and MULT = 2^-12 * COEF exactly: the same trajectory."""
    plain = _plain(dev, cfg_name)
    max_norm = 0.5 * plain["norm"]
    a, batch = _trainer(dev, cfg_name, max_grad_norm=max_norm)
    b, _ = _trainer(dev, cfg_name, max_grad_norm=max_norm, loss_scale=2.0 ** 12)
    for s in range(3):
        la, _, _ = a.step(*batch)
        lb, _, _ = b.step(*batch)
        diff = (a.flat.params - b.flat.params).abs().max().item()
        print(f"{cfg_name} step {s + 1}: norm {a.last_grad_norm:.9g} / {b.last_grad_norm:.9g}, coef {a.last_clip_coef:.9g} / "
              f"{b.last_clip_coef:.9g}, max |param diff| {diff:.3e}")
        assert _same(la, lb)
        assert a.last_grad_norm == b.last_grad_norm and a.last_clip_coef == b.last_clip_coef < 1.0
        assert _same(a.flat.params, b.flat.params), s
    assert _same(a.flat.m, b.flat.m) and _same(a.flat.v, b.flat.v)
    assert (b.skipped_steps, b.optimizer_steps) == (0, 3)


def test_trainer_skipped_step_leaves_the_shadow(dev):
    tr, batch = _trainer(dev, "TINY", loss_scale="dynamic", max_grad_norm=1.0, ema_decay=0.999)
    tr.step(*batch)
    assert not _same(tr.ema_shadow, tr.flat.params) and tr.skipped_steps == 0
    tr.flat.zero_grad()
    tr.forward_backward(*batch)
    keep = [x.clone() for x in (tr.flat.params, tr.flat.m, tr.flat.v, tr.ema_shadow)]
    tr.flat.grads[tr.flat.numel // 2] = float("inf")
    tr.optimizer_step()
    for got, want in zip((tr.flat.params, tr.flat.m, tr.flat.v, tr.ema_shadow), keep):
        assert _same(got, want)
    assert (tr.skipped_steps, tr.optimizer_steps, tr.t) == (1, 1, 2)
    assert not np.isfinite(tr.last_grad_norm)


# ------------------------------------------------------------------------------------------ 6. apply_shadow / restore
def test_apply_shadow_and_restore(dev):
    decay = 0.9
    L, model, cfg = _make(dev, "SMALL")
    tr = L.LoRATrainer(model, lr=1e-2, ema_decay=decay)  # a rate at which two steps move the features visibly
    batch = _batch(dev, cfg)
    s64 = tr.flat.params.double().cpu()
    assert _same(tr.ema_shadow, tr.flat.params) and tr.ema_shadow.data_ptr() != tr.flat.params.data_ptr()  # register()
    for _ in range(2):
        tr.step(*batch)
        s64 = _ema64(s64, tr.flat.params, decay)
    model.eval()
    live = tr.flat.params.clone()
    with torch.no_grad():
        f_live = model.encode_image(batch[0]).clone()
        tr.apply_shadow()
        assert tr.shadow_applied and _same(tr.flat.params, tr.ema_shadow) and not _same(tr.flat.params, live)
        f_avg = model.encode_image(batch[0]).clone()
        t_avg = model.encode_text(batch[1]).clone()
    with pytest.raises(RuntimeError, match="already applied"):
        tr.apply_shadow()
    with pytest.raises(RuntimeError, match="restore"):
        tr.optimizer_step()
    tr.restore()
    assert not tr.shadow_applied and _same(tr.flat.params, live)
    with pytest.raises(RuntimeError, match="apply_shadow"):
        tr.restore()
    with torch.no_grad():
        assert _same(model.encode_image(batch[0]), f_live)
    # a second model whose adapters are set to the float64-restated average
    L2, model2, _ = _make(dev, "SMALL")
    tr2 = L2.LoRATrainer(model2, lr=1e-2)
    with torch.no_grad():
        tr2.flat.params.copy_(s64.float())
    tr2.flat.sync_packed()
    model2.eval()
    with torch.no_grad():
        w_img, w_txt = model2.encode_image(batch[0]), model2.encode_text(batch[1])
    e_img, e_txt = (f_avg - w_img).abs().max().item(), (t_avg - w_txt).abs().max().item()
    gap = (f_avg - f_live).abs().max().item()
    print(f"apply_shadow: image features {e_img:.3e}, text features {e_txt:.3e} from the restated average (bound 2e-5); "
          f"averaged and live image features differ by {gap:.3e}")
    assert e_img < 2e-5 and e_txt < 2e-5
    assert gap > 1e-4  # the comparison above is not vacuous
    tr.step(*batch)    # training goes on after restore()
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr2.apply_shadow()


# ---------------------------------------------------------------------------------------------------------- 7. resume
def _roundtrip(sd):
    """Through torch.save and a load that accepts tensors and plain Python values only."""
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


def _state_tensors(tr):
    return [tr.flat.params, tr.flat.m, tr.flat.v, tr.ema_shadow, tr.scale_state, tr.clip_state]


def test_resume_lora_trainer(dev):
    max_norm = 0.5 * _plain(dev, "TINY")["norm"]
    kw = dict(loss_scale="dynamic", growth_interval=2, max_grad_norm=max_norm, ema_decay=0.999)
    a, batch = _trainer(dev, "TINY", **kw)
    losses_a = [a.step(*batch)[0].clone() for _ in range(4)]
    assert a.loss_scale_value == 65536.0 * 4 and a.last_clip_coef < 1.0
    b, _ = _trainer(dev, "TINY", **kw)
    losses_b = [b.step(*batch)[0].clone() for _ in range(2)]
    sd = _roundtrip(b.state_dict())
    assert all(not t.is_cuda for t in sd.values() if torch.is_tensor(t))
    assert sd["t"] == 2 and sd["engine"]["step"] == b.model.engine.step > 0 and sd["scale_state"].numel() == 16
    c, _ = _trainer(dev, "TINY", **kw)  # a freshly built model and trainer
    c.load_state_dict(sd)
    assert c.t == 2 and c.model.engine.step == b.model.engine.step
    losses_b += [c.step(*batch)[0].clone() for _ in range(2)]
    for x, y in zip(_state_tensors(a), _state_tensors(c)):
        assert _same(x, y)
    for x, y in zip(losses_a, losses_b):
        assert _same(x, y)
    assert (c.t, c.optimizer_steps, c.skipped_steps) == (a.t, a.optimizer_steps, a.skipped_steps) == (4, 4, 0)
    # refused: another adapter layout, another set of options -- the message names the difference
    other, _ = _trainer(dev, "TINY", r=2, **kw)
    with pytest.raises(ValueError, match=r"layout.*lora_A_qkv.*saved \d+ floats, this trainer \d+"):
        other.load_state_dict(sd)
    no_ema, _ = _trainer(dev, "TINY", loss_scale="dynamic", growth_interval=2, max_grad_norm=max_norm)
    with pytest.raises(ValueError, match="ema_decay is on in the saved state and off in this trainer"):
        no_ema.load_state_dict(sd)
    no_clip, _ = _trainer(dev, "TINY", loss_scale="dynamic", growth_interval=2, ema_decay=0.999)
    before = no_clip.flat.params.clone()
    with pytest.raises(ValueError, match="max_grad_norm is on in the saved state and off in this trainer"):
        no_clip.load_state_dict(sd)
    assert _same(no_clip.flat.params, before) and no_clip.t == 0  # a refusal changes nothing
    unscaled, _ = _trainer(dev, "TINY", max_grad_norm=max_norm, ema_decay=0.999)
    with pytest.raises(ValueError, match="loss_scale is on in the saved state and off in this trainer"):
        unscaled.load_state_dict(sd)


# -------------------------------------------------------------------------------------------------- 8. fused stage 2
def _stage2(dev, **kw):
    from test_stage2_fused_gpu import _setup
    return _setup(dev, p=0.25, fused=True, **kw)


def _s2_step(s):
    return s.tr.step(s.images, s.target, s.index)


@pytest.fixture(scope="module")
def stage2_plain(dev):
    s = _stage2(dev)
    out = dict(p0=s.tr.flat.params.clone(), params=[], losses=[])
    for i in range(3):
        loss, _, _ = _s2_step(s)
        if i == 0:
            out["grad"] = s.tr.flat.grads.clone()
            out["norm"] = _norm64(out["grad"])
        out["params"].append(s.tr.flat.params.clone())
        out["losses"].append(loss.clone())
    return out


def test_stage2_with_a_huge_max_norm_is_the_plain_trainer(dev, stage2_plain):
    s = _stage2(dev, max_grad_norm=1e30)
    for i in range(3):
        loss, _, _ = _s2_step(s)
        assert s.tr.last_clip_coef == 1.0
        assert _same(loss, stage2_plain["losses"][i]) and _same(s.tr.flat.params, stage2_plain["params"][i]), i


def test_stage2_clipped_step(dev, stage2_plain):
    from oracle import clip_oracle as O
    from test_glue_kernels_gpu import _adamw_f32
    plain = stage2_plain
    max_norm = float(np.float32(0.5 * plain["norm"]))
    s = _stage2(dev, max_grad_norm=max_norm)
    _s2_step(s)
    tr = s.tr
    assert abs(tr.last_grad_norm - plain["norm"]) <= _two_ulp(plain["norm"])
    coef = min(1.0, max_norm / (plain["norm"] + 1e-6))
    assert abs(tr.last_clip_coef - coef) <= REL * coef
    p0, g = plain["p0"].cpu(), plain["grad"].cpu()
    zero = torch.zeros_like(p0)
    lr = 1e-3  # the pre-step rate of test_stage2_fused_gpu._setup
    want, _, _ = O.jt_adamw_step(p0.double(), g.double() * coef, zero.double(), zero.double(), 1, lr, BETAS, EPS, WD)
    r32, _, _ = _adamw_f32(p0, g, zero, zero.clone(), 1, lr, BETAS[0], BETAS[1], EPS, WD, float(np.float32(coef)))
    e32 = (r32.double() - want).abs().max().item()
    err = (tr.flat.params.double().cpu() - want).abs().max().item()
    print(f"stage 2: norm {tr.last_grad_norm:.9g} coef {tr.last_clip_coef:.9g}; max |param - float64| = {err:.3e}; "
          f"fp32 restatement {e32:.3e} -> bound {4 * e32:.3e}")
    assert err <= 4 * e32
    assert not _same(tr.flat.params, plain["params"][0])


def test_stage2_resume_across_the_cosine_schedule(dev, stage2_plain):
    kw = dict(loss_scale="dynamic", growth_interval=2, max_grad_norm=0.5 * stage2_plain["norm"], ema_decay=0.999)
    a = _stage2(dev, **kw)
    losses_a = [_s2_step(a)[0].clone() for _ in range(4)]
    b = _stage2(dev, **kw)
    losses_b = [_s2_step(b)[0].clone() for _ in range(2)]
    sd = _roundtrip(b.tr.state_dict())
    assert sd["scheduler"]["last_epoch"] == 2 and sd["lr"] == b.tr.lr < 1e-3
    c = _stage2(dev, **kw)
    c.tr.load_state_dict(sd)
    assert c.tr.lr == b.tr.lr and c.tr.sched.last_epoch == 2
    losses_b += [_s2_step(c)[0].clone() for _ in range(2)]
    for x, y in zip(_state_tensors(a.tr), _state_tensors(c.tr)):
        assert _same(x, y)
    for x, y in zip(losses_a, losses_b):
        assert _same(x, y)
    assert c.tr.lr == a.tr.lr and c.tr.sched.last_epoch == a.tr.sched.last_epoch == 4
    # a stage-1 state does not fit a stage-2 trainer
    lora, batch = _trainer(dev, "TINY", **kw)
    lora.step(*batch)
    with pytest.raises(ValueError, match="layout"):
        c.tr.load_state_dict(lora.state_dict())


# ------------------------------------------------------------------------------------------------ 9. data parallelism
def _rank_main(rank, world, port, max_norm, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root, os.path.join(root, "tests")):
        if path not in sys.path:
            sys.path.insert(0, path)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from clipfs import dist as D
    import test_dp_gpu as T
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    L, model, ctx, img, cap, tgt = T._make(dev)
    model.eval()
    tr = L.LoRATrainer(model, prompt_ctx=ctx, max_grad_norm=max_norm)
    lo, hi = D.shard_bounds(img.shape[0], rank, world)
    tr.flat.zero_grad()
    tr.forward_backward(img[lo:hi].contiguous(), cap, tgt[lo:hi].contiguous(), 1, img.shape[0], row_offset=lo)
    tr.optimizer_step()
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), record=tr.clip_state.cpu().numpy(),
             params=tr.flat.params.cpu().numpy())
    dist.destroy_process_group()


def test_two_ranks_clip_alike(tmp_path, dev):
    import test_dp_gpu as T
    L, model, ctx, img, cap, tgt = T._make(dev)
    model.eval()
    plain = L.LoRATrainer(model, prompt_ctx=ctx)
    plain.flat.zero_grad()
    plain.forward_backward(img, cap, tgt)
    max_norm = float(np.float32(0.5 * _norm64(plain.flat.grads)))
    L, model, ctx, img, cap, tgt = T._make(dev)
    model.eval()
    one = L.LoRATrainer(model, prompt_ctx=ctx, max_grad_norm=max_norm)
    one.step(img, cap, tgt)
    assert 0.49 < one.last_clip_coef < 0.51
    ctx_ = mp.spawn(_rank_main, args=(2, T._free_port(), max_norm, str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120  # each rank lives under this limit: a rank that hangs is killed, not waited for
    try:
        while not ctx_.join(timeout=5):
            assert time.monotonic() < deadline, "a data-parallel rank did not finish in time"
    finally:
        for pr in ctx_.processes:
            if pr.is_alive():
                pr.kill()
    z = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(2)]
    assert np.array_equal(z[0]["record"].view(np.int32), z[1]["record"].view(np.int32))  # NORM, COEF, MULT: bit for bit
    assert np.array_equal(z[0]["params"].view(np.int32), z[1]["params"].view(np.int32))
    norm, coef = float(z[0]["record"][0]), float(z[0]["record"][1])
    print(f"two ranks: NORM {norm:.9g} COEF {coef:.9g}; one process: {one.last_grad_norm:.9g} {one.last_clip_coef:.9g}")
    assert abs(norm - one.last_grad_norm) <= 2e-5 * one.last_grad_norm  # tests/test_dp_gpu.py's bound on the gradients
    assert coef < 1.0
    assert np.abs(z[0]["params"] - one.flat.params.cpu().numpy()).max() < 1e-6
