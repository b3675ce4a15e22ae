"""The training-free dynamic adapter on the GPU (csrc/tda.hip, ops.tda_adapt, tda.TestTimeDynamicAdapter) against the fp64
sequential rule of tda_ref.py.  Geometries G1 (C 5, B 70, d 64: eviction-heavy, three row tiles with a ragged last one)
and G2 (C 37, B 90, d 132: ragged class and feature chunks), Sp 3, Sn 2, s 100, clustered features.  Before the GPU is
touched the reference asserts that every comparison the rule decides has a margin far above the fp32 error of H and that
every kind of event occurs, so decisions must be EXACT and logits within the project's 1e-3 logit bound."""
import numpy as np
import pytest
import torch

import tda_ref as R
from poison import FILLS, assert_same_runs, poison_, same_bits
from test_tda_cpu import G1, G2

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3   # absolute, against fp64: the bound of test_cache_head_gpu.py
STATE = ("pos_keys", "pos_ent", "pos_seq", "neg_keys", "neg_ent", "neg_seq", "neg_mask", "counter")
PER_SAMPLE = ("pred", "entropy", "hnorm", "band", "seq", "mask", "pos_slot", "neg_slot")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


_REF = {}


def _ref(geo):
    """(T, F, out, record, state, reference) of one call over the whole stream from empty caches: computed once, shared,
    never written.  The condition is asserted here, on the reference."""
    if geo not in _REF:
        C, B, d, seed = geo
        T, F, _ = R.clustered(C, B, d, seed)
        ref = R.TDARef(T)
        out, rec = ref.adapt(F)
        assert ref.well_conditioned() == [], ref.events
        _REF[geo] = (T, F, out, rec, ref.state(), ref)
    return _REF[geo]


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).float().to(dev)


def _new_state(geo, dev, Sp=3, Sn=2):
    from clipfs import ops
    return ops.tda_new_state(geo[0], geo[2], Sp, Sn, dev)


def _clone(state):
    return {k: v.clone() for k, v in state.items()}


def _states_same(a, b):
    return all(same_bits(a[k], b[k]) for k in STATE)


def _seq_sets(seq):
    return [sorted(int(s) for s in row if s >= 0) for row in np.asarray(seq)]


def _check_against_reference(geo, out, rec, state, F32):
    T, F, want, wrec, wstate, _ = _ref(geo)
    assert rec["pred"].tolist() == wrec["pred"].tolist()
    assert (rec["pos_slot"] >= 0).tolist() == (wrec["pos_slot"] >= 0).tolist()
    assert (rec["neg_slot"] >= 0).tolist() == (wrec["neg_slot"] >= 0).tolist()
    assert rec["band"].tolist() == wrec["band"].tolist()
    rows = np.flatnonzero(wrec["band"])  # the rows whose mask the rule uses
    assert np.array_equal(rec["mask"].cpu().numpy()[rows], wrec["mask"][rows])
    for name in ("pos", "neg"):
        seq = state[name + "_seq"].cpu().numpy()
        assert _seq_sets(seq) == _seq_sets(wstate[name + "_seq"]), name
        keys = state[name + "_keys"].cpu()
        for c, k in zip(*np.nonzero(seq >= 0)):
            assert same_bits(keys[c, k], F32[int(seq[c, k])].cpu()), (name, c, k)  # bitwise the input row
            assert abs(float(state[name + "_ent"][c, k]) - wrec["entropy"][int(seq[c, k])]) < 1e-4
            if name == "neg":
                assert np.array_equal(state["neg_mask"][c, k].cpu().numpy(), wrec["mask"][int(seq[c, k])])
    assert int(state["counter"]) == wstate["counter"]
    eh = np.abs(rec["entropy"].double().cpu().numpy() - wrec["entropy"]).max()
    err = np.abs(out.double().cpu().numpy() - want).max()
    return err, eh


# -------------------------------------------------------------------------------- 1. one call against the reference
@pytest.mark.parametrize("geo", [G1, G2], ids=["G1", "G2"])
def test_one_call_matches_the_sequential_rule(dev, geo):
    from clipfs import ops
    T, F = _ref(geo)[:2]
    T32, F32, state = _dev(T, dev), _dev(F, dev), _new_state(geo, dev)
    out, rec = ops.tda_adapt(F32, T32, state)
    err, eh = _check_against_reference(geo, out, rec, state, F32)
    print(f"tda {geo}: max |logit - fp64| = {err:.2e}, max |H - fp64| = {eh:.2e}")
    assert err <= LOGIT_TOL


# ------------------------------------------------------------------------------------------- 2. split invariance
def test_split_invariance(dev):
    from clipfs import ops
    T, F, want = _ref(G1)[:3]
    T32, F32 = _dev(T, dev), _dev(F, dev)
    runs = []
    for split in ((70,), (1, 31, 38), (1,) * 70):
        state, b0, outs, recs = _new_state(G1, dev), 0, [], []
        for n in split:
            o, r = ops.tda_adapt(F32[b0:b0 + n], T32, state)
            outs.append(o)
            recs.append(r)
            b0 += n
        out = torch.cat(outs)
        rec = {k: torch.cat([r[k] for r in recs]) for k in PER_SAMPLE}
        err = np.abs(out.double().cpu().numpy() - want).max()
        print(f"tda split {split[:3]}{'...' if len(split) > 3 else ''}: max |logit - fp64| = {err:.2e}")
        assert err <= LOGIT_TOL
        runs.append((state, rec))
    for state, rec in runs[1:]:
        assert _states_same(state, runs[0][0])
        for k in PER_SAMPLE:
            assert same_bits(rec[k], runs[0][1][k]), k


# ---------------------------------------------------------------------------------------- 3. carry-over and resume
def test_carry_over_and_resume(dev):
    from tda import TestTimeDynamicAdapter
    T, F = _ref(G1)[:2]
    T32, F32 = _dev(T, dev), _dev(F, dev)
    a = TestTimeDynamicAdapter(T32, n_classes=5)
    a.adapt_features(F32[:20])
    a.adapt_features(F32[20:45])
    sd = a.state_dict()
    assert all(not v.is_cuda for v in sd.values() if isinstance(v, torch.Tensor))
    last = a.adapt_features(F32[45:])
    b = TestTimeDynamicAdapter(T32, n_classes=5)
    b.load_state_dict(sd)
    again = b.adapt_features(F32[45:])
    assert _states_same(a.state, b.state)
    for x, y in zip(last, again):
        assert same_bits(x, y)
    whole = TestTimeDynamicAdapter(T32, n_classes=5)
    whole.adapt_features(F32)
    assert _states_same(a.state, whole.state)
    with pytest.raises(ValueError, match="pos_cap"):
        TestTimeDynamicAdapter(T32, pos_cap=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="n_classes"):
        TestTimeDynamicAdapter(T32[:4].contiguous()).load_state_dict(sd)
    with pytest.raises(ValueError, match="neg_beta"):
        TestTimeDynamicAdapter(T32, neg_beta=2.0).load_state_dict(sd)


# ------------------------------------------------------------------------------------- 4. determinism and poison
def test_determinism_and_poison(dev):
    from clipfs import ops
    T, F = _ref(G2)[:2]
    C, B = G2[0], G2[1]
    T32, F32 = _dev(T, dev), _dev(F, dev)
    start = _new_state(G2, dev)
    ops.tda_adapt(F32[:40], T32, start)  # a filled state to start from
    runs = []
    for i, fill in enumerate(FILLS + (None,)):
        state = _clone(start)
        if fill is None:  # a plain second run
            out, rec = ops.tda_adapt(F32[40:], T32, state)
            guard = None
        else:
            wide = torch.empty(B - 40, C + 3, device=dev)
            poison_(wide, fill)
            rec = ops.tda_new_record(C, B - 40, 3, 2, dev)
            for t in rec.values():
                if t.dtype.is_floating_point:
                    poison_(t, fill)
                else:
                    t.fill_((0, -1, 77)[i])
            out, rec = ops.tda_adapt(F32[40:], T32, state, out=wide[:, :C], record=rec)
            guard = wide[:, C:]
            assert same_bits(guard, torch.full_like(guard, fill)), "the guard columns past C were written"
            out = out.contiguous()
        # the state goes in as raw bits: an empty slot's entropy is +inf by design, and only outputs must be finite
        bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
        runs.append({"logits": out, **{"rec_" + k: v for k, v in rec.items()}, **{"st_" + k: bits(state[k]) for k in STATE}})
    assert_same_runs(runs, ids=("zero", "nan", "1e30", "plain"))


# ------------------------------------------------------------------------------------------------ 5. update=False
def test_frozen_scoring(dev):
    from clipfs import ops
    T, F, _, _, wstate, _ = _ref(G2)
    T32, F32, state = _dev(T, dev), _dev(F, dev), _new_state(G2, dev)
    ops.tda_adapt(F32, T32, state)
    before = _clone(state)
    out, rec = ops.tda_adapt(F32[:50], T32, state, update=False)
    assert _states_same(state, before)
    frozen = R.TDARef(T, state=R.copy_state(wstate))
    want, _ = frozen.adapt(F[:50], update=False)
    err = np.abs(out.double().cpu().numpy() - want).max()
    print(f"tda frozen: max |logit - fp64| = {err:.2e}")
    assert err <= LOGIT_TOL
    assert (rec["pos_slot"] == -1).all() and (rec["neg_slot"] == -1).all()


# ---------------------------------------------------------------------------------------------------- 6. switches
@pytest.mark.parametrize("caps", [(3, 0), (0, 2), (0, 0)], ids=str)
def test_switches(dev, caps):
    from clipfs import ops
    T, F = _ref(G1)[:2]
    T32, F32 = _dev(T, dev), _dev(F, dev)
    ref = R.TDARef(T, pos_cap=caps[0], neg_cap=caps[1])
    want, wrec = ref.adapt(F)
    state = _new_state(G1, dev, *caps)
    out, rec = ops.tda_adapt(F32, T32, state)
    assert np.abs(out.double().cpu().numpy() - want).max() <= LOGIT_TOL
    assert rec["pred"].tolist() == wrec["pred"].tolist()
    assert (rec["pos_slot"] >= 0).tolist() == (wrec["pos_slot"] >= 0).tolist()
    assert (rec["neg_slot"] >= 0).tolist() == (wrec["neg_slot"] >= 0).tolist()
    assert int(state["counter"]) == len(F)
    if caps == (0, 0):  # out IS the z of the statistics phase: what the full adapter scores against empty caches
        z, _ = ops.tda_adapt(F32, T32, _new_state(G1, dev), update=False)
        assert same_bits(out, z)
        assert np.abs(z.double().cpu().numpy() - wrec["z"]).max() <= 1e-4


def test_fresh_state_single_sample(dev):
    """B = 1 from empty caches: out = z + pos_alpha onehot(pred) - neg_alpha m when in band; the self-affinity is
    exp(0) up to the rounding of f . f."""
    from clipfs import ops
    T, F, _, wrec = _ref(G1)[:4]
    T32, F32 = _dev(T, dev), _dev(F, dev)
    seen = set()
    for b in range(len(F)):
        band = int(wrec["band"][b])
        if band in seen:
            continue
        seen.add(band)
        z, _ = ops.tda_adapt(F32[b:b + 1], T32, _new_state(G1, dev, 0, 0))
        out, rec = ops.tda_adapt(F32[b:b + 1], T32, _new_state(G1, dev))
        want = z.clone()
        want[0, int(rec["pred"][0])] += 2.0
        if band:
            want -= 0.117 * rec["mask"].float()
        assert int(rec["band"][0]) == band and int(rec["pos_slot"][0]) == 0 and int(rec["neg_slot"][0]) == (0 if band else -1)
        assert (out - want).abs().max().item() <= 1e-5
    assert seen == {0, 1}


def test_streams_longer_than_a_call_are_chunked(dev):
    """8200 samples through the adapter = a call of 8192 (the entry point's largest batch: eight passes of the scan's
    staging) and a call of 8, bitwise; and the state is that of 8200 calls' worth of the rule run in 100-row calls."""
    from clipfs import ops
    from tda import MAX_BATCH, TestTimeDynamicAdapter
    T, F, _ = R.clustered(5, MAX_BATCH + 8, 64, 3)
    T32, F32 = _dev(T, dev), _dev(F, dev)
    a = TestTimeDynamicAdapter(T32)
    res = a.adapt_features(F32)
    state = _new_state(G1, dev)
    o1, r1 = ops.tda_adapt(F32[:MAX_BATCH], a.text, state)
    o2, r2 = ops.tda_adapt(F32[MAX_BATCH:], a.text, state)
    assert _states_same(a.state, state) and int(state["counter"]) == MAX_BATCH + 8
    assert same_bits(res.logits, torch.cat([o1, o2])) and same_bits(res.clip_pred, torch.cat([r1["pred"], r2["pred"]]))
    small = _new_state(G1, dev)
    for b0 in range(0, MAX_BATCH + 8, 1000):
        ops.tda_adapt(F32[b0:b0 + 1000], a.text, small)
    assert _states_same(small, state)


# ------------------------------------------------------------------------------------------------- 7. model level
def _tiny_models(dev):
    import modified_resnet_ref as MR
    from clipfs import synth
    from jclip.model import build_model
    vit = build_model(synth.synth_state_dict(synth.TINY, seed=2), device=dev)
    geo = MR.geometries()["RN_TINY"]
    rn = build_model(MR.synth_sd(geo), device=dev)
    return {"vit": (vit, synth.TINY.image_resolution, synth.TINY.context_length, synth.TINY.vocab_size),
            "resnet": (rn, geo.resolution, geo.text.context_length, geo.text.vocab_size)}


@pytest.mark.parametrize("tower", ["vit", "resnet"])
def test_model_level(dev, tower):
    from clipfs import ops, synth
    from tda import TestTimeDynamicAdapter, evaluate_tda
    model, res, ctx_len, vocab = _tiny_models(dev)[tower]
    C = 6
    prompts = synth.synth_captions(C, ctx_len, vocab, seed=4, max_len=10)
    images = synth.synth_images(12, res, seed=3).to(dev)
    a = TestTimeDynamicAdapter(clip_model=model, tokenized_prompts=prompts, n_classes=C)
    b = TestTimeDynamicAdapter(clip_model=model, tokenized_prompts=prompts, n_classes=C)
    got = a.adapt_images(images)
    with torch.no_grad():
        f = ops.l2norm_fwd(model.encode_image(images).float().contiguous())
    want = b.adapt_features(f)
    for x, y in zip(got, want):
        assert same_bits(x, y)
    assert _states_same(a.state, b.state) and torch.isfinite(got.logits).all()
    target = synth.synth_labels(12, C, seed=2)
    a.reset()
    acc = evaluate_tda(model, [(images[:5], target[:5]), (images[5:], target[5:])], a)
    assert acc["n"] == 12 and 0.0 <= acc["top1_clip"] <= 1.0 and 0.0 <= acc["top1_tda"] <= 1.0
    assert int(a.state["counter"]) == 12
