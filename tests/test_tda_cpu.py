"""The batch algorithm of csrc/tda.hip, modelled in Python (tda_ref.two_phase: statistics -> scan -> intervals -> masked
sums -> write-back), against the sequential TDA rule (tda_ref.TDARef): state exactly equal, logits to 1e-12.  No GPU; this
proves the interval construction before any kernel runs.  Also: the committed seeds satisfy the condition the GPU tests
assert, and the host side of the Python interface."""
import numpy as np
import pytest

import tda_ref as R

# (C, B, d, seed) of the GPU tests
G1 = (5, 70, 64, 1)
G2 = (37, 90, 132, 7)
GEOS = {"G1": G1, "G2": G2}
LOGIT_TOL = 1e-12


def _case(geo):
    C, B, d, seed = geo
    T, F, _ = R.clustered(C, B, d, seed)
    return T, F


def _check(T, F, state, update, **hyper):
    """One call of both models from ``state``; returns the new state."""
    ref = R.TDARef(T, state=R.copy_state(state), **hyper)
    want, wrec = ref.adapt(F, update)
    got, rec, new = R.two_phase(T, F, state, update, **hyper)
    assert np.abs(got - want).max() <= LOGIT_TOL
    assert R.state_equal(new, ref.state())
    for k in ("pred", "band", "pos_slot", "neg_slot", "mask"):
        assert np.array_equal(rec[k], wrec[k]), k
    assert np.array_equal(rec["entropy"], wrec["entropy"])
    if not update:
        assert R.state_equal(new, state)
    return new


@pytest.mark.parametrize("geo", list(GEOS), ids=list(GEOS))
def test_committed_seed_is_well_conditioned(geo):
    T, F = _case(GEOS[geo])
    ref = R.TDARef(T)
    ref.adapt(F)
    assert ref.well_conditioned() == [], ref.events


@pytest.mark.parametrize("caps", [(3, 2), (1, 1), (0, 2), (3, 0), (0, 0), (1, 3)], ids=str)
@pytest.mark.parametrize("geo", list(GEOS), ids=list(GEOS))
def test_two_phase_equals_sequential(geo, caps):
    T, F = _case(GEOS[geo])
    C, d = T.shape
    hyper = dict(pos_cap=caps[0], neg_cap=caps[1])
    _check(T, F, R.empty_state(C, d, *caps), True, **hyper)


@pytest.mark.parametrize("geo", list(GEOS), ids=list(GEOS))
def test_carried_over_state_and_frozen_scoring(geo):
    """Three calls from a carried state equal one call; update=False against a filled state changes nothing."""
    T, F = _case(GEOS[geo])
    C, d = T.shape
    st = R.empty_state(C, d, 3, 2)
    for lo, hi in ((0, 1), (1, 32), (32, len(F))):
        st = _check(T, F[lo:hi], st, True)
    _, _, whole = R.two_phase(T, F, R.empty_state(C, d, 3, 2))
    assert R.state_equal(st, whole)
    _check(T, F[:17], st, False)
    _check(T, F[:17], R.empty_state(C, d, 3, 2), False)


def test_ties_go_to_the_most_recent_and_replacement_is_strict():
    """Identical samples: equal entropies never replace (strict <); a lower entropy replaces the LATEST of equal worst."""
    T, F = _case(G1)
    C, d = T.shape
    same = np.repeat(F[:1], 6, axis=0)
    st = _check(T, same, R.empty_state(C, d, 3, 2), True)
    pred = R.stats(T, F[0], R.DEFAULTS)[2]
    assert sorted(st["pos_seq"][pred].tolist()) == [0, 1, 2]
    H = [R.stats(T, f, R.DEFAULTS)[1] for f in F]
    lower = [f for f, h in zip(F, H) if h < H[0] and R.stats(T, f, R.DEFAULTS)[2] == pred]
    assert lower, "the case needs a sample of the same class with a lower entropy"
    st2 = _check(T, np.stack(lower[:1]), st, True)
    assert sorted(st2["pos_seq"][pred].tolist()) == [0, 1, 6]


def test_adapter_refuses_by_name_without_a_gpu():
    """Constructor refusals that need no device."""
    import torch

    from tda import TestTimeDynamicAdapter
    T = torch.from_numpy(_case(G1)[0]).float()
    with pytest.raises(ValueError, match="pos_capacity"):
        TestTimeDynamicAdapter(T, pos_capacity=3)
    with pytest.raises(ValueError, match="neg_cap"):
        TestTimeDynamicAdapter(T, neg_cap=9)
    with pytest.raises(ValueError, match="text_features"):
        TestTimeDynamicAdapter()
