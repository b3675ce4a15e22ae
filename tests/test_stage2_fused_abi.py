"""The fused stage-2 step without a GPU: clipfs_stage2_objective is declared, exported and bound and refuses bad
arguments before launching anything; Stage2Trainer refuses what the fused step does not cover, and the fused-only
arguments without ``fused=True``, before it touches the model."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x40000  # 16-byte aligned, never dereferenced: every call below carries one argument that is refused first
STATE = 0x80000


def _lib():
    from clipfs import _lib
    return _lib.load()


def _call(lib, **kw):
    a = dict(cos=P, zs_logits=P, target=P, img=P, zs_img=P, txt=P, zs_txt=P, dcos=P, dimg=P, dtxt=P, work=P, terms=P,
             correct=P, B=4, C=6, d=8, C_loc=6, inv=0.25, state=None)
    a.update(kw)
    return lib.clipfs_stage2_objective(a["cos"], a["zs_logits"], a["target"], a["img"], a["zs_img"], a["txt"], a["zs_txt"],
                                       a["dcos"], a["dimg"], a["dtxt"], a["work"], a["terms"], a["correct"], a["B"], a["C"],
                                       a["d"], a["C_loc"], a["inv"], a["state"], None)


def _refused(lib, rc, word):
    assert rc == 1, rc  # CLIPFS_EINVAL
    assert word in lib.clipfs_last_error(), lib.clipfs_last_error()


def test_entry_point_is_declared_exported_and_bound():
    from clipfs import _lib, ops
    src = open(os.path.join(ROOT, "include", "clipfs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+clipfs_stage2_objective\s*\(([^)]*)\)", code)
    assert m, "clipfs_stage2_objective is not declared in include/clipfs.h"
    n_args = len(m.group(1).split(","))
    res, args = _lib.SIGNATURES["clipfs_stage2_objective"]
    assert len(args) == n_args == 20
    assert hasattr(_lib.load(), "clipfs_stage2_objective") and callable(ops.stage2_objective)
    # the header cites the reference lines the launch replaces
    doc = src[:src.index("int clipfs_stage2_objective")]
    assert "slow_pace.py:1640,1650-1658,1684-1686" in doc[-3000:]


@pytest.mark.parametrize("name", ["cos", "zs_logits", "target", "img", "zs_img", "txt", "zs_txt", "work", "terms"])
def test_null_pointers_are_refused(name):
    lib = _lib()
    _refused(lib, _call(lib, **{name: None}), b"null pointer")


def test_optional_pointers_and_an_empty_class_block_pass_the_null_check():
    """txt / zs_txt may be NULL only with C_loc = 0: the call then gets as far as the next refusal (a bad size)."""
    lib = _lib()
    _refused(lib, _call(lib, txt=None, zs_txt=None, dtxt=None, C_loc=0, inv=0.0), b"inv_global_batch")
    _refused(lib, _call(lib, dcos=None, dimg=None, dtxt=None, correct=None, inv=0.0), b"inv_global_batch")


@pytest.mark.parametrize("kw,word", [
    (dict(B=0), b"positive"), (dict(B=-3), b"positive"), (dict(C=0, C_loc=0), b"positive"), (dict(C=-1), b"positive"),
    (dict(d=0), b"positive"), (dict(d=-8), b"positive"),
    (dict(C_loc=7), b"C_loc"), (dict(C_loc=-1), b"C_loc"),
    (dict(inv=0.0), b"inv_global_batch"), (dict(inv=-0.5), b"inv_global_batch"), (dict(inv=float("inf")), b"inv_global_batch"),
    (dict(inv=float("nan")), b"inv_global_batch"),
    (dict(cos=P + 2), b"misaligned"), (dict(dimg=P + 1), b"misaligned"), (dict(target=P + 4), b"misaligned"),
    (dict(state=STATE + 4), b"scaler state")])
def test_bad_sizes_and_alignment_are_refused(kw, word):
    lib = _lib()
    _refused(lib, _call(lib, **kw), word)


# ------------------------------------------------------------------------------------------------------ the trainer
class _Adapted(torch.nn.Module):
    """Stands in for a CLIP model with one LoRA projection: the refusal reads parameter names and flags only."""

    def __init__(self):
        super().__init__()
        self.q_proj = torch.nn.Module()
        self.q_proj.w_lora_A = torch.nn.Parameter(torch.zeros(2, 4))
        self.q_proj.w_lora_B = torch.nn.Parameter(torch.zeros(4, 2), requires_grad=False)


def test_fused_refuses_the_moco_branch():
    import slow_pace as S
    for kw in (dict(moco_model=object()), dict(moco_adapter=object()), dict(moco_model=object(), moco_adapter=object())):
        with pytest.raises(ValueError, match="MoCo"):
            S.Stage2Trainer(None, None, None, None, None, fused=True, **kw)


def test_fused_refuses_a_trainable_adapter():
    import slow_pace as S
    with pytest.raises(ValueError, match="q_proj.w_lora_A"):
        S.Stage2Trainer(_Adapted(), None, None, None, None, fused=True)


def test_loss_scale_needs_fused():
    import slow_pace as S
    for kw in (dict(loss_scale=1024.0), dict(loss_scale="dynamic"), dict(loss_scale=1024.0, fused=False)):
        with pytest.raises(ValueError, match="fused=True"):
            S.Stage2Trainer(None, None, None, None, None, **kw)


def test_process_group_needs_fused():
    """A two-rank group (torch's in-process fake backend: no peer, no communication) without fused=True."""
    import torch.distributed as dist
    from torch.testing._internal.distributed.fake_pg import FakeStore
    import slow_pace as S
    assert not dist.is_initialized()
    dist.init_process_group("fake", rank=0, world_size=2, store=FakeStore())
    try:
        with pytest.raises(ValueError, match="fused=True"):
            S.Stage2Trainer(None, None, None, None, None, process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kw", [
    dict(loss_scale=0.0), dict(loss_scale=-2.0), dict(loss_scale=float("inf")), dict(loss_scale=float("nan")),
    dict(loss_scale="static"), dict(loss_scale=True),
    dict(loss_scale="dynamic", growth_factor=1.0), dict(loss_scale="dynamic", backoff_factor=0.0),
    dict(loss_scale="dynamic", backoff_factor=1.0), dict(loss_scale="dynamic", growth_interval=0),
    dict(loss_scale="dynamic", init_scale=0.0)])
def test_bad_scaler_settings_are_refused(kw, fused):
    """Refused by value (lora_train_vlp._check_loss_scale), before the model is looked at; the message names the
    argument, not the missing ``fused``."""
    import slow_pace as S
    with pytest.raises(ValueError) as e:
        S.Stage2Trainer(None, None, None, None, None, fused=fused, **kw)
    assert "fused=True" not in str(e.value)


def test_fused_is_a_stage2_trainer_and_the_default_is_not_fused():
    import inspect
    import slow_pace as S
    assert issubclass(S.FusedStage2Trainer, S.Stage2Trainer)
    names = list(inspect.signature(S.Stage2Trainer.__init__).parameters)
    assert names[-8:] == ["fused", "process_group", "shard_text", "loss_scale", "growth_factor", "backoff_factor",
                          "growth_interval", "init_scale"]
    assert names[:14] == ["self", "clip_model", "prompt_learner", "channel_lp", "zs_image_features", "zs_text_features",
                          "zs_text_feature_sets", "lr", "total_epoch", "weight_decay", "betas", "eps", "moco_model",
                          "moco_adapter"]
    assert list(inspect.signature(S.FusedStage2Trainer.__init__).parameters) == names
    assert list(inspect.signature(S.FusedStage2Trainer.step).parameters) == [
        "self", "images", "target", "index", "template_choice", "global_batch", "row_offset"]
