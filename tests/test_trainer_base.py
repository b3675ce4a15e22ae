"""The structure of the flat-buffer trainers, without a GPU: ``LoRATrainer`` and ``FusedStage2Trainer`` derive from one
base class that owns the shared step, nothing is borrowed from one trainer by the other, and ``LoRATrainer``'s public
signatures are the ones callers were written against (the fused trainer's are pinned in test_stage2_fused_abi.py)."""
import inspect

import pytest

SHARED = ["optimizer_step", "state_dict", "load_state_dict", "apply_shadow", "restore", "loss_scale_value", "skipped_steps",
          "optimizer_steps", "last_grad_norm", "last_clip_coef", "collective_times_ms"]


def _modules():
    import lora_train_vlp as L
    import slow_pace as S
    return L, S


def test_both_trainers_derive_from_the_one_base():
    L, S = _modules()
    base = L.FlatStepTrainer
    assert issubclass(L.LoRATrainer, base) and issubclass(S.FusedStage2Trainer, base)
    assert issubclass(S.FusedStage2Trainer, S.Stage2Trainer)
    assert not issubclass(S.Stage2Trainer, base)  # the unfused trainer stays the autograd-route step
    assert not issubclass(S.FusedStage2Trainer, L.LoRATrainer) and not issubclass(L.LoRATrainer, S.Stage2Trainer)
    assert S.FlatStepTrainer is base  # slow_pace imports the base, not a copy
    assert base.__doc__ and "self.flat" in base.__doc__ and "self.model" in base.__doc__  # the contract is written down


def test_the_fused_trainer_borrows_nothing_from_loratrainer():
    _, S = _modules()
    for name, obj in vars(S.FusedStage2Trainer).items():
        fn = obj.fget if isinstance(obj, property) else getattr(obj, "__func__", obj)
        qual = getattr(fn, "__qualname__", "")
        assert not qual.startswith("LoRATrainer."), f"FusedStage2Trainer.{name} is {qual}"


@pytest.mark.parametrize("name", SHARED)
def test_shared_members_are_the_base_class_own(name):
    L, S = _modules()
    base = L.FlatStepTrainer
    assert name in vars(base), f"{name} is not defined on FlatStepTrainer"
    own = vars(base)[name]
    for cls in (L.LoRATrainer, S.FusedStage2Trainer):
        owner = next(k for k in cls.__mro__ if name in vars(k))
        assert owner is base, f"{cls.__name__}.{name} comes from {owner.__name__}"
        assert inspect.getattr_static(cls, name) is own


def test_loratrainer_signatures():
    L, _ = _modules()
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(L.LoRATrainer.__init__) == [
        "self", "model", "lr", "weight_decay", "betas", "eps", "logit_scale", "prompt_ctx", "process_group", "shard_text",
        "loss_scale", "growth_factor", "backoff_factor", "growth_interval", "init_scale", "max_grad_norm", "ema_decay"]
    assert params(L.LoRATrainer.forward_backward) == [
        "self", "images", "captions", "target", "templates_per_class", "global_batch", "row_offset"]
    assert params(L.LoRATrainer.step) == [
        "self", "images", "captions", "target", "templates_per_class", "global_batch", "row_offset"]
    assert params(L.LoRATrainer.optimizer_step) == ["self"]
