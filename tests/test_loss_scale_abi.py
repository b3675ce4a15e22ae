"""Loss scaling without a GPU: the four entry points refuse bad arguments before launching anything, and LoRATrainer
refuses bad scaler settings before it touches the model."""
import pytest

STATE = 0x10000  # never dereferenced: every call below carries one argument that is refused first
BUF = 0x20000


def _lib():
    from clipfs import _lib
    return _lib.load()


def _refused(lib, rc, word):
    assert rc == 1, rc  # CLIPFS_EINVAL
    assert word in lib.clipfs_last_error(), lib.clipfs_last_error()


def test_grads_nonfinite_refusals():
    lib = _lib()
    _refused(lib, lib.clipfs_grads_nonfinite(BUF, 8, None, None), b"scaler state")
    _refused(lib, lib.clipfs_grads_nonfinite(BUF, 8, STATE + 4, None), b"scaler state")  # record not 16-byte aligned
    _refused(lib, lib.clipfs_grads_nonfinite(None, 8, STATE, None), b"gradient pointer")
    _refused(lib, lib.clipfs_grads_nonfinite(BUF + 2, 8, STATE, None), b"gradient pointer")  # not a float address
    _refused(lib, lib.clipfs_grads_nonfinite(BUF, 0, STATE, None), b"n = 0")


def test_scaler_decide_refusals():
    lib = _lib()
    _refused(lib, lib.clipfs_scaler_decide(None, 2e-4, 0.9, 0.999, 2.0, 0.5, 2000, None), b"scaler state")
    _refused(lib, lib.clipfs_scaler_decide(STATE + 8, 2e-4, 0.9, 0.999, 2.0, 0.5, 2000, None), b"scaler state")
    _refused(lib, lib.clipfs_scaler_decide(STATE, 2e-4, 0.9, 0.999, 0.5, 0.5, 2000, None), b"growth_factor")
    _refused(lib, lib.clipfs_scaler_decide(STATE, 2e-4, 0.9, 0.999, 2.0, 0.0, 2000, None), b"backoff_factor")
    _refused(lib, lib.clipfs_scaler_decide(STATE, 2e-4, 0.9, 0.999, 2.0, 1.5, 2000, None), b"backoff_factor")
    _refused(lib, lib.clipfs_scaler_decide(STATE, 2e-4, 0.9, 0.999, 2.0, 0.5, -1, None), b"growth_interval")


def test_adamw_scaled_refusals():
    lib = _lib()
    a = (2e-4, 0.9, 0.999, 1e-8, 1e-2)
    _refused(lib, lib.clipfs_adamw_scaled(BUF, BUF, BUF, BUF, 8, *a, None, None), b"scaler state")
    _refused(lib, lib.clipfs_adamw_scaled(BUF, None, BUF, BUF, 8, *a, STATE, None), b"pointer")
    _refused(lib, lib.clipfs_adamw_scaled(BUF, BUF + 1, BUF, BUF, 8, *a, STATE, None), b"pointer")
    _refused(lib, lib.clipfs_adamw_scaled(None, BUF, BUF, BUF, 8, *a, STATE, None), b"pointer")
    _refused(lib, lib.clipfs_adamw_scaled(BUF, BUF, BUF, BUF, 0, *a, STATE, None), b"n = 0")


def test_cross_entropy_scaled_refusals():
    lib = _lib()
    _refused(lib, lib.clipfs_cross_entropy_scaled(BUF, BUF, BUF, BUF, BUF, None, 4, 6, 1.0, None, None), b"scaler state")
    _refused(lib, lib.clipfs_cross_entropy_scaled(BUF, BUF, BUF, BUF, BUF, None, 4, 6, 1.0, STATE + 4, None), b"scaler state")
    _refused(lib, lib.clipfs_cross_entropy_scaled(None, BUF, BUF, BUF, BUF, None, 4, 6, 1.0, STATE, None), b"bad args")
    _refused(lib, lib.clipfs_cross_entropy_scaled(BUF, BUF, BUF, BUF, BUF, None, 0, 6, 1.0, STATE, None), b"bad args")


def test_record_layout_matches_the_header():
    """The word indices of clipfs/_lib.py are the CLIPFS_SCALER_* of include/clipfs.h."""
    import os
    import re
    from clipfs import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "clipfs.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define CLIPFS_SCALER_([A-Z0-9_]+) (\d+)", src)}
    assert len(header) == 10 and header["WORDS"] == 16
    assert header == {k: getattr(_lib, "SCALER_" + k) for k in header}
    assert len({v for k, v in header.items() if k != "WORDS"}) == 9  # nine distinct words


@pytest.mark.parametrize("kw", [
    dict(loss_scale=0.0), dict(loss_scale=-2.0), dict(loss_scale=float("inf")), dict(loss_scale=float("nan")),
    dict(loss_scale="static"), dict(loss_scale=True),
    dict(loss_scale="dynamic", growth_factor=1.0), dict(loss_scale="dynamic", growth_factor=0.5),
    dict(loss_scale="dynamic", backoff_factor=0.0), dict(loss_scale="dynamic", backoff_factor=1.0),
    dict(loss_scale="dynamic", backoff_factor=1.5), dict(loss_scale="dynamic", backoff_factor=-0.5),
    dict(loss_scale="dynamic", growth_interval=0), dict(loss_scale="dynamic", init_scale=0.0)])
def test_trainer_rejects_bad_scaler_settings(kw):
    """Refused by value, before the model is looked at (none is needed to get here)."""
    import lora_train_vlp as L
    with pytest.raises(ValueError):
        L.LoRATrainer(None, **kw)
