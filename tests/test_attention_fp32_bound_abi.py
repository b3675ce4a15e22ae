"""The exact-fp32 MFMA attention's length bound and the argument checks of its long-sequence hook, seen at the C ABI without
a GPU.  clipfs_attention_mfma_long_fwd / _bwd take an explicit chunk size and run length (the test hook of the chunk / run
machinery that the default dispatch drives with 0, 0); every bad argument is refused on the host before anything is
launched, with a message that names it.  The addresses below are fake (16-byte aligned, never touched) and the stream is
the null stream, as in tests/test_f16_attention_bound_abi.py."""
import pytest

QKV, DOUT, OUT, LSE, DQKV, WORK = 4096, 8192, 12288, 16384, 20480, 24576


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _fwd(lib, seq, chunk=0, run=0, qkv=QKV):
    return lib.clipfs_attention_mfma_long_fwd(qkv, OUT, LSE, 1, seq, 1, 0, chunk, run, None)


def _bwd(lib, seq, chunk=0, run=0, qkv=QKV):
    return lib.clipfs_attention_mfma_long_bwd(qkv, DOUT, OUT, LSE, DQKV, WORK, 1, seq, 1, 0, chunk, run, None)


def test_max_seq_is_1024(lib):
    from clipfs import ops
    assert lib.clipfs_attention_mfma_max_seq() == ops.attention_mfma_max_seq() == 1024


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("seq", [1025, 96])
def test_seq_outside_the_range_is_refused(lib, call, seq):
    assert call(lib, seq) == 1
    err = lib.clipfs_last_error()
    assert f"seq {seq}".encode() in err and b"97" in err and b"1024" in err


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("chunk", [48, 320])
def test_bad_chunk_tokens_is_refused(lib, call, chunk):
    """48 is no multiple of 32; 320 is past the 288 tokens whose image fits LDS."""
    assert call(lib, 577, chunk=chunk) == 1
    assert f"chunk_tokens {chunk}".encode() in lib.clipfs_last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_run_tiles_above_the_compiled_run_is_refused(lib, call):
    """The message carries the compiled bound, which ops.ATTENTION_MFMA_LONG_RUN mirrors."""
    from clipfs import ops
    run = ops.ATTENTION_MFMA_LONG_RUN
    assert call(lib, 577, run=run + 1) == 1
    err = lib.clipfs_last_error()
    assert f"run_tiles {run + 1}".encode() in err and f"0..{run}".encode() in err
    assert call(lib, 577, run=-1) == 1
    assert b"run_tiles -1" in lib.clipfs_last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_null_qkv_is_refused(lib, call):
    assert call(lib, 577, qkv=None) == 1
    err = lib.clipfs_last_error()
    assert b"null" in err and b"qkv" in err


def test_misaligned_pointer_is_refused(lib):
    assert _fwd(lib, 577, qkv=QKV + 4) == 1
    assert b"misaligned" in lib.clipfs_last_error()
    assert _bwd(lib, 577, qkv=QKV + 4) == 1
    assert b"misaligned" in lib.clipfs_last_error()
