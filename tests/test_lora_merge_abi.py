"""clipfs_lora_merge at the C ABI, without a GPU: every refusal is made on the HOST copy of the job table before anything
is enqueued, returns CLIPFS_EINVAL (1) and names the job index and the field.  The addresses below are fake: the
host-side checks never dereference them, and no call here gets as far as a launch."""
import ctypes

import pytest

W, A, B, OUT, PLANES, TABLE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _table(*jobs):
    """A well-formed table of (n, k, nseg, seg_mask) jobs with its tile prefix."""
    from clipfs import _lib
    t = (_lib.MergeJob * len(jobs))()
    tile0 = 0
    for rec, (n, k, nseg, mask) in zip(t, jobs):
        rec.w, rec.a, rec.b, rec.out, rec.planes = W, A, B, OUT, None
        rec.n, rec.k, rec.nseg, rec.seg_mask, rec.tile0 = n, k, nseg, mask, tile0
        tile0 += _lib.merge_job_tiles(n, k, nseg)
    return t


def _call(lib, t, njobs=None, size=None, r=4, fmt=0, dev=TABLE):
    from clipfs import _lib
    rc = lib.clipfs_lora_merge(t, dev, len(t) if njobs is None else njobs,
                               ctypes.sizeof(_lib.MergeJob) if size is None else size, r, 0.5, fmt, None)
    return rc, lib.clipfs_last_error().decode()


def _refused(lib, t, *words, **kw):
    rc, msg = _call(lib, t, **kw)
    assert rc == 1, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)
    return msg


def test_struct_matches_the_header():
    from clipfs import _lib
    assert ctypes.sizeof(_lib.MergeJob) == 64  # 5 pointers + 6 ints: the layout of struct clipfs_lora_merge_job
    assert (_lib.MERGE_TILE_ROWS, _lib.MERGE_TILE_COLS) == (32, 256)
    assert _lib.merge_job_tiles(2304, 768, 3) == 3 * 24 * 3
    assert _lib.merge_job_tiles(72, 40, 1) == 3
    assert _lib.merge_job_tiles(216, 264, 3) == 3 * 3 * 2  # 72-row segments: a tile never crosses a segment


def test_struct_size_and_table(lib):
    t = _table((192, 64, 3, 7))
    _refused(lib, t, "struct_size", size=56)
    _refused(lib, t, "struct_size", size=72)
    _refused(lib, t, "njobs", njobs=0)
    _refused(lib, t, "njobs", njobs=-1)
    _refused(lib, t, "null job table", dev=None)
    rc = lib.clipfs_lora_merge(None, TABLE, 1, 64, 4, 0.5, 0, None)
    assert rc == 1 and "null job table" in lib.clipfs_last_error().decode()
    _refused(lib, t, "plane_format", fmt=3)


@pytest.mark.parametrize("r", [0, 65, -1])
def test_rank_range(lib, r):
    _refused(lib, _table((192, 64, 3, 7)), "r %d" % r, r=r)


@pytest.mark.parametrize("field", ["w", "a", "b", "out"])
def test_null_and_misaligned_pointers(lib, field):
    t = _table((192, 64, 3, 7), (512, 128, 1, 1))
    setattr(t[1], field, None)
    _refused(lib, t, "job 1", f"{field} is NULL")
    setattr(t[1], field, 0x70004)
    _refused(lib, t, "job 1", f"{field} is not 16-byte aligned")


def test_planes(lib):
    t = _table((192, 64, 3, 7))
    t[0].planes = PLANES + 8
    _refused(lib, t, "job 0", "planes is not 16-byte aligned", fmt=2)
    t[0].planes = PLANES
    _refused(lib, t, "job 0", "planes", "plane_format 0", fmt=0)


def test_out_must_not_alias_w(lib):
    t = _table((192, 64, 3, 7), (512, 128, 1, 1), (128, 512, 1, 1))
    t[2].out = t[2].w
    _refused(lib, t, "job 2", "out aliases w")


def test_shapes(lib):
    t = _table((72, 40, 1, 1))
    t[0].k = 36
    _refused(lib, t, "job 0", "k 36")
    for nseg in (2, 0, 4):
        t = _table((192, 64, 3, 7), (192, 64, 1, 1))
        t[1].nseg = nseg
        _refused(lib, t, "job 1", "nseg %d" % nseg)
    t = _table((192, 64, 3, 7))
    t[0].n = 193
    _refused(lib, t, "job 0", "n 193", "nseg 3")
    t = _table((192, 64, 3, 7))
    t[0].n = 0
    _refused(lib, t, "job 0", "n 0")


def test_seg_mask(lib):
    for nseg, mask in ((3, 0), (3, 8), (1, 0), (1, 2), (3, 0x17)):
        t = _table((192, 64, 3, 7), (192, 64, nseg, 1))
        t[1].seg_mask = mask
        _refused(lib, t, "job 1", "seg_mask 0x%x" % mask)


def test_tile_prefix(lib):
    t = _table((192, 64, 3, 7), (512, 128, 1, 1))
    t[1].tile0 += 1
    _refused(lib, t, "job 1", "tile0")
    t = _table((192, 64, 3, 7))
    t[0].tile0 = 1
    _refused(lib, t, "job 0", "tile0")
