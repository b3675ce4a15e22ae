"""Host side of the GPU training-batch generation (csrc/crops.hip, clipfs/data.py) without a GPU: the C entry point's
argument checks, the split reader and the per-epoch record table (permutation, boxes, flips, batches, rank shards)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sizes:
    """Just what the record table reads from an ImagePool: sizes and names."""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        self.paths = [f"img{i}.jpg" for i in range(len(self.sizes))]

    def __len__(self):
        return len(self.sizes)

    def size(self, i):
        return self.sizes[i]


def _pool(n=37, seed=0):
    rng = np.random.RandomState(seed)
    return _Sizes([(int(rng.randint(60, 700)), int(rng.randint(60, 700))) for _ in range(n)])


def test_crop_batch_is_declared_exported_and_bound():
    from clipfs import _lib
    src = open(os.path.join(ROOT, "include", "clipfs.h")).read()
    assert "int clipfs_crop_batch(" in src
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "clipfs_crop_batch")
    assert "clipfs_crop_batch" in _lib.SIGNATURES
    assert _lib.load().clipfs_abi_version() == 2


def _call(lib, table, recs, pool=16, pool_bytes=1 << 30, out_norm=16, out_raw=None, size=224, src_dev=16, recs_dev=16):
    """Device pointers are dummies: every call here must be refused before anything is launched or dereferenced."""
    table = np.ascontiguousarray(table, dtype=np.int64)
    recs = np.ascontiguousarray(recs, dtype=np.int32)
    return lib.clipfs_crop_batch(pool, pool_bytes, table.ctypes.data, src_dev, table.shape[0], recs.ctypes.data,
                                 recs_dev, recs.shape[0], size, 16, 16, out_norm, out_raw, None)


def test_argument_errors_do_not_touch_the_gpu():
    from clipfs import _lib
    lib = _lib.load()
    table = np.array([[0, 375, 500], [375 * 500 * 3, 3000, 2000]], dtype=np.int64)
    good = np.array([[0, 10, 20, 200, 300, 1, 224, 224, 0, 0, 0, 0]], dtype=np.int32)

    def refused(what, **kw):
        t = kw.pop("table", table)
        r = kw.pop("recs", good)
        assert _call(lib, t, r, **kw) == 1, what
        return lib.clipfs_last_error().decode()

    assert "null" in refused("null pool", pool=None)
    assert "null" in refused("null device table", src_dev=None)
    assert lib.clipfs_crop_batch(16, 1 << 30, None, 16, 2, good.ctypes.data, 16, 1, 224, 16, 16, 16, None, None) == 1
    assert lib.clipfs_crop_batch(16, 1 << 30, table.ctypes.data, 16, 2, None, 16, 1, 224, 16, 16, 16, None, None) == 1
    assert "both outputs" in refused("no output", out_norm=None, out_raw=None)
    r = good.copy()
    r[0, 0] = 2
    assert "source 2 of 2" in refused("src index out of range", recs=r)
    r[0, 0] = -1
    assert "source -1" in refused("negative src index", recs=r)
    r = good.copy()
    r[0, 1] = 375 - 199  # top + h = 376 > 375
    assert "outside" in refused("box below the source", recs=r)
    r = good.copy()
    r[0, 4] = 501
    assert "outside" in refused("box wider than the source", recs=r)
    r = good.copy()
    r[0, 8] = 1  # window 1 + 224 > out_w 224
    assert "window" in refused("window outside the resize", recs=r)
    # a bilinear crop of 2000 px to 24 px needs ceil(2000 / 24) * 2 + 1 = 169 taps
    r = np.array([[1, 0, 0, 3000, 2000, 0, 24, 24, 0, 0, 0, 0]], dtype=np.int32)
    assert "taps" in refused("too many taps", recs=r, size=24)
    t = table.copy()
    t[1] = (t[1, 0], 4097, 2000)
    assert "4096" in refused("source over the side limit", table=t)
    assert "pool" in refused("source outside the pool", pool_bytes=1000)


def test_tap_counts():
    from clipfs import data
    from clipfs.views import BICUBIC, BILINEAR
    assert data.crop_taps(BICUBIC, 4096, 256) == 65       # bicubic centre view of a 4096 px short side
    assert data.crop_taps(BILINEAR, 4096, 224) == 39      # scale-1.0 bilinear crop of a 4096 px side
    assert data.crop_taps(BICUBIC, 4096, 224) == 75 <= data.MAX_TAPS
    assert data.crop_taps(BILINEAR, 3000, 224) == 29 > 24  # beyond clipfs_tta_views' limit
    assert data.crop_taps(BILINEAR, 11, 224) == 3         # upsampling: support stays 1


def test_read_split_keeps_the_class_grouped_order(tmp_path):
    from clipfs import data
    lines = ["a/1.jpg 3", "b/1.jpg 0", "a/2.jpg 3", "c/1.jpg 7", "b/2.jpg 0", "a/3.jpg 3", ""]
    split = tmp_path / "train.txt"
    split.write_text("\n".join(lines))
    paths, labels = data.read_split(str(split), "Dataset")
    assert paths == [os.path.join("Dataset", p) for p in ("a/1.jpg", "a/2.jpg", "a/3.jpg", "b/1.jpg", "b/2.jpg",
                                                           "c/1.jpg")]
    assert labels == [3, 3, 3, 0, 0, 7]


def _loader(pool, **kw):
    from clipfs import data
    return data.TrainLoader(pool, **kw)


def test_every_index_once_per_epoch_and_boxes_inside():
    pool = _pool()
    ld = _loader(pool, batch_size=8, scale=(0.05, 1.0))
    for epoch in range(3):
        t = ld.epoch_records(epoch)
        assert t.shape == (len(pool), 12) and t.dtype == np.int32
        assert sorted(t[:, 0].tolist()) == list(range(len(pool)))
        for r in t:
            h, w = pool.size(int(r[0]))
            assert 0 <= r[1] and r[1] + r[3] <= h and 0 <= r[2] and r[2] + r[4] <= w and r[3] > 0 and r[4] > 0
            assert r[5] in (0, 1) and tuple(r[6:]) == (224, 224, 0, 0, 0, 0)
    flips = np.concatenate([ld.epoch_records(e)[:, 5] for e in range(20)])
    assert 0.35 < flips.mean() < 0.65


def test_table_is_a_function_of_seed_and_epoch():
    pool = _pool()
    a = _loader(pool, seed=5)
    b = _loader(pool, seed=5)
    assert np.array_equal(a.epoch_records(0), b.epoch_records(0))
    assert np.array_equal(a.epoch_records(3), b.epoch_records(3))
    assert not np.array_equal(a.epoch_records(0), a.epoch_records(1))
    assert not np.array_equal(a.epoch_records(0)[:, 0], a.epoch_records(1)[:, 0])
    assert not np.array_equal(a.epoch_records(0), _loader(pool, seed=6).epoch_records(0))
    # no shuffle: pool order, boxes still drawn
    t = _loader(pool, shuffle=False).epoch_records(0)
    assert t[:, 0].tolist() == list(range(len(pool)))


def test_partial_last_batch_and_drop_last():
    pool = _pool(37)
    keep = _loader(pool, batch_size=8)
    drop = _loader(pool, batch_size=8, drop_last=True)
    assert len(keep) == 5 and len(drop) == 4
    tk, td = keep.epoch_records(2), drop.epoch_records(2)
    assert tk.shape[0] == 37 and td.shape[0] == 32
    assert np.array_equal(tk[:32, 0], td[:, 0])  # same permutation, the tail is dropped
    assert [keep.batch_rows(k, 37) for k in range(5)] == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 37)]
    assert [drop.batch_rows(k, 32) for k in range(4)] == [(0, 8), (8, 16), (16, 24), (24, 32)]
    assert len(_loader(pool, batch_size=64, drop_last=True)) == 0
    assert len(_loader(pool, batch_size=64)) == 1


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("drop_last", [False, True])
def test_rank_shards_concatenate_to_the_one_process_table(world, drop_last):
    pool = _pool(37)
    one = _loader(pool, batch_size=10, drop_last=drop_last, seed=9)
    full = one.epoch_records(1)
    ranks = [_loader(pool, batch_size=10, drop_last=drop_last, seed=9, rank=r, world=world) for r in range(world)]
    assert all(len(ld) == len(one) for ld in ranks)
    for k in range(len(one)):
        lo, hi = one.batch_rows(k, full.shape[0])
        parts = []
        for r, ld in enumerate(ranks):
            t = ld.epoch_records(1)
            assert np.array_equal(t, full)  # every rank draws the same global table
            a, b = ld.batch_rows(k, t.shape[0])
            parts.append(t[a:b])
            # rank r's rows start where forward_backward(..., row_offset=) expects them
            from clipfs.dist import shard_bounds
            assert a - lo == shard_bounds(hi - lo, r, world)[0]
        assert np.array_equal(np.concatenate(parts), full[lo:hi])


def test_over_limit_sources_are_refused_when_the_pool_is_built(tmp_path):
    from PIL import Image
    from clipfs import data
    big = np.zeros((4097, 8, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="huge.png"):
        data.ImagePool.from_arrays([np.zeros((8, 8, 3), np.uint8), big], [0, 1], paths=["ok.png", "huge.png"])
    p_ok, p_big = tmp_path / "small.png", tmp_path / "wide_4100.png"
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(p_ok)
    Image.fromarray(np.zeros((4, 4100), np.uint8)).save(p_big)
    with pytest.raises(ValueError, match="wide_4100.png"):
        data.ImagePool.from_files([str(p_ok), str(p_big)], [0, 1])
    with pytest.raises(ValueError, match="uint8"):
        data.ImagePool.from_arrays([np.zeros((8, 8), np.uint8)], [0])


def test_loader_refuses_a_source_its_crop_size_cannot_take():
    pool = _Sizes([(300, 400), (4000, 1200)])
    with pytest.raises(ValueError, match="img1.jpg"):
        _loader(pool, size=96)  # a whole-image box of 4000 px -> 96 px needs 85 taps
    _loader(pool, size=224)
    with pytest.raises(ValueError):
        _loader(pool, outputs=("norm",))


def test_crop_kernel_compiles_without_scratch(tmp_path):
    """The kernel keeps its coefficient tables in LDS: no runtime-indexed per-thread arrays, so no scratch on gfx950."""
    import re
    import subprocess
    pkg = os.path.join(ROOT, "jittor-clip-fewshot_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(pkg, "csrc"), "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", os.path.join(pkg, "csrc", "crops.hip"), "-o",
                        str(tmp_path / "crops.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    log = r.stderr
    assert "crop_batch_kernel" in log
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert scratch and all(v == 0 for v in scratch), log
    assert not re.search(r"VGPRs Spill: [1-9]", log)
