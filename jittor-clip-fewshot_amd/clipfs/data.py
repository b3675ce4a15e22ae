"""Few-shot training batches made on the GPU from a device-resident image pool (csrc/crops.hip).

The reference makes every training batch on 8 CPU workers with PIL (lora_train_vlp.py:1196-1218, slow_pace.py:
1903-1935): decode, RandomResizedCrop(224, scale=(0.05, 1)), RandomHorizontalFlip, [ImageNormalize], ToTensor, upload.
The few-shot training set is small (1 495 images), so here every image is decoded ONCE into a uint8 HWC pool in HBM
(``ImagePool``) and an epoch needs no host pixel work: ``TrainLoader`` samples the crop boxes on the host (integer work,
``views.sample_crop``) and one kernel launch per batch writes the crops, PIL-exact, as the CLIP-normalised batch and / or
the [0, 1] batch the stage-2 MoCo branch reads.

Reproducibility: the permutation, boxes and flips of an epoch are a function of ``(seed, epoch)`` only; every rank of a
data-parallel run draws the same global table and generates its own rows of each global batch (``dist.shard_bounds``,
the ``row_offset`` layout of ``LoRATrainer.forward_backward``).  Jittor's own random stream cannot be reproduced.
"""
from __future__ import annotations

import math
import os
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .dist import shard_bounds
from .streams import side_stream
from .views import BILINEAR, CLIP_MEAN, CLIP_STD, sample_crop

MAX_SIDE = 4096  # largest source side the kernel takes (CROP_MAX_SIDE of csrc/crops.hip)
MAX_TAPS = 80    # filter taps per axis the kernel takes (CROP_KMAX of csrc/crops.hip)
REC_COLS = 12    # int32 columns of a crop record (CropRec of csrc/crops.hip)
MAX_THREADS = 16


def crop_taps(filt: int, in_size: int, out_size: int) -> int:
    """Pillow's ksize for in_size -> out_size: ceil(support * max(in / out, 1)) * 2 + 1 (the kernel's bound too)."""
    scale = in_size / out_size
    return int(math.ceil((1.0 if filt == BILINEAR else 2.0) * max(scale, 1.0))) * 2 + 1


def read_split(split_path: str, image_dir: str = "") -> Tuple[List[str], List[int]]:
    """``path label`` per line (the reference's ``JtDataset.read_split``, lora_train_vlp.py:1094-1104) -> (paths, labels)
    grouped by class in order of each class's first appearance, file order inside a class.  The position in this list
    is the sample ``index`` the loader returns (stage 2 indexes its cached zero-shot features by it)."""
    groups = defaultdict(list)
    with open(split_path) as f:
        for line in f:
            if not line.strip():
                continue
            path, label = line.strip().split()
            groups[int(label)].append(os.path.join(image_dir, path))
    paths = [p for _, ps in groups.items() for p in ps]
    labels = [lab for lab, ps in groups.items() for _ in ps]
    return paths, labels


def _check_size(h: int, w: int, name: str) -> None:
    if not (0 < h <= MAX_SIDE and 0 < w <= MAX_SIDE):
        raise ValueError(f"image {name!r} is {w} x {h}: the GPU crop kernel takes sources up to {MAX_SIDE} px per side")


class ImagePool:
    """Every source image once, uint8 HWC, back to back in one device buffer; ``table`` int64 [n, 3] = {byte offset,
    height, width} (host and device copies), ``labels`` int64 [n] (device), ``paths`` their names."""

    def __init__(self, data: torch.Tensor, table: np.ndarray, labels: Sequence[int], paths: Sequence[str]):
        assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1
        self.data = data
        self.device = data.device
        self.table = np.ascontiguousarray(table, dtype=np.int64)
        self.table_dev = torch.from_numpy(self.table).to(self.device)
        self.labels_host = np.asarray(labels, dtype=np.int64)
        self.labels = torch.from_numpy(self.labels_host).to(self.device)
        self.paths = list(paths)
        assert self.table.shape == (len(self.paths), 3) == (len(self.labels_host), 3)

    def __len__(self) -> int:
        return self.table.shape[0]

    def size(self, i: int) -> Tuple[int, int]:
        """(height, width) of source ``i``."""
        return int(self.table[i, 1]), int(self.table[i, 2])

    def image(self, i: int) -> torch.Tensor:
        """uint8 [H, W, 3] device view of source ``i``."""
        off, h, w = (int(v) for v in self.table[i])
        return self.data[off:off + h * w * 3].view(h, w, 3)

    @classmethod
    def _build(cls, n: int, sizes: Sequence[Tuple[int, int]], fill, labels, paths, device) -> "ImagePool":
        for (h, w), name in zip(sizes, paths):
            _check_size(h, w, name)
        if len(labels) != n:
            raise ValueError(f"{n} images but {len(labels)} labels")
        table = np.zeros((n, 3), dtype=np.int64)
        off = 0
        for i, (h, w) in enumerate(sizes):
            table[i] = (off, h, w)
            off += h * w * 3
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        data = torch.empty(max(off, 1), dtype=torch.uint8, device=device)
        fill(data, table)
        return cls(data, table, labels, paths)

    @classmethod
    def from_arrays(cls, arrays, labels: Sequence[int], paths: Optional[Sequence[str]] = None,
                    device=None) -> "ImagePool":
        """uint8 [H, W, 3] numpy arrays or tensors (host or device)."""
        arrays = list(arrays)
        paths = list(paths) if paths is not None else [f"array[{i}]" for i in range(len(arrays))]
        sizes = []
        for a, name in zip(arrays, paths):
            ok = a.dtype == torch.uint8 if torch.is_tensor(a) else a.dtype == np.uint8
            if not ok or len(a.shape) != 3 or a.shape[2] != 3:
                raise ValueError(f"image {name!r}: expected uint8 [H, W, 3], got {a.dtype} {tuple(a.shape)}")
            sizes.append((int(a.shape[0]), int(a.shape[1])))

        def fill(data, table):
            for a, (off, h, w) in zip(arrays, table):
                t = a if torch.is_tensor(a) else torch.from_numpy(np.array(a, copy=not a.flags.writeable, order="C"))
                data[off:off + h * w * 3].copy_(t.reshape(-1))

        return cls._build(len(arrays), sizes, fill, labels, paths, device)

    @classmethod
    def from_files(cls, paths: Sequence[str], labels: Sequence[int], threads: int = 8, device=None) -> "ImagePool":
        """Decodes each file once (PIL ``.convert("RGB")``, as the reference's ``read_image``) on at most 16 threads and
        uploads it.  Sizes are read from the headers first, so an over-size image is refused before any decode."""
        from PIL import Image
        paths = list(paths)
        sizes = []
        for p in paths:
            with Image.open(p) as im:
                sizes.append((im.height, im.width))
        threads = max(1, min(int(threads), MAX_THREADS))

        def decode(p):
            with Image.open(p) as im:
                return np.array(im.convert("RGB"))

        def fill(data, table):
            with ThreadPoolExecutor(max_workers=threads) as ex:
                for (off, h, w), a, p in zip(table, ex.map(decode, paths), paths):
                    if a.shape != (h, w, 3):
                        raise ValueError(f"image {p!r} decoded to {a.shape}, its header says {(h, w)}")
                    data[off:off + h * w * 3].copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))

        return cls._build(len(paths), sizes, fill, labels, paths, device)


def crop_batch(pool: ImagePool, recs: np.ndarray, size: int = 224, out_norm: Optional[torch.Tensor] = None,
               out_raw: Optional[torch.Tensor] = None, mean: Sequence[float] = CLIP_MEAN,
               std: Sequence[float] = CLIP_STD) -> None:
    """One launch of clipfs_crop_batch on the current stream: int32 [n, 12] records -> ``out_norm`` and / or ``out_raw``
    (contiguous fp32 [n, 3, size, size] on the pool's device)."""
    from .views import _norm_constants
    recs = np.ascontiguousarray(recs, dtype=np.int32)
    n = recs.shape[0]
    if recs.ndim != 2 or recs.shape[1] != REC_COLS:
        raise ValueError(f"crop_batch: records must be int32 [n, {REC_COLS}], got {recs.shape}")
    dev = pool.device
    for o in (out_norm, out_raw):
        if o is not None and (tuple(o.shape) != (n, 3, size, size) or o.dtype != torch.float32 or not o.is_contiguous()
                              or o.device != dev):
            raise ValueError(f"crop_batch: outputs must be contiguous fp32 [{n}, 3, {size}, {size}] tensors on {dev}")
    # pinned: the upload does not wait for the device (the host pointer is what the library validates)
    host = torch.from_numpy(recs).pin_memory()
    recs_dev = host.to(dev, non_blocking=True)
    m, s = _norm_constants(dev, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    ptr = lambda t: t.data_ptr() if t is not None else None
    check(_lib.load().clipfs_crop_batch(pool.data.data_ptr(), pool.data.numel(), pool.table.ctypes.data,
                                        pool.table_dev.data_ptr(), len(pool), host.data_ptr(), recs_dev.data_ptr(), n,
                                        size, m.data_ptr(), s.data_ptr(), ptr(out_norm), ptr(out_raw),
                                        torch.cuda.current_stream(dev).cuda_stream), "crop_batch")


class TrainLoader:
    """One epoch per iteration of ``(images, raw, target, index)``: fp32 [b, 3, size, size] CLIP-normalised and [0, 1]
    batches (``None`` for an output not in ``outputs``), int64 [b] labels and pool indices, all on the pool's device,
    ``b`` = this rank's rows of the global batch.  The yielded tensors live in two loader-owned buffers: a batch stays
    valid until the consumer asks for the batch after next (clone it to keep it longer).

    ``prefetch``: batch k+1 is generated on the process's side stream (clipfs/streams.py) while the caller's stream runs
    step k; the side stream waits for an event recorded on the caller's stream before it overwrites a buffer, and the
    caller's stream waits for the batch it receives.  The values are the same with and without prefetch."""

    def __init__(self, pool: ImagePool, batch_size: int = 256, scale=(0.05, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
                 flip_p: float = 0.5, size: int = 224, shuffle: bool = True, drop_last: bool = False, seed: int = 0,
                 outputs: Sequence[str] = ("clip",), rank: int = 0, world: int = 1, prefetch: bool = True,
                 mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD):
        outputs = tuple(outputs)
        if not outputs or any(o not in ("clip", "raw") for o in outputs):
            raise ValueError(f"outputs must be a non-empty subset of ('clip', 'raw'), got {outputs}")
        if batch_size <= 0 or size <= 0 or not (0 <= rank < world):
            raise ValueError(f"bad loader shape: batch_size {batch_size}, size {size}, rank {rank} of {world}")
        self.pool, self.batch_size, self.scale, self.ratio = pool, int(batch_size), tuple(scale), tuple(ratio)
        self.flip_p, self.size, self.shuffle, self.drop_last, self.seed = flip_p, int(size), shuffle, drop_last, seed
        self.outputs, self.rank, self.world, self.prefetch = outputs, rank, world, prefetch
        self.mean, self.std = tuple(mean), tuple(std)
        self.epoch = 0
        # the largest box of a source is the whole image: refuse here, never in the middle of an epoch
        for i in range(len(pool)):
            h, w = pool.size(i)
            taps = crop_taps(BILINEAR, max(h, w), self.size)
            if taps > MAX_TAPS:
                raise ValueError(f"image {pool.paths[i]!r} ({w} x {h}) needs {taps} filter taps for a {self.size} px "
                                 f"crop (at most {MAX_TAPS})")
        self._bufs = None

    def __len__(self) -> int:
        n = len(self.pool)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        """The epoch the next iteration draws (it advances by one after each iteration)."""
        self.epoch = int(epoch)

    def epoch_records(self, epoch: int) -> np.ndarray:
        """int32 [N, 12] global record table of ``epoch`` (N = len(self) * batch_size with drop_last, else the pool
        size): row j is sample j of the epoch; column 0 is its pool index."""
        n = len(self.pool)
        rng = np.random.RandomState([int(self.seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF])
        order = rng.permutation(n) if self.shuffle else np.arange(n)
        if self.drop_last:
            order = order[:len(self) * self.batch_size]
        recs = np.zeros((len(order), REC_COLS), dtype=np.int32)
        for j, i in enumerate(order):
            h, w = self.pool.size(int(i))
            top, left, bh, bw = sample_crop(w, h, self.scale, self.ratio, rng)
            flip = int(rng.random_sample() < self.flip_p)
            recs[j] = (i, top, left, bh, bw, flip, self.size, self.size, 0, 0, BILINEAR, 0)
        return recs

    def batch_rows(self, k: int, n_rows: int) -> Tuple[int, int]:
        """[lo, hi) rows of the epoch table this rank generates for batch k."""
        b0 = k * self.batch_size
        b1 = min(b0 + self.batch_size, n_rows)
        lo, hi = shard_bounds(b1 - b0, self.rank, self.world)
        return b0 + lo, b0 + hi

    def _buffers(self):
        if self._bufs is None:
            rows = -(-self.batch_size // self.world) if self.world > 1 else self.batch_size
            dev, S = self.pool.device, self.size

            def one():
                img = torch.empty(rows, 3, S, S, device=dev) if "clip" in self.outputs else None
                raw = torch.empty(rows, 3, S, S, device=dev) if "raw" in self.outputs else None
                return img, raw, torch.empty(rows, dtype=torch.int64, device=dev), torch.empty(rows, dtype=torch.int64,
                                                                                                device=dev)
            self._bufs = [one(), one()]
            from .views import _norm_constants  # made here, on the caller's stream, not inside the side-stream launch
            _norm_constants(dev, tuple(float(v) for v in self.mean), tuple(float(v) for v in self.std))
        return self._bufs

    def _generate(self, recs: np.ndarray, buf):
        img, raw, tgt, idx = buf
        b = recs.shape[0]
        img, raw, tgt, idx = (t[:b] if t is not None else None for t in (img, raw, tgt, idx))
        if b:
            crop_batch(self.pool, recs, self.size, img, raw, self.mean, self.std)
            idx.copy_(torch.from_numpy(recs[:, 0].astype(np.int64)).pin_memory(), non_blocking=True)
            torch.index_select(self.pool.labels, 0, idx, out=tgt)
        return img, raw, tgt, idx

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        table = self.epoch_records(epoch)
        nb = len(self)
        if nb == 0:
            return
        dev = self.pool.device
        bufs = self._buffers()
        gen = side_stream(dev) if self.prefetch else None
        # event on the caller's stream: its work on the buffer's last batch is issued before it.  At the start of an
        # epoch both buffers may still be read by the caller's earlier steps (of the last epoch, or of one left early).
        start = torch.cuda.Event()
        start.record(torch.cuda.current_stream(dev))
        free = [start, start]
        ready = [None, None]  # event on the side stream: the buffer's batch is written
        out = [None, None]

        def launch(k):
            s = k % 2
            lo, hi = self.batch_rows(k, table.shape[0])
            if gen is None:
                out[s] = self._generate(table[lo:hi], bufs[s])
                return
            with torch.cuda.stream(gen):
                gen.wait_event(free[s])
                out[s] = self._generate(table[lo:hi], bufs[s])
                ready[s] = torch.cuda.Event()
                ready[s].record(gen)

        if gen is not None:
            launch(0)
        for k in range(nb):
            s = k % 2
            caller = torch.cuda.current_stream(dev)
            if gen is None:
                launch(k)
            else:
                if k + 1 < nb:
                    if k >= 1:  # buffer (k + 1) % 2 held batch k - 1, whose consumer has issued its work by now
                        free[(k + 1) % 2] = torch.cuda.Event()
                        free[(k + 1) % 2].record(caller)
                    launch(k + 1)
                caller.wait_event(ready[s])
            yield out[s]
