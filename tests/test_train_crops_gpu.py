"""GPU training batches (csrc/crops.hip + clipfs/data.py) against PIL itself, against the TTA view kernel, prefetch
against no prefetch, rank shards against one process, and trainer steps fed from image files through the public
``gpu_train_loader`` entry points.  PIL is the library the reference's CPU loader workers call (jittor.transform); it is
not part of the oracle."""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _image(H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    arr = np.stack([np.sin(xx / 17.0) * 90 + 128, np.cos(yy / 23.0) * 90 + 128, (xx + yy) % 256], -1)
    return np.clip(arr + rng.randint(-30, 30, arr.shape), 0, 255).astype(np.uint8)


def _pil_u8(arr, rec, size):
    """uint8 [3, S, S] of one record through PIL: crop -> resize -> window -> flip."""
    from PIL import Image
    _, top, left, h, w, flip, ow, oh, wx, wy, filt, _ = (int(v) for v in rec)
    im = Image.fromarray(arr).crop((left, top, left + w, top + h))
    im = im.resize((ow, oh), Image.BICUBIC if filt == 1 else Image.BILINEAR)
    im = im.crop((wx, wy, wx + size, wy + size))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im).transpose(2, 0, 1)


def _normalise(u8):
    """The kernel's formula in float32, operation for operation: (u8 - mean * 255) * ((1 / 255) / std)."""
    from clipfs.views import CLIP_MEAN, CLIP_STD
    f32 = np.float32
    mean = np.asarray(CLIP_MEAN, f32).reshape(-1, 1, 1)
    std = np.asarray(CLIP_STD, f32).reshape(-1, 1, 1)
    return (u8.astype(f32) - mean * f32(255)) * ((f32(1) / f32(255)) / std)


def _sources():
    from PIL import Image
    grey = np.asarray(Image.fromarray(_image(300, 420, 7)[..., 0]).convert("L").convert("RGB"))
    return [_image(375, 500, 1), _image(500, 375, 2), _image(224, 224, 3), grey, _image(2000, 3000, 5),
            _image(2731, 4096, 6), _image(40, 57, 8)]


@gpu
def test_batch_matches_pil_bit_exactly(dev):
    from clipfs import data, views
    arrays = _sources()
    pool = data.ImagePool.from_arrays(arrays, list(range(len(arrays))), device=dev)
    rng = np.random.RandomState(0)
    recs = []
    for i, a in enumerate(arrays):
        H, W = a.shape[:2]
        for flip in (0, 1):
            recs.append((i, 0, 0, H, W, flip, 224, 224, 0, 0, views.BILINEAR, 0))  # scale 1.0: the whole image
        for scale in ((0.05, 0.05), (0.05, 1.0), (0.05, 1.0)):
            top, left, h, w = views.sample_crop(W, H, scale, (3 / 4, 4 / 3), rng)
            recs.append((i, top, left, h, w, int(rng.random_sample() < 0.5), 224, 224, 0, 0, views.BILINEAR, 0))
        recs.append((i,) + views.centre_view_record(W, H) + (0,))  # bicubic Resize(256) + CenterCrop(224)
    H, W = arrays[5].shape[:2]
    recs.append((5, 0, 0, H, W, 1, 224, 224, 0, 0, views.BICUBIC, 0))  # bicubic 4096 -> 224: the most taps (75)
    recs = np.asarray(recs, dtype=np.int32)
    taps = [max(data.crop_taps(r[10], r[4], r[6]), data.crop_taps(r[10], r[3], r[7])) for r in recs]
    assert max(taps) == 75 and sum(t > 24 for t in taps) >= 4  # far beyond clipfs_tta_views' 24
    n = recs.shape[0]
    norm = torch.empty(n, 3, 224, 224, device=dev)
    raw = torch.empty(n, 3, 224, 224, device=dev)
    data.crop_batch(pool, recs, 224, norm, raw)
    norm, raw = norm.cpu().numpy(), raw.cpu().numpy()
    for v, r in enumerate(recs):
        want = _pil_u8(arrays[r[0]], r, 224)
        got_raw = raw[v]
        assert np.array_equal(got_raw.view(np.uint32), (want.astype(np.float32) / np.float32(255)).view(np.uint32)), v
        mean = np.float32(views.CLIP_MEAN).reshape(-1, 1, 1)
        std = np.float32(views.CLIP_STD).reshape(-1, 1, 1)
        rec_u8 = np.rint(norm[v] * std * 255.0 + mean * 255.0).astype(np.int64)
        assert np.array_equal(rec_u8, want.astype(np.int64)), (v, tuple(r), np.abs(rec_u8 - want).max())
        assert np.array_equal(norm[v].view(np.uint32), _normalise(want).view(np.uint32)), v
    # one output only: the same values
    only = torch.empty(n, 3, 224, 224, device=dev)
    data.crop_batch(pool, recs, 224, out_raw=only)
    assert np.array_equal(only.cpu().numpy(), raw)


@gpu
def test_same_values_as_the_tta_view_kernel(dev):
    from clipfs import data, views
    arrays = [_image(375, 500, 11), _image(333, 500, 12)]
    pool = data.ImagePool.from_arrays(arrays, [0, 1], device=dev)
    got_all, want_all = [], []
    for i, a in enumerate(arrays):
        H, W = a.shape[:2]
        r10 = views.view_records(W, H, 24, scale=(0.05, 1.0), seed=i)
        want_all.append(views.make_views(torch.from_numpy(a).to(dev), r10).cpu())
        got_all.append(np.concatenate([np.full((len(r10), 1), i, np.int32), r10, np.zeros((len(r10), 1), np.int32)], 1))
    recs = np.concatenate(got_all)
    out = torch.empty(len(recs), 3, 224, 224, device=dev)
    data.crop_batch(pool, recs, 224, out_norm=out)
    assert torch.equal(out.cpu(), torch.cat(want_all))


def _epochs(loader, epochs):
    out = []
    for _ in range(epochs):
        for img, raw, tgt, idx in loader:
            # the consumer's own work on its stream between batches (what the prefetch overlaps)
            x = torch.randn(512, 512, device=tgt.device)
            for _ in range(4):
                x = x @ x * 1e-3
            out.append(tuple(t.clone() if t is not None else None for t in (img, raw, tgt, idx)))
    torch.cuda.synchronize()
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert (s is None) == (t is None)
            if s is not None:
                assert torch.equal(s, t)


@gpu
def test_loader_prefetch_changes_nothing_and_shards_concatenate(dev):
    from clipfs import data
    arrays = [_image(int(h), int(w), s) for s, (h, w) in
              enumerate(np.random.RandomState(3).randint(120, 700, size=(23, 2)))]
    labels = [i % 5 for i in range(len(arrays))]
    pool = data.ImagePool.from_arrays(arrays, labels, device=dev)
    kw = dict(batch_size=8, seed=4, outputs=("clip", "raw"))
    on = _epochs(data.TrainLoader(pool, prefetch=True, **kw), 2)
    off = _epochs(data.TrainLoader(pool, prefetch=False, **kw), 2)
    _same(on, off)
    assert len(on) == 6 and on[2][0].shape[0] == 7  # 23 = 8 + 8 + 7 per epoch
    ld = data.TrainLoader(pool, **kw)
    for k, (img, raw, tgt, idx) in enumerate(on[:3]):
        t = ld.epoch_records(0)[8 * k:8 * k + 8]
        assert idx.cpu().tolist() == t[:, 0].tolist()
        assert tgt.cpu().tolist() == [labels[i] for i in t[:, 0]]
    assert not torch.equal(on[0][3], on[3][3])  # epoch 1 draws a new permutation
    for world in (2, 3):
        shards = [_epochs(data.TrainLoader(pool, rank=r, world=world, **kw), 2) for r in range(world)]
        cat = [tuple(torch.cat([s[k][j] for s in shards]) for j in range(4)) for k in range(len(on))]
        _same(cat, on)


def _write_dataset(root, n_cls=3, per_cls=3, seed=0):
    """A few PNG / JPEG files (one greyscale) and a class-grouped ``train.txt`` in the reference's list format."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n_cls * per_cls):
        lab = i % n_cls
        h, w = (int(v) for v in rng.randint(90, 260, size=2))
        arr = _image(h, w, 100 + i)
        ext = "png" if i % 2 else "jpg"
        rel = os.path.join(f"c{lab}", f"{i}.{ext}")
        os.makedirs(os.path.join(root, f"c{lab}"), exist_ok=True)
        im = Image.fromarray(arr[..., 0]).convert("L") if i == 4 else Image.fromarray(arr)
        im.save(os.path.join(root, rel))
        lines.append(f"{rel} {lab}")
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def _lora_run(dev, root, prefetch, monkeypatch, steps=3):
    torch.manual_seed(0)  # parameter initialisers that draw from torch's generator (VPT, head)
    import test_engine_gpu as T
    import lora_train_vlp as L
    from clipfs import synth
    cfg = synth.SMALL
    _, model = T._build(cfg, dev)
    args = T._args("small", r=4)
    T._apply(model, cfg, args, synth.synth_lora(cfg, 4, seed=5), monkeypatch)
    L.mark_only_lora_as_trainable(model)
    model.train()
    tr = L.LoRATrainer(model)
    captions = synth.synth_captions(3, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev)
    loader = L.gpu_train_loader(str(root), image_dir=str(root), batch_size=3, size=cfg.image_resolution, seed=1,
                                prefetch=prefetch, device=dev)
    losses = []
    while len(losses) < steps:
        for img, raw, tgt, idx in loader:
            assert raw is None and img.shape[1:] == (3, cfg.image_resolution, cfg.image_resolution)
            loss_sum, _, _ = tr.step(img, captions, tgt)
            losses.append(loss_sum.clone())
            if len(losses) == steps:
                break
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in model.parameters()]


@gpu
def test_lora_trainer_fed_from_files_is_the_same_with_and_without_prefetch(dev, tmp_path, monkeypatch):
    _write_dataset(tmp_path)
    l_on, p_on = _lora_run(dev, tmp_path, True, monkeypatch)
    l_off, p_off = _lora_run(dev, tmp_path, False, monkeypatch)
    assert torch.isfinite(l_on).all() and len(l_on) == 3
    assert torch.equal(l_on, l_off)
    assert all(torch.equal(a, b) for a, b in zip(p_on, p_off))


def _stage2_run(dev, root, prefetch, monkeypatch, steps=2):
    torch.manual_seed(0)  # parameter initialisers that draw from torch's generator (VPT, head)
    import test_engine_gpu as T
    import slow_pace as S
    from clipfs import synth
    cfg = synth.SMALL
    _, model = T._build(cfg, dev, n_vpt=4)
    T._apply(model, cfg, T._args("small", r=4), synth.synth_lora(cfg, 4, seed=5), monkeypatch)
    model.eval()
    C, d, N = 3, cfg.embed_dim, 9
    g = torch.Generator().manual_seed(1)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    zs_img = unit(torch.randn(N, d, generator=g, dtype=torch.float64))
    zs_txt = unit(torch.randn(C, d, generator=g, dtype=torch.float64))
    ids = synth.synth_captions(C, cfg.context_length, cfg.vocab_size, seed=4, max_len=12)
    learner = S.VLPromptLearner.__new__(S.VLPromptLearner)
    torch.nn.Module.__init__(learner)
    learner.ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids[0, 1:5].to(dev)].clone())
    learner.tokenized_prompts, learner.n_ctx, learner.n_cls = ids.to(dev), 4, C
    learner._model = [model]
    head = S.Channel_LP(d, C, device=dev)
    with torch.no_grad():
        head.fc.weight.copy_(zs_txt.float())
    tr = S.Stage2Trainer(model, learner, head, zs_img, zs_txt, lr=1e-3, total_epoch=20)
    loader = S.gpu_train_loader(str(root), image_dir=str(root), batch_size=4, size=cfg.image_resolution, seed=2,
                                prefetch=prefetch, device=dev)
    losses = []
    for img, raw, tgt, idx in loader:
        assert img is None and float(raw.min()) >= 0 and float(raw.max()) <= 1
        loss, _, _ = tr.step(S.tfm_clip(raw), tgt, idx, raw_images=raw)
        losses.append(loss.clone())
        if len(losses) == steps:
            break
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in tr.params]


@gpu
def test_stage2_trainer_fed_from_files_is_the_same_with_and_without_prefetch(dev, tmp_path, monkeypatch):
    _write_dataset(tmp_path)
    l_on, p_on = _stage2_run(dev, tmp_path, True, monkeypatch)
    l_off, p_off = _stage2_run(dev, tmp_path, False, monkeypatch)
    assert torch.isfinite(l_on).all() and len(l_on) == 2
    assert torch.equal(l_on, l_off)
    assert all(torch.equal(a, b) for a, b in zip(p_on, p_off))
