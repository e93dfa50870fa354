"""GPU: the augmented input chain (ubdvss_amd/augmentation.py, SegmapManager.prepare_batches_on_device; reference
augmentation.py:50-85 + segmap_manager.py:24-39) against the host chain the reference runs, with the same plan, bit for bit:
Pillow rotate -> crop -> quarter turn -> perspective transform, then _rescale_image_and_markup -> convert('L') for grey nets
-> build_segmentation_map.  Images, label maps and markups are compared exactly.  The imgaug photometric stage is not built
and not tested.  One training smoke on an augmented batch (finite loss, no accuracy claim)."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from ubdvss_amd import (NetConfig, SegmapManager, ObjectMarkup, ClassifiedObjectMarkup, Model, Trainer, SegLinksImageAugmentation,
                        synthetic)
from ubdvss_amd import augmentation as aug

pytestmark = pytest.mark.gpu


def _pillow_chain(im, plan):
    for st in plan.stages:
        if st.kind in ("rotate", "quarter"):
            im = im.rotate(st.params["angle"], Image.BILINEAR, expand=True)
        elif st.kind == "crop":
            im = im.crop(st.params["box"])
        else:
            im = im.transform(im.size, Image.PERSPECTIVE, st.params["coeffs"], Image.BILINEAR)
        assert im.size == tuple(st.size), (im.size, st)
    return im


def _host_path(im, markup, plan, cfg):
    """what the reference does with this plan: (image array (h, w, c_in), label map, rescaled markup)"""
    im2 = _pillow_chain(im, plan)
    mk2 = aug.apply_plan_to_markup(plan, markup)
    im3, mk3 = SegmapManager._rescale_image_and_markup(im2, mk2, cfg)
    seg = SegmapManager.build_segmentation_map(im3, mk3 or [], scale=cfg.get_scale())
    if cfg.is_grey():
        im3 = im3.convert("L")
    a = np.asarray(im3)
    return (a[..., None] if a.ndim == 2 else a), np.asarray(seg, dtype=np.int32), mk3


def _cases(n_min=40, classified_every=2, grey_sources=False):
    """seeded (image array, markup, plan) triples whose plans together contain every stage combination; markup from
    synthetic.random_quads (no folded quads); the second image has no markup"""
    rs = np.random.default_rng(5)
    out, combos, seed = [], set(), 0
    while len(out) < n_min or len(combos) < 16:
        seed += 1
        h, w = int(rs.integers(200, 700)), int(rs.integers(200, 700))
        c = 1 if grey_sources and seed % 3 == 0 else 3
        a = rs.integers(0, 256, (h, w, c), dtype=np.uint8)
        quads = synthetic.random_quads(rs, h, w, n_min=1, n_max=5, side_min=12, side_max=50)
        if seed % classified_every == 0:
            mk = [ClassifiedObjectMarkup(q.reshape(-1), int(rs.integers(0, 3))) for q in quads]
        else:
            mk = [ObjectMarkup(q.reshape(-1).tolist()) for q in quads]
        if len(out) == 1:
            mk = []
        plan = aug.sample_plan((w, h), mk, random.Random(seed), np.random.RandomState(seed))
        kinds = tuple(s.kind for s in plan.stages)
        if mk and (plan.original or (kinds in combos and len(out) >= n_min)):
            continue
        if mk:
            combos.add(kinds)
        out.append((a, mk, plan))
    return out


def _pil(a):
    return Image.fromarray(a[..., 0] if a.shape[2] == 1 else a, "L" if a.shape[2] == 1 else "RGB")


def test_device_chain_equals_pillow_chain():
    cases = _cases()
    assert len(cases) >= 40 and len({tuple(s.kind for s in p.stages) for _, mk, p in cases if mk}) == 16
    got = aug.augment_arrays_on_device([a for a, _, _ in cases], [p for _, _, p in cases])
    for k, ((a, _, plan), g) in enumerate(zip(cases, got)):
        ref = np.asarray(_pillow_chain(_pil(a), plan))
        g = g.cpu().numpy()
        assert g.shape == ref.shape, (k, plan, g.shape, ref.shape)
        assert np.array_equal(g, ref), (k, plan, f"{int((g != ref).sum())} bytes differ")
    # grey images, device tensors as sources (read in place), one image alone
    rs = np.random.default_rng(6)
    for a, _, plan in cases[2:8]:
        grey = np.ascontiguousarray(a[:, :, :1])
        g = aug.augment_arrays_on_device([torch.from_numpy(grey).cuda()], [plan])[0].cpu().numpy()
        ref = np.asarray(_pillow_chain(_pil(grey), plan))[..., None]
        assert np.array_equal(g, ref), (plan, f"{int((g != ref).sum())} bytes differ")


@pytest.mark.parametrize("grey", [True, False])
def test_prepare_batches_equals_the_host_path(grey):
    cfg = NetConfig() if grey else NetConfig(grey=False)
    cases = _cases()
    images = [_pil(a) if k % 3 == 0 else (torch.from_numpy(a).cuda() if k % 3 == 1 else a) for k, (a, _, _) in enumerate(cases)]
    markups = [mk for _, mk, _ in cases]
    before = [[list(np.asarray(m.bbox).tolist()) for m in mk] for mk in markups]
    groups = SegmapManager.prepare_batches_on_device(images, markups, cfg, augment=True, plans=[p for _, _, p in cases])
    assert [[list(np.asarray(m.bbox).tolist()) for m in mk] for mk in markups] == before          # the caller's markup is untouched
    assert sorted(i for idx, *_ in groups for i in idx) == list(range(len(cases)))
    assert len(groups) > 1                                                                      # augmented sizes differ
    n_objects = 0
    for idx, x, labels, rescaled, plans in groups:
        assert x.dtype == torch.uint8 and labels.dtype == torch.int32 and x.shape[0] == labels.shape[0] == len(idx) == len(rescaled) == len(plans)
        xs, ls = x.cpu().numpy(), labels.cpu().numpy()
        for j, i in enumerate(idx):
            a, mk, plan = cases[i]
            assert plans[j] is plan
            ref_x, ref_l, ref_mk = _host_path(_pil(a), mk, plan, cfg)
            assert xs[j].shape == ref_x.shape and ls[j].shape == ref_l.shape, (i, xs[j].shape, ref_x.shape)
            assert np.array_equal(xs[j], ref_x), (i, plan, f"{int((xs[j] != ref_x).sum())} image bytes differ")
            assert np.array_equal(ls[j], ref_l), (i, plan, f"{int((ls[j] != ref_l).sum())} label pixels differ")
            assert len(rescaled[j] or []) == len(ref_mk or [])
            for m, r in zip(rescaled[j] or [], ref_mk or []):
                assert type(m) is type(r) and getattr(m, "object_type", None) == getattr(r, "object_type", None)
                assert np.array_equal(np.asarray(m.bbox), np.asarray(r.bbox))
                n_objects += 1
    assert n_objects > 40
    # augment=False: empty plans, the plain preparation grouped by size
    same = [c for c in cases if c[0].shape[:2] == cases[0][0].shape[:2]] + [cases[0]]
    groups = SegmapManager.prepare_batches_on_device([a for a, _, _ in same], [mk for _, mk, _ in same], cfg, augment=False)
    x0, l0, _ = SegmapManager.prepare_batch_on_device([a for a, _, _ in same], [mk for _, mk, _ in same], cfg)
    assert len(groups) == 1 and torch.equal(groups[0][1], x0) and torch.equal(groups[0][2], l0)
    assert all(p.stages == () for p in groups[0][4])


def test_single_image_entry_points_follow_their_plan():
    rs = np.random.default_rng(9)
    cfg = NetConfig(grey=False)
    done = 0
    for seed in range(14):
        h, w = int(rs.integers(200, 600)), int(rs.integers(200, 600))
        mode = "L" if seed % 4 == 3 else "RGB"
        a = rs.integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)
        im = Image.fromarray(a, mode)
        mk = [ObjectMarkup(q.reshape(-1).tolist()) for q in synthetic.random_quads(rs, h, w, 1, 4, 12, 50)]
        boxes = [list(m.bbox) for m in mk]

        def reseed():
            random.seed(seed)
            np.random.seed(seed)
        reseed()
        plan = aug.sample_plan(im.size, mk)
        reseed()
        sa = SegLinksImageAugmentation(im, mk, cfg)
        assert sa.plan == plan
        ref = _pillow_chain(im, plan)
        got = sa.get_modified_image()
        assert got.mode == mode and got.size == ref.size and np.array_equal(np.asarray(got), np.asarray(ref)), (seed, plan)
        for m, r in zip(sa.get_modified_markup(), aug.apply_plan_to_markup(plan, mk)):
            assert type(m) is type(r) and np.array_equal(np.asarray(m.bbox), np.asarray(r.bbox))
        reseed()
        image, markup, seg = SegmapManager.prepare_image_and_target(im, mk, cfg, augment=True)
        im3, mk3 = SegmapManager._rescale_image_and_markup(ref, aug.apply_plan_to_markup(plan, mk), cfg)
        assert image.size == im3.size and np.array_equal(np.asarray(image), np.asarray(im3)), (seed, plan)
        assert np.array_equal(np.asarray(seg), np.asarray(SegmapManager.build_segmentation_map(im3, mk3, scale=cfg.get_scale())))
        for m, r in zip(markup, mk3):
            assert np.array_equal(np.asarray(m.bbox), np.asarray(r.bbox))
        assert [list(m.bbox) for m in mk] == boxes                                               # not mutated
        done += bool(plan.stages)
    assert done >= 8
    # empty markup: nothing drawn, the image itself comes back
    state = random.getstate()
    im = Image.new("RGB", (100, 80))
    sa = SegLinksImageAugmentation(im, [], cfg)
    assert sa.get_modified_image() is im and sa.get_modified_markup() == [] and random.getstate() == state
    with pytest.raises(ValueError, match="mode"):
        SegLinksImageAugmentation(Image.new("RGBA", (10, 10)), [ObjectMarkup([1, 1, 5, 1, 5, 5, 1, 5])], cfg)


def test_train_steps_on_an_augmented_batch():
    cfg = NetConfig()
    rs = np.random.default_rng(21)
    random.seed(3)
    np.random.seed(3)
    frames = [rs.integers(0, 256, (360, 640, 3), dtype=np.uint8) for _ in range(8)]
    markups = [[ObjectMarkup(q.reshape(-1).tolist()) for q in synthetic.random_quads(rs, 360, 640, 2, 5, 12, 50)] for _ in frames]
    groups = SegmapManager.prepare_batches_on_device(frames, markups, cfg, augment=True)
    idx, x, labels, _, plans = max(groups, key=lambda g: len(g[0]))
    assert any(p.stages for g in groups for p in g[4])
    model = Model(cfg, seed=0)
    trainer = Trainer(model)
    for _ in range(2):
        loss = trainer.train_step_on_device(x, labels)
    torch.cuda.synchronize()
    assert np.isfinite(loss.cpu().numpy()).all(), loss
