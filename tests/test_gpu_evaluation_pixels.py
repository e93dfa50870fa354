"""GPU: ubd_evaluate_pixels (argmax, correctness mask, pixel counts, per-object accuracies over filled external components,
device sums) against the CPU oracle of tests/pixel_eval_oracle.py (border following + contour fill of oracle.cv_post).

Bounds.  n_correct, n_total, n_objects and the mask are integers: compared exactly.  object_acc_sum of an image: within
n_objects * 2^-52 of the exact rational sum -- one correctly rounded fp64 division per object (<= 2^-54 each, the quotients
are <= 1) plus one rounding of a sum <= n_objects (the device keeps the ordered sum as an unevaluated pair of doubles).
The accumulator adds the images' records one by one in plain fp64: on top of the records' own bounds every addition rounds a
partial sum <= the total object count, i.e. <= total * 2^-53 per image added.  No case of the set is excluded.
"""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import pixel_eval_oracle as po  # noqa: E402
from ubdvss_amd import NetConfig, Model, ModelRunner, ClassifiedObjectMarkup, ObjectMarkup, SegmapManager, _lib  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402

pytestmark = pytest.mark.gpu


def _acc():
    return torch.zeros(ev.pixel_accumulator_bytes(), dtype=torch.uint8, device="cuda")


def _run(z, labels, n_classes, acc=None, want_mask=True, full=True):
    """z: numpy (n, h, w, 1 + C).  full: pass the net-shaped tensor (strided view), else a contiguous class slice"""
    acc = _acc() if acc is None else acc
    zt = torch.from_numpy(z).cuda()
    if not full:
        zt = zt[..., 1:].contiguous()
    rec, mask = ev.evaluate_pixels(zt, torch.from_numpy(labels).cuda(), acc, want_mask=want_mask, n_classes=n_classes)
    torch.cuda.synchronize()
    return ev.pixel_records_to_numpy(rec), (mask.cpu().numpy() if mask is not None else None), acc


def _check_against_oracle(z, labels, n_classes, recs, mask, where=""):
    want = po.batch_stats(z[..., 1:], labels)
    for i, s in enumerate(want):
        r = recs[i]
        got = (int(r["n_correct"]), int(r["n_total"]), int(r["n_objects"]))
        exact = po.exact_acc_sum(s["objects"])
        err = abs(Fraction(float(r["object_acc_sum"])) - exact)
        print(f"{where} image {i}: device {got} acc_sum {float(r['object_acc_sum'])!r}; oracle "
              f"({s['n_correct']}, {s['n_total']}, {len(s['objects'])}) acc_sum {float(exact)!r}; error {float(err):.3e} "
              f"bound {len(s['objects']) * 2.0 ** -52:.3e}")
        assert got == (s["n_correct"], s["n_total"], len(s["objects"])), (where, i)
        assert err <= Fraction(len(s["objects"]), 2 ** 52), (where, i, float(err))
        if mask is not None:
            assert np.array_equal(mask[i], s["mask"]), (where, i, int((mask[i] != s["mask"]).sum()))
    return want


@pytest.mark.parametrize("seed,n,h,w,C", po.seeded_cases())
def test_seeded_batches_against_the_oracle(seed, n, h, w, C):
    labels, z = po.random_batch(seed, n, h, w, C)
    recs, mask, _ = _run(z, labels, C)
    _check_against_oracle(z, labels, C, recs, mask, f"seed {seed} {h}x{w} C={C}")


@pytest.mark.parametrize("name", sorted(po.quirk_maps()))
def test_quirk_maps(name):
    labels, pred, want = po.quirk_maps()[name]
    z = po.logits_from_pred(pred)[None]
    recs, mask, _ = _run(z, labels[None], 3)
    r = recs[0]
    assert (int(r["n_correct"]), int(r["n_total"]), int(r["n_objects"])) == (want["n_correct"], want["n_total"], len(want["objects"]))
    assert abs(Fraction(float(r["object_acc_sum"])) - po.exact_acc_sum(want["objects"])) <= Fraction(len(want["objects"]), 2 ** 52)
    _check_against_oracle(z, labels[None], 3, recs, mask, name)


def test_argmax_ties_nan_and_labels_outside_the_classes():
    # one row of single-pixel objects two apart: (logits of the 3 classes, label, correct?)
    rows = [([1.0, 1.0, 0.0], 1, True),        # tie: the lowest index wins -> class 0
            ([1.0, 1.0, 0.0], 2, False),
            ([0.0, 2.0, 2.0], 3, False),       # the second of two equal maxima never wins
            ([0.0, 2.0, 2.0], 2, True),
            ([0.0, np.nan, 5.0], 2, True),     # a NaN counts as the maximum
            ([0.0, np.nan, np.nan], 3, False),  # the first NaN wins
            ([np.nan, 9.0, 9.0], 1, True),
            ([3.0, 1.0, 1.0], 4, False),       # a label above C is never correct
            ([3.0, 1.0, 1.0], 40, False),
            ([-np.inf, -np.inf, -np.inf], 1, True)]
    w = 2 * len(rows) + 1
    labels = np.zeros((1, 3, w), np.int32)
    z = np.zeros((1, 3, w, 4), np.float32)
    z[..., 0] = 7.0
    z[..., 2] = 1.0                            # background predicts class 1
    for k, (lg, t, _) in enumerate(rows):
        labels[0, 1, 2 * k + 1] = t
        z[0, 1, 2 * k + 1, 1:] = lg
    labels[0, 0, 0] = -3                       # negative labels are background
    labels[0, 2, w - 1] = -(2 ** 31)
    recs, mask, _ = _run(z, labels, 3)
    assert [int(v) for v in mask[0, 1, 1::2]] == [1 if ok else -1 for _, _, ok in rows]
    assert mask[0, 0, 0] == 0 and mask[0, 2, w - 1] == 0
    n_ok = sum(ok for _, _, ok in rows)
    assert (int(recs[0]["n_correct"]), int(recs[0]["n_total"]), int(recs[0]["n_objects"])) == (n_ok, len(rows), len(rows))
    assert float(recs[0]["object_acc_sum"]) == float(n_ok)
    _check_against_oracle(z, labels, 3, recs, mask, "argmax rules")


def test_input_forms_give_identical_records():
    labels, z = po.random_batch(77, 3, 50, 70, 3)
    recs_full, mask_full, acc_full = _run(z, labels, 3, full=True)
    recs_slice, mask_slice, acc_slice = _run(z, labels, 3, full=False)
    assert recs_full.tobytes() == recs_slice.tobytes() and np.array_equal(mask_full, mask_slice)
    assert acc_full.cpu().numpy().tobytes() == acc_slice.cpu().numpy().tobytes()
    # the full tensor is passed as it lies: no copy is made of a regular pixel grid
    zt = torch.from_numpy(z).cuda()
    assert ev._pixel_stride(zt[..., 1:]) == 4 and ev._pixel_stride(zt[..., 1:].contiguous()) == 3
    # labels as (N, h, w, 1) numpy; a class slice without n_classes; no mask, no records
    acc = _acc()
    rec, mask = ev.evaluate_pixels(zt[..., 1:], labels[..., None], acc, want_mask=False, per_image=False)
    torch.cuda.synchronize()
    assert rec is None and mask is None
    assert acc.cpu().numpy().tobytes() == acc_full.cpu().numpy().tobytes()
    # a wide pixel stride (direct reads) and 31 classes at stride 32 (half-wave rounds) agree with the contiguous slices
    for C, pad in ((3, 37), (31, 0)):
        labels, z = po.random_batch(78 + C, 2, 37, 41, C)
        wide = np.zeros(z.shape[:3] + (1 + C + pad,), np.float32)
        wide[..., :1 + C] = z
        wt = torch.from_numpy(wide).cuda()
        a1, a2 = _acc(), _acc()
        r1, m1 = ev.evaluate_pixels(wt[..., 1:1 + C], torch.from_numpy(labels).cuda(), a1, want_mask=True)
        r2, m2 = ev.evaluate_pixels(torch.from_numpy(z).cuda()[..., 1:].contiguous(), torch.from_numpy(labels).cuda(), a2, want_mask=True)
        torch.cuda.synchronize()
        assert ev._pixel_stride(wt[..., 1:1 + C]) == 1 + C + pad
        assert torch.equal(r1, r2) and torch.equal(m1, m2) and torch.equal(a1, a2)
        _check_against_oracle(z, labels, C, ev.pixel_records_to_numpy(r1), m1.cpu().numpy(), f"stride {1 + C + pad}")


def _acc_bound(stats_per_image):
    total = sum(len(s["objects"]) for s in stats_per_image)
    return Fraction(total, 2 ** 52) + len(stats_per_image) * Fraction(total, 2 ** 53)


def test_accumulator_adds_repeats_and_takes_seventy_images():
    labels, z = po.random_batch(91, 70, 24, 40, 3)
    want = po.batch_stats(z[..., 1:], labels)
    recs, _, acc = _run(z, labels, 3, want_mask=False)                      # n = 70 in one call
    _check_against_oracle(z, labels, 3, recs, None, "70 images")
    a = ev.unpack_pixel_accumulator(acc.cpu().numpy())
    assert (a["n_correct"], a["n_total"], a["n_objects"], a["images"]) == (
        sum(s["n_correct"] for s in want), sum(s["n_total"] for s in want), sum(len(s["objects"]) for s in want), 70)
    exact = sum((po.exact_acc_sum(s["objects"]) for s in want), Fraction(0))
    assert abs(Fraction(a["object_acc_sum"]) - exact) <= _acc_bound(want)
    # the accumulator is the ordered plain sum of the records
    s = 0.0
    for r in recs:
        s += float(r["object_acc_sum"])
    assert a["object_acc_sum"] == s
    # two calls add: the same images in two calls give the same bits as in one
    acc2 = _acc()
    _run(z[:33], labels[:33], 3, acc=acc2, want_mask=False)
    _run(z[33:], labels[33:], 3, acc=acc2, want_mask=False)
    assert acc2.cpu().numpy().tobytes() == acc.cpu().numpy().tobytes()
    # repeated calls give bit-equal accumulators
    for _ in range(3):
        _, _, again = _run(z, labels, 3, want_mask=False)
        assert again.cpu().numpy().tobytes() == acc.cpu().numpy().tobytes()


def test_lds_and_global_forms_agree():
    labels, z = po.random_batch(92, 3, 128, 128, 3)
    recs_a, mask_a, acc_a = _run(z, labels, 3)
    lp = np.zeros((3, 128, 129), np.int32)                                   # one empty column: 16512 pixels, the global-memory form
    lp[:, :, :128] = labels
    zp = np.zeros((3, 128, 129, 4), np.float32)
    zp[:, :, :128] = z
    recs_b, mask_b, acc_b = _run(zp, lp, 3)
    assert recs_a.tobytes() == recs_b.tobytes()
    assert acc_a.cpu().numpy().tobytes() == acc_b.cpu().numpy().tobytes()
    assert np.array_equal(mask_a, mask_b[:, :, :128]) and not mask_b[:, :, 128].any()
    # a tall one-pixel-wide map and a wide one-pixel-high map above the LDS limit
    for shape in ((1, 20000), (20000, 1)):
        labels, z = po.random_batch(93, 1, shape[0], shape[1], 2)
        recs, mask, _ = _run(z, labels, 2)
        _check_against_oracle(z, labels, 2, recs, mask, f"{shape}")


class _Raw:
    """the C entry point with every argument under the test's control"""

    def __init__(self, n, h, w, C):
        self.lib = _lib.load()
        self.n, self.h, self.w, self.C = n, h, w, C
        labels, z = po.random_batch(5, n, h, w, C)
        self.labels_h, self.z_h = labels, z
        self.z = torch.from_numpy(z).cuda()
        self.labels = torch.from_numpy(labels).cuda()
        self.need = int(self.lib.ubd_evaluate_pixels_workspace_bytes(n, h, w))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")
        self.acc = _acc()
        self.mask = torch.empty((n, h, w), dtype=torch.int8, device="cuda")
        self.rec = torch.empty((n, 32), dtype=torch.uint8, device="cuda")

    def __call__(self, **kw):
        a = dict(logits=self.z.data_ptr() + 4, stride=self.C + 1, C=self.C, labels=self.labels.data_ptr(), n=self.n, h=self.h, w=self.w,
                 mask=self.mask.data_ptr(), rec=self.rec.data_ptr(), acc=self.acc.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.need)
        a.update(kw)
        return self.lib.ubd_evaluate_pixels(a["logits"], a["stride"], a["C"], a["labels"], a["n"], a["h"], a["w"], a["mask"], a["rec"],
                                            a["acc"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)


def test_null_mask_and_null_records_forms():
    raw = _Raw(3, 50, 70, 3)
    assert raw() == 0, raw.lib.ubd_last_error()
    torch.cuda.synchronize()
    full = raw.acc.cpu().numpy().tobytes()
    _check_against_oracle(raw.z_h, raw.labels_h, 3, ev.pixel_records_to_numpy(raw.rec), raw.mask.cpu().numpy(), "raw")
    for kw in (dict(mask=None), dict(rec=None), dict(mask=None, rec=None)):
        raw.acc.zero_()
        assert raw(**kw) == 0, raw.lib.ubd_last_error()
        torch.cuda.synchronize()
        assert raw.acc.cpu().numpy().tobytes() == full


def test_capture_in_a_hip_graph():
    for h, w in ((64, 96), (136, 200)):                                      # the LDS form and the global-memory form
        raw = _Raw(4, h, w, 3)
        assert raw() == 0 and raw() == 0, raw.lib.ubd_last_error()
        torch.cuda.synchronize()
        raw.acc.zero_()
        assert raw() == 0
        torch.cuda.synchronize()
        direct, direct_mask, direct_rec = raw.acc.cpu().numpy().tobytes(), raw.mask.clone(), raw.rec.clone()
        raw.mask.zero_(); raw.rec.zero_(); raw.acc.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert raw() == 0, raw.lib.ubd_last_error()
        raw.acc.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert raw.acc.cpu().numpy().tobytes() == direct
        assert torch.equal(raw.mask, direct_mask) and torch.equal(raw.rec, direct_rec)
        g.replay()                                                           # sums keep adding
        torch.cuda.synchronize()
        a, b = ev.unpack_pixel_accumulator(np.frombuffer(direct, np.uint8)), ev.unpack_pixel_accumulator(raw.acc.cpu().numpy())
        assert b["images"] == 8 and b["n_correct"] == 2 * a["n_correct"] and b["n_objects"] == 2 * a["n_objects"]


def test_every_error_path_launches_nothing():
    raw = _Raw(2, 12, 20, 3)
    lib = raw.lib
    raw.acc.fill_(0x5A)
    bad = [(dict(C=0), b"n_classes"), (dict(C=32), b"n_classes"), (dict(stride=2), b"pixel_stride"), (dict(n=0), b"n must be"),
           (dict(h=0), b"bad sizes"), (dict(w=-4), b"bad sizes"), (dict(h=32768), b"too large"), (dict(w=40000), b"too large"),
           (dict(logits=None), b"null"), (dict(labels=None), b"null"), (dict(acc=None), b"accumulator"), (dict(ws=None), b"workspace"),
           (dict(ws_bytes=raw.need - 1), b"too small")]
    for kw, msg in bad:
        assert raw(**kw) != 0, kw
        assert msg in lib.ubd_last_error(), (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    assert (raw.acc.cpu().numpy() == 0x5A).all()                             # untouched
    assert lib.ubd_evaluate_pixels_workspace_bytes(0, 8, 8) == 0
    assert lib.ubd_evaluate_pixels_workspace_bytes(1, 0, 8) == 0
    assert lib.ubd_evaluate_pixels_workspace_bytes(1, 8, 32768) == 0
    assert lib.ubd_evaluate_pixels_workspace_bytes(1, 3, 5) > 0               # no multiple-of-4 requirement
    assert lib.ubd_evaluate_pixels_accumulator_bytes() >= 40
    # the wrapper's own checks
    z = torch.zeros((1, 4, 4, 4), device="cuda")
    lab = torch.zeros((1, 4, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="channels"):
        ev.evaluate_pixels(z, lab, _acc(), n_classes=5)
    with pytest.raises(ValueError, match="do not match"):
        ev.evaluate_pixels(z, lab[:, :3], _acc(), n_classes=3)
    with pytest.raises(ValueError, match="outside the limits"):
        ev.evaluate_pixels(torch.zeros((1, 4, 4, 40), device="cuda"), lab, _acc())


def test_end_to_end_through_the_model_runner():
    rng = np.random.default_rng(3)
    cfg = NetConfig(class_names=["a", "b", "c"], grey=False)
    images = [rng.integers(0, 256, (300, 600, 3), dtype=np.uint8) for _ in range(4)]
    markups = []
    for k in range(4):
        objs = []
        for j in range(3):
            x0, y0 = 40 + 180 * j, 30 + 20 * k
            objs.append(ClassifiedObjectMarkup([x0, y0, x0 + 120, y0, x0 + 120, y0 + 90 + 30 * j, x0, y0 + 90 + 30 * j], (j + k) % 3))
        markups.append(objs)
    x, labels, rescaled = SegmapManager.prepare_batch_on_device(images, markups, cfg)
    assert labels.dtype == torch.int32 and int(labels.max()) == 3
    model = Model(cfg, seed=0)
    runner = ModelRunner(cfg)
    with4 = runner.evaluate_batches(model, [(x[:2], rescaled[:2], None, labels[:2]), (x[2:], rescaled[2:], None, labels[2:].cpu().numpy()[..., None])])
    with3 = ModelRunner(cfg).evaluate_batches(model, [(x[:2], rescaled[:2], None), (x[2:], rescaled[2:], None)])
    new = {"classification_pixel_acc_total", "classification_pixel_acc_object"}
    assert set(with4) - set(with3) == new and set(with3) - set(with4) == set()
    for k in with3:
        assert with4[k] == with3[k] or (with4[k] != with4[k] and with3[k] != with3[k]), k
    xh = x.cpu().numpy()
    logits = np.concatenate([model.predict(xh[:2]), model.predict(xh[2:])])          # the batches the runner saw
    want = po.batch_stats(logits[..., 1:], labels.cpu().numpy())
    n_ok, n_fg = sum(s["n_correct"] for s in want), sum(s["n_total"] for s in want)
    objs = [o for s in want for o in s["objects"]]
    assert n_fg > 0 and len(objs) == 12
    assert with4["classification_pixel_acc_total"] == n_ok / n_fg
    exact = po.exact_acc_sum(objs) / len(objs)
    assert abs(Fraction(with4["classification_pixel_acc_object"]) - exact) <= Fraction(1, 2 ** 50)   # sum within 12 * 2^-52 + 4 * 12 * 2^-53, one division
    # evaluate_batch itself returns the mask; without label maps it returns None as before
    calc = ev.DatasetMetricCalculator(cfg)
    lg, _, quads, classes, counts = runner.predict_on_device(model, x)
    rec, mask = calc.evaluate_batch(rescaled, (quads, classes, counts), gt_segmap=labels, classification_logits=lg)
    torch.cuda.synchronize()
    assert mask.dtype == torch.int8 and tuple(mask.shape) == tuple(labels.shape)
    assert np.array_equal(mask.cpu().numpy(), np.stack([s["mask"] for s in po.batch_stats(lg.cpu().numpy()[..., 1:], labels.cpu().numpy())]))
    assert calc.evaluate_batch(rescaled, (quads, classes, counts))[1] is None
    # a detection-only config with 4-tuples adds no key
    det = NetConfig(grey=False)
    dmodel = Model(det, seed=0)
    dgt = [[ObjectMarkup(m.bbox) for m in objs_] for objs_ in rescaled]
    d4 = ModelRunner(det).evaluate_batches(dmodel, [(x, dgt, None, labels)])
    d3 = ModelRunner(det).evaluate_batches(dmodel, [(x, dgt, None)])
    assert d4 == d3 and not (new & set(d4))
