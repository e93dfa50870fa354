"""MI355X x 2: the entry points that used to launch without a device guard (losses, pixel evaluation, visualisations) on tensors of
cuda:1 while cuda:0 is current -- bit-equal to the same calls made with cuda:1 current (ubdvss_amd/_lib.py, launch)."""
import numpy as np
import pytest
import torch

from ubdvss_amd import evaluation, losses, visualizations

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: tensors on a device that is not the current one "
                                                                       "(the GPU box of the test run has one)")]


def _calls(dev):
    """the three calls on inputs that live on ``dev`` -> every tensor they produce"""
    rng = np.random.default_rng(5)
    logits = torch.from_numpy(rng.normal(0, 2.0, (2, 8, 8, 3)).astype(np.float32)).to(dev)       # 2 classes
    labels = torch.from_numpy(rng.integers(0, 3, (2, 8, 8)).astype(np.int32)).to(dev)
    images = torch.from_numpy(rng.integers(0, 256, (2, 16, 16, 3)).astype(np.uint8)).to(dev)
    gt_map = torch.from_numpy((rng.random((2, 4, 4)) < 0.4).astype(np.int32)).to(dev)
    loss, grad = losses.loss_and_grad(labels, logits)
    acc = torch.zeros(evaluation.pixel_accumulator_bytes(), dtype=torch.uint8, device=dev)
    rec, mask = evaluation.evaluate_pixels(logits, labels, acc, want_mask=True, n_classes=2)
    drawn = visualizations._draw(images, gt=gt_map)["gt"]
    out = dict(loss=loss, grad=grad, acc=acc, rec=rec, mask=mask, drawn=drawn)
    assert all(t.device == dev for t in out.values())
    torch.cuda.synchronize(dev)
    return out


def test_launches_on_another_device_than_the_current_one():
    dev = torch.device("cuda:1")
    with torch.cuda.device(0):
        got = _calls(dev)
        assert torch.cuda.current_device() == 0
    with torch.cuda.device(1):
        want = _calls(dev)
    assert float(want["loss"][0]) > 0 and int(want["drawn"].ne(0).sum()) > 0 and int(want["mask"].ne(0).sum()) > 0
    for key in want:
        assert torch.equal(got[key], want[key]), key
