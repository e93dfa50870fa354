"""Phase-major activation layouts of the fp32 inference pass (wino6.hip, P_p): a3 and the outputs of L4 .. L8 are stored with each row's
pixels permuted phase by phase, and the Winograd layers of dilation 1 and 2 group their tiles by sub-grid phase.  Only which lane holds
a tile and where it is stored change, not the arithmetic: the logits are BIT-identical to UBD_WINO6_LAYOUT=natural (every activation
in the natural column order) for every stem variant, input form, batch, ragged width and head."""
import numpy as np
import pytest
import torch

from oracle import net_numpy as onet
from ubdvss_amd import NetConfig, Model, ModelRunner, synthetic

pytestmark = pytest.mark.gpu

# W4 = W / 4 odd: W4 mod 2d != 0 for every dilation d = 1, 2, 4, 8, 16
SHAPES = ((1, 64, 140), (1, 136, 516), (3, 72, 68), (32, 64, 132))


def _pair(monkeypatch, cin, ncls, w):
    """(phase-major model, natural-layout model) with the same weights; the layout switch is read when the handle is made"""
    cfg = NetConfig(class_names=[f"c{i}" for i in range(ncls)] if ncls else None, grey=(cin == 1))
    monkeypatch.setenv("UBD_WINO6_LAYOUT", "natural")
    nat = Model(cfg)
    nat.set_weights(w)
    monkeypatch.delenv("UBD_WINO6_LAYOUT")
    ph = Model(cfg)
    ph.set_weights(w)
    return ph, nat


def _unaligned(t, nbytes=4):
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    lead = ((-buf.data_ptr()) % 16 + nbytes) // t.element_size()
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes
    return v


def _inputs(seed, n, hh, ww, cin):
    x8 = synthetic.noise_images(seed, n, hh, ww, cin, as_float=False)
    xf = torch.from_numpy((x8.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)).cuda()
    return {"u8": torch.from_numpy(x8).cuda(), "f32": xf, "f32_off4": _unaligned(xf)}


@pytest.mark.parametrize("stem", ["default", "fused123", "cold123", "fused", "unfused"])
@pytest.mark.parametrize("cin,ncls", [(3, 0), (1, 2)])
def test_logits_bit_identical_to_natural_layout(monkeypatch, stem, cin, ncls):
    if stem == "default":
        monkeypatch.delenv("UBD_STEM", raising=False)
    else:
        monkeypatch.setenv("UBD_STEM", stem)
    w = onet.init_weights(70 + cin + ncls, cin, ncls, bias_scale=0.2)
    ph, nat = _pair(monkeypatch, cin, ncls, w)
    for k, (n, hh, ww) in enumerate(SHAPES):
        for name, x in _inputs(5 + k, n, hh, ww, cin).items():
            a = ph.predict_on_device(x).cpu().numpy()
            b = nat.predict_on_device(x).cpu().numpy()
            assert float(np.abs(b).max()) > 1e-5, (stem, n, hh, ww, name)
            assert np.array_equal(a, b), (stem, cin, ncls, n, hh, ww, name, float(np.abs(a - b).max()))


@pytest.mark.parametrize("ncls", [0, 1])
def test_pipelined_and_graphed_bit_identical_to_natural_layout(monkeypatch, ncls):
    """ubd_forward_postprocess (the postprocess of the previous batch inside the stem kernel) and a captured graph of the pass, at the
    headline shape and a ragged one"""
    monkeypatch.delenv("UBD_STEM", raising=False)
    w = onet.init_weights(90 + ncls, 3, ncls, bias_scale=0.2)
    ph, nat = _pair(monkeypatch, 3, ncls, w)
    cfg = ph.net_config
    for n, hh, ww in ((32, 512, 512), (32, 128, 516)):
        labs = synthetic.rectangle_maps(3, n, hh // 4, ww // 4)
        xs = [torch.from_numpy(synthetic.textured_images(4 + s, labs, 4, 3).astype(np.float32) / 127.5 - 1.0).cuda() for s in range(3)]
        outs = []
        for m in (ph, nat):
            runner = ModelRunner(cfg, max_objects_per_image=256, pipelined=True)
            got = []
            for x in xs:
                lg, bmap, quads, classes, counts = runner.predict_on_device(m, x)
                got.append(lg.cpu().numpy())
            runner.flush()
            got.append((bmap.cpu().numpy(), quads.cpu().numpy(), counts.cpu().numpy()))
            gf = m.graphed_forward(n, hh, ww)
            got.append(gf(xs[1]).cpu().numpy())
            outs.append(got)
        for a, b in zip(outs[0][:3] + [outs[0][4]], outs[1][:3] + [outs[1][4]]):
            assert np.array_equal(a, b), (n, hh, ww, float(np.abs(a - b).max()))
        (bm0, q0, c0), (bm1, q1, c1) = outs[0][3], outs[1][3]
        assert np.array_equal(bm0, bm1) and np.array_equal(c0, c1), (n, hh, ww)
        for i in range(n):                                   # quads past the count are not written
            assert np.array_equal(q0[i, :c0[i]], q1[i, :c1[i]]), (n, hh, ww, i)
