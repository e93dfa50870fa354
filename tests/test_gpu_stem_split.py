"""The one-kernel fp32 stem (stem123.h) computes the pointwise products of L2 and L3 as exact three-way bf16 split products
(split3.h): scaling, determinism, accuracy against the fp32-MFMA stem kernels, and the cold-tile / strip-walk identity."""
import numpy as np
import pytest

from oracle import net_numpy as onet
from ubdvss_amd import NetConfig, Model, synthetic

pytestmark = pytest.mark.gpu


def _model(cin, ncls, fml, w):
    cfg = NetConfig(class_names=[f"c{i}" for i in range(ncls)] if ncls else None, grey=(cin == 1), fml_compatible=fml)
    m = Model(cfg)
    m.set_weights(w)
    return m


@pytest.mark.parametrize("cin,stem", [(3, "fused123"), (1, "fused123"), (3, "cold123"), (1, "cold123")])
def test_whole_pass_is_homogeneous_and_deterministic(monkeypatch, cin, stem):
    """Every piece of the split scales exactly with a power of two: with all biases zero the whole fp32 forward pass satisfies
    f(2x) = 2 f(x) and f(x / 4) = f(x) / 4 bit for bit, and two launches on the same input give the same bits.  The fp32-MFMA stem
    has these properties too: this guards them, it does not tell the split from the fp32 products (the accuracy test below would
    catch a dropped or misindexed piece product)."""
    monkeypatch.setenv("UBD_STEM", stem)
    w = onet.init_weights(31 + cin, cin, 0)                                   # zero biases
    m = _model(cin, 0, True, w)
    x = synthetic.noise_images(5, 2, 96, 136, cin)
    y = m.predict(x)
    assert float(np.abs(y).max()) > 1e-5                              # not all zero (ReLU)
    assert np.array_equal(m.predict(x), y)
    assert np.array_equal(m.predict(2.0 * x), 2.0 * y)
    assert np.array_equal(m.predict(0.25 * x), 0.25 * y)


FACTOR = 2.0     # the split stem's max error against fp64 may exceed the fp32-MFMA stem's by at most this factor (+ 1e-7 max|y|)


@pytest.mark.parametrize("few_cus", [False, True])
def test_error_vs_oracle_no_worse_than_fp32_mfma_stem(monkeypatch, few_cus):
    """Against the fp64 oracle, the one-kernel stem with split products is as accurate as the three fp32-MFMA stem kernels
    ("unfused"): ragged sizes (multiples of 4 only), a strip walk on two CUs, RGB and grey."""
    if few_cus:
        monkeypatch.setenv("UBD_TEST_NUM_CUS", "2")
    cases = ((3, 0, 2, 128, 192), (1, 2, 1, 72, 100), (3, 1, 3, 64, 200), (1, 0, 2, 136, 72), (3, 0, 1, 512, 512))
    for cin, ncls, n, hh, ww in cases:
        w = onet.init_weights(500 + cin + ncls, cin, ncls, bias_scale=0.25)
        x = synthetic.noise_images(23, n, hh, ww, cin)
        ref = onet.forward(x.astype(np.float64), w, True)
        err = {}
        for stem in ("unfused", "fused123"):
            monkeypatch.setenv("UBD_STEM", stem)
            err[stem] = float(np.abs(_model(cin, ncls, True, w).predict(x).astype(np.float64) - ref).max())
        scale = float(np.abs(ref).max())
        assert err["fused123"] <= FACTOR * err["unfused"] + 1e-7 * scale, (cin, n, hh, ww, err)


def test_cold_tiles_match_strip_walk_at_512(monkeypatch):
    """One 512 x 512 image: the cold-started tiles and the strip walk run the same split products on the same values."""
    w = onet.init_weights(9, 3, 0, bias_scale=0.2)
    x = synthetic.noise_images(3, 1, 512, 512, 3)
    out = {}
    for stem in ("cold123", "fused123"):
        monkeypatch.setenv("UBD_STEM", stem)
        out[stem] = _model(3, 0, True, w).predict(x)
    assert np.array_equal(out["cold123"], out["fused123"])
