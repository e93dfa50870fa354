"""GPU: multi-scale inference (ubd_multiscale_gather / ubd_multiscale_fuse / ubd_forward_multiscale, MultiscaleModel) against
tests/multiscale_oracle.py.  The pyramid and the mean are held bit for bit (the gather copies, the mean's arithmetic is fixed:
fp32 adds in level order, one IEEE division); the whole chain is held bit for bit to the fp32 mean of the base model's own outputs
on the sliced inputs, and to the fp64 oracle -- whose pyramid is the GENERAL bilinear resize -- within the forward pass's bound."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import multiscale_oracle as mo  # noqa: E402
from oracle import net_numpy as onet  # noqa: E402
from ubdvss_amd import NetConfig, Model, ModelRunner, MultiscaleModel, NetManager, PreprocessingType, SegmapManager, _lib, synthetic  # noqa: E402
from ubdvss_amd.data_markup import ObjectMarkup  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 64          # bytes on either side of a buffer under test (keeps the 16-byte alignment)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------- 1. gather
# the last two: the one scale power the others are too small for, and uint8 rows whose width is 8 mod 16 (8-byte pieces)
@pytest.mark.parametrize("n,hh,ww", [(2, 32, 32), (3, 64, 160), (1, 96, 32), (1, 64, 128), (2, 16, 40)])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("c", [1, 3])
def test_gather_is_the_numpy_slice(n, hh, ww, u8, c):
    lib = _lib.load()
    rng = np.random.default_rng(n * 1000 + hh + ww + c)
    if u8:
        x = rng.integers(0, 256, (n, hh, ww, c), dtype=np.uint8)
    else:
        x = rng.standard_normal((n, hh, ww, c)).astype(np.float32)
        x.reshape(-1)[::97] = np.nan                                     # a copy keeps every bit pattern
    xt = torch.from_numpy(x).cuda()
    done = []
    for power in (1, 3, 4):
        if hh % (4 << power) or ww % (4 << power):
            continue
        pixel = c * x.itemsize
        nbytes = lib.ubd_multiscale_levels_bytes(n, hh, ww, pixel, 1, power)
        assert nbytes == sum(n * (hh >> s) * (ww >> s) * pixel for s in range(1, power + 1))
        buf = torch.full((nbytes + 2 * CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        rc = lib.ubd_multiscale_gather(xt.data_ptr(), _lib.UBD_IN_U8 if u8 else _lib.UBD_IN_F32, n, hh, ww, c, power,
                                       buf.data_ptr() + CANARY, nbytes, _stream())
        assert rc == 0, lib.ubd_last_error()
        got = buf.cpu().numpy()
        assert (got[:CANARY] == 0xA5).all() and (got[CANARY + nbytes:] == 0xA5).all(), "wrote outside the packed levels"
        off = CANARY
        for s in range(1, power + 1):
            want = mo.decimate(x, s)
            assert off - CANARY == lib.ubd_multiscale_levels_bytes(n, hh, ww, pixel, 1, s - 1)
            lv = got[off:off + want.nbytes]
            assert np.array_equal(lv, want.reshape(-1).view(np.uint8)), (power, s)
            off += want.nbytes
        assert off == CANARY + nbytes
        done.append(power)
    assert done, "no scale power fits this shape"
    assert done == {(32, 32): [1, 3], (64, 160): [1, 3], (96, 32): [1, 3], (64, 128): [1, 3, 4], (16, 40): [1]}[(hh, ww)]


def test_gather_refusals():
    lib = _lib.load()
    x = torch.zeros((1, 48, 32, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    g = lambda *a: lib.ubd_multiscale_gather(*a, _stream())             # noqa: E731
    assert g(x.data_ptr(), _lib.UBD_IN_U8, 1, 48, 32, 3, 3, out.data_ptr(), 4096) != 0 and b"multiples of 32" in lib.ubd_last_error()
    assert g(x.data_ptr(), _lib.UBD_IN_U8, 1, 48, 32, 3, 5, out.data_ptr(), 4096) != 0 and b"outside 0..4" in lib.ubd_last_error()
    assert g(x.data_ptr(), _lib.UBD_IN_U8, 1, 48, 32, 2, 1, out.data_ptr(), 4096) != 0 and b"channels" in lib.ubd_last_error()
    assert g(x.data_ptr(), _lib.UBD_IN_U8, 1, 48, 32, 3, 1, out.data_ptr(), 100) != 0 and b"too small" in lib.ubd_last_error()
    assert g(x.data_ptr() + 4, _lib.UBD_IN_U8, 1, 16, 16, 3, 1, out.data_ptr(), 4096) != 0 and b"aligned" in lib.ubd_last_error()
    assert lib.ubd_multiscale_levels_bytes(1, 48, 32, 3, 1, 5) == 0 and lib.ubd_multiscale_levels_bytes(1, 44, 32, 3, 1, 3) == 0


# ---------------------------------------------------------------------------------------------- 2. fuse
@pytest.mark.parametrize("mh,mw", [(8, 8), (16, 24), (32, 48)])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("power", [1, 2, 3])
def test_fuse_is_the_fp32_oracle_bit_for_bit(mh, mw, k, power):
    lib = _lib.load()
    n = 2
    rng = np.random.default_rng(mh * 100 + k * 10 + power)
    levels = [(rng.standard_normal((n, mh >> s, mw >> s, k)) * 10 ** rng.uniform(-3, 3)).astype(np.float32) for s in range(power + 1)]
    want = mo.fuse_mean_f32(levels)
    packed = np.concatenate([l.reshape(-1) for l in levels])
    assert packed.nbytes == lib.ubd_multiscale_levels_bytes(n, mh, mw, 4 * k, 0, power)
    pt = torch.from_numpy(packed).cuda()
    out = torch.full((want.size + 2 * CANARY // 4,), 7.0, dtype=torch.float32, device="cuda")
    rc = lib.ubd_multiscale_fuse(pt.data_ptr(), n, mh, mw, k, power, out.data_ptr() + CANARY, _stream())
    assert rc == 0, lib.ubd_last_error()
    got = out.cpu().numpy()
    assert (got[:CANARY // 4] == 7.0).all() and (got[CANARY // 4 + want.size:] == 7.0).all()
    assert np.array_equal(got[CANARY // 4:CANARY // 4 + want.size].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.array_equal(pt.cpu().numpy(), packed)                     # the inputs are only read
    # out = level 0 itself; and an output that is only 4-byte aligned (the narrow form) gives the same bits
    rc = lib.ubd_multiscale_fuse(pt.data_ptr(), n, mh, mw, k, power, pt.data_ptr(), _stream())
    assert rc == 0, lib.ubd_last_error()
    alias = pt.cpu().numpy()
    assert np.array_equal(alias[:want.size].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.array_equal(alias[want.size:], packed[want.size:])        # the coarser levels are untouched
    rc = lib.ubd_multiscale_fuse(torch.from_numpy(packed).cuda().data_ptr(), n, mh, mw, k, power, out.data_ptr() + 4, _stream())
    assert rc == 0, lib.ubd_last_error()
    assert np.array_equal(out.cpu().numpy()[1:1 + want.size].view(np.uint32), want.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("mh,mw,k,power", [(4, 6, 1, 1), (4, 6, 3, 1), (2, 2, 5, 1), (16, 32, 2, 4), (3, 5, 1, 0)])
def test_fuse_narrow_rows_and_the_outer_powers(mh, mw, k, power):
    """rows of 6 floats (8-byte accesses), of 10 floats, the largest scale power, and power 0 (the mean of one level: y / 1)"""
    lib = _lib.load()
    rng = np.random.default_rng(mw + k)
    levels = [rng.standard_normal((3, mh >> s, mw >> s, k)).astype(np.float32) for s in range(power + 1)]
    want = mo.fuse_mean_f32(levels)
    pt = torch.from_numpy(np.concatenate([l.reshape(-1) for l in levels])).cuda()
    out = torch.full((want.size + 32,), 7.0, dtype=torch.float32, device="cuda")
    assert lib.ubd_multiscale_fuse(pt.data_ptr(), 3, mh, mw, k, power, out.data_ptr() + 64, _stream()) == 0, lib.ubd_last_error()
    got = out.cpu().numpy()
    assert (got[:16] == 7.0).all() and (got[16 + want.size:] == 7.0).all()
    assert np.array_equal(got[16:16 + want.size].view(np.uint32), want.reshape(-1).view(np.uint32))


def test_fuse_refusals():
    lib = _lib.load()
    t = torch.zeros(4096, dtype=torch.float32, device="cuda")
    assert lib.ubd_multiscale_fuse(t.data_ptr(), 1, 12, 8, 1, 3, t.data_ptr(), _stream()) != 0 and b"multiples of 8" in lib.ubd_last_error()
    assert lib.ubd_multiscale_fuse(t.data_ptr(), 1, 8, 8, 1, 5, t.data_ptr(), _stream()) != 0 and b"outside 0..4" in lib.ubd_last_error()
    assert lib.ubd_multiscale_fuse(t.data_ptr(), 1, 8, 8, 33, 1, t.data_ptr(), _stream()) != 0 and b"k must be" in lib.ubd_last_error()


# ---------------------------------------------------------------------------------------------- 3-5. end to end
# (c_in, n_classes, fml, n, H, W, P): the smallest level keeps sides >= 16
CASES = [(3, 0, True, 2, 128, 192, 3), (1, 2, False, 1, 64, 96, 1), (3, 0, True, 1, 64, 64, 2)]


def _config(cin, ncls, fml, pre=PreprocessingType.NONE):
    return NetConfig(class_names=[f"c{i}" for i in range(ncls)] if ncls else None, grey=(cin == 1), fml_compatible=fml, preprocessing=pre)


def _inputs(case, u8):
    cin, ncls, fml, n, hh, ww, power = case
    rng = np.random.default_rng(hh + ww + power)
    if u8:
        return rng.integers(0, 256, (n, hh, ww, cin), dtype=np.uint8)
    return synthetic.noise_images(hh + power, n, hh, ww, cin).astype(np.float32)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("u8", [False, True])
def test_end_to_end_equals_the_fused_base_outputs(case, dtype, u8):
    cin, ncls, fml, n, hh, ww, power = case
    cfg = _config(cin, ncls, fml, PreprocessingType.MOBILENET_LIKE if u8 else PreprocessingType.NONE)
    base = Model(cfg, dtype=dtype)
    base.set_weights(onet.init_weights(40 + cin + ncls, cin, ncls, bias_scale=0.25))
    ms = MultiscaleModel(base, power)
    assert ms.params is base.params and ms.k_out == base.k_out == 1 + ncls and ms.device == base.device and ms.net_config is cfg
    x = torch.from_numpy(_inputs(case, u8)).cuda()
    got = ms.predict_on_device(x)
    levels = [base.predict_on_device(x[:, ::2 ** s, ::2 ** s].contiguous()).cpu().numpy() for s in range(power + 1)]
    want = mo.fuse_mean_f32(levels)
    assert tuple(got.shape) == want.shape == (n, hh // 4, ww // 4, 1 + ncls) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a second call (the packed fragments are reused) and a call into a given tensor give the same bits
    out = torch.empty_like(got)
    assert ms.predict_on_device(x, out=out) is out and torch.equal(out, got)
    # numpy in, numpy out
    assert np.array_equal(ms.predict(x.cpu().numpy()).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("case", CASES)
def test_end_to_end_against_the_fp64_oracle(case):
    cin, ncls, fml, n, hh, ww, power = case
    w = onet.init_weights(40 + cin + ncls, cin, ncls, bias_scale=0.25)
    base = Model(_config(cin, ncls, fml))
    base.set_weights(w)
    x = _inputs(case, False)
    ref, ref_levels = mo.forward_f64(x, w, power, fml)
    got = MultiscaleModel(base, power).predict(x).astype(np.float64)
    big = max(float(np.abs(l).max()) for l in ref_levels)
    tol = 2e-5 * big + 1e-6 + (power + 1) * 2.0 ** -23 * big
    err = float(np.abs(got - ref).max())
    print(f"{case}: max |device - fp64| = {err:.3e}, bound {tol:.3e}, largest |logit| {big:.3f}")
    assert err <= tol, (err, tol)
    assert err <= 1e-3, err
    assert np.abs(ref - ref_levels[0]).max() > 10 * tol and np.abs(got - ref_levels[0]).max() > 10 * tol     # the other scales do contribute


def test_uint8_end_to_end_against_the_fp64_oracle():
    case = CASES[0]
    cin, ncls, fml, n, hh, ww, power = case
    w = onet.init_weights(41, cin, ncls, bias_scale=0.25)
    base = Model(_config(cin, ncls, fml, PreprocessingType.MOBILENET_LIKE))
    base.set_weights(w)
    x8 = _inputs(case, True)
    ref, ref_levels = mo.forward_f64(x8, w, power, fml, preprocess=lambda a: (a - 127.5) / 127.5)
    got = MultiscaleModel(base, power).predict(x8).astype(np.float64)
    big = max(float(np.abs(l).max()) for l in ref_levels)
    tol = 2e-5 * big + 1e-6 + (power + 1) * 2.0 ** -23 * big
    err = float(np.abs(got - ref).max())
    assert err <= tol and err <= 1e-3, (err, tol)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_power_zero_is_the_single_scale_pass(dtype):
    cfg = _config(3, 2, True, PreprocessingType.MOBILENET_LIKE)
    base = Model(cfg, dtype=dtype, seed=3)
    ms = MultiscaleModel(base, 0)
    lib = _lib.load()
    for shape, dt in [((2, 72, 100, 3), torch.uint8), ((1, 64, 64, 3), torch.float32)]:     # sides that are only multiples of 4
        x = (torch.rand(shape, device="cuda") * 255).to(dt) if dt == torch.uint8 else torch.randn(shape, device="cuda")
        assert torch.equal(ms.predict_on_device(x), base.predict_on_device(x))
        n, hh, ww, _ = shape
        for code in (_lib.UBD_IN_U8, _lib.UBD_IN_F32):
            assert lib.ubd_forward_multiscale_workspace_bytes(base._h, code, n, hh, ww, 0) == lib.ubd_forward_workspace_bytes(base._h, n, hh, ww)


# ---------------------------------------------------------------------------------------------- 6. ModelRunner
def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("ncls", [0, 2])
def test_model_runner_takes_a_multiscale_model(ncls):
    cfg = _config(3, ncls, True, PreprocessingType.MOBILENET_LIKE)
    base = Model(cfg)
    base.set_weights(onet.init_weights(77, 3, ncls, bias_scale=0.25))
    ms = MultiscaleModel(base, 3)
    rng = np.random.default_rng(5)
    batches = [torch.from_numpy(rng.integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)).cuda() for _ in range(3)]
    plain, piped = ModelRunner(cfg), ModelRunner(cfg, pipelined=True, slots=3)
    thr, total = plain.logit_threshold, 0
    res_piped = [piped.predict_on_device(ms, x) for x in batches]       # batch k's postprocess rides behind batch k + 1's chain
    piped.synchronize()
    for x, rp in zip(batches, res_piped):
        logits = ms.predict_on_device(x)
        want = ms.postprocess_on_device(logits, thr, cfg.get_scale(), cfg.get_min_pixels_for_detection(), cap=256)
        r = plain.predict_on_device(ms, x)
        torch.cuda.synchronize()
        for res in (r, rp):
            assert torch.equal(res[0], logits)
            assert torch.equal(res[1], want[0]) and torch.equal(res[4], want[3])
            cnt = want[3].cpu().numpy()
            assert (cnt <= 256).all()
            for i, c in enumerate(cnt):
                assert torch.equal(res[2][i, :c], want[1][i, :c])
                assert ncls == 0 or torch.equal(res[3][i, :c], want[2][i, :c])
        total += int(want[3].sum())
    assert total > 0, "the comparison covers no object"
    # evaluation: the same metrics both ways
    gt = [[ObjectMarkup([8, 8, 72, 8, 72, 56, 8, 56])], [ObjectMarkup([40, 60, 100, 60, 100, 120, 40, 120])]]
    if ncls:
        from ubdvss_amd.data_markup import ClassifiedObjectMarkup
        gt = [[ClassifiedObjectMarkup(o.bbox, k % ncls) for o in objs] for k, objs in enumerate(gt)]
    m_plain = ModelRunner(cfg).evaluate_batches(ms, [(x, gt, None) for x in batches])
    m_piped = ModelRunner(cfg, pipelined=True).evaluate_batches(ms, [(x, gt, None) for x in batches])
    assert m_plain and set(m_plain) == set(m_piped)
    for key in m_plain:
        assert m_plain[key] == m_piped[key] or (m_plain[key] != m_plain[key] and m_piped[key] != m_piped[key]), key


def test_predict_images_with_a_multiscale_model():
    """two raw images of different sizes: resized on the device to sides that are multiples of NetConfig's side multiple (64, a
    multiple of 32), one multi-scale chain per size"""
    cfg = _config(1, 0, True, PreprocessingType.MOBILENET_LIKE)
    manager = NetManager(None, cfg)
    manager.build_multiscale_model(max_scale_power=3, seed=1)
    ms = manager.get_model()
    assert isinstance(ms, MultiscaleModel) and ms.max_scale_power == 3 and manager.get_keras_model() is ms
    ms.set_weights(onet.init_weights(9, 1, 0, bias_scale=0.25))
    rng = np.random.default_rng(8)
    images = [rng.integers(0, 256, (300, 420, 3), dtype=np.uint8), rng.integers(0, 256, (200, 150, 3), dtype=np.uint8)]
    runner = ModelRunner(cfg, max_objects_per_image=2048)
    found = runner.predict_images(ms, images)
    assert len(found) == 2
    for im, objs in zip(images, found):
        x, metas = SegmapManager.rescale_images_on_device([im], cfg)
        assert x.shape[1] % 32 == 0 and x.shape[2] % 32 == 0
        _, _, want = runner.predict(ms, x.cpu().numpy(), rescale=True, meta_infos=metas)
        assert [tuple(int(v) for v in o.bbox) for o in objs] == [tuple(int(v) for v in o.bbox) for o in want[0]]
    assert sum(len(o) for o in found) > 0


# ---------------------------------------------------------------------------------------------- 7. graph
def test_graphed_chain_replays_bit_identically():
    cfg = _config(3, 0, True, PreprocessingType.MOBILENET_LIKE)
    base = Model(cfg, seed=4)
    ms = MultiscaleModel(base, 3)
    gf = ms.graphed_forward(1, 128, 192, torch.uint8)
    assert ms.graphed_forward(1, 128, 192, torch.uint8) is gf
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randint(0, 256, (1, 128, 192, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(2)]
    replays = [gf(x).clone() for x in xs]
    eager = [ms.predict_on_device(x) for x in xs]
    assert not torch.equal(eager[0], eager[1])
    for r, e in zip(replays, eager):
        assert torch.equal(r, e)
    base.set_weights(onet.init_weights(3, 3, 0, bias_scale=0.25))      # new parameters: the graph re-packs and re-captures
    assert torch.equal(gf(xs[0]), ms.predict_on_device(xs[0])) and not torch.equal(gf(xs[0]), replays[0])


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_name_the_rule():
    cfg = _config(3, 0, True)
    base = Model(cfg, seed=0)
    lib = _lib.load()
    for bad in (-1, 5):
        with pytest.raises(ValueError, match=r"0\.\.4"):
            MultiscaleModel(base, bad)
    ms = MultiscaleModel(base, 3)
    with pytest.raises(ValueError, match="multiples of 32"):
        ms.predict_on_device(torch.zeros((1, 48, 64, 3), device="cuda"))             # 48: a multiple of 4 (and 16), not of 32
    with pytest.raises(ValueError, match="device"):
        ms.predict_on_device(torch.zeros((1, 64, 64, 3)))
    with pytest.raises(ValueError, match="3 channels"):
        ms.predict_on_device(torch.zeros((1, 64, 64, 1), device="cuda"))
    with pytest.raises(ValueError, match="dtype"):
        ms.predict_on_device(torch.zeros((1, 64, 64, 3), device="cuda", dtype=torch.float16))
    # the C entry point
    x = torch.zeros((1, 64, 64, 3), device="cuda")
    out = torch.full((1, 16, 16, 1), 3.0, device="cuda")
    need = lib.ubd_forward_multiscale_workspace_bytes(base._h, _lib.UBD_IN_F32, 1, 64, 64, 3)
    assert need > lib.ubd_forward_workspace_bytes(base._h, 1, 64, 64)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(hh, ww, power, nbytes):
        return lib.ubd_forward_multiscale(base._h, base.params.data_ptr(), x.data_ptr(), _lib.UBD_IN_F32, _lib.UBD_PRE_NONE, 1, hh, ww, power,
                                          out.data_ptr(), ws.data_ptr(), nbytes, _stream())
    assert call(64, 64, 3, need - 1) != 0 and b"workspace too small" in lib.ubd_last_error()
    assert call(48, 64, 3, need) != 0 and b"multiples of 32" in lib.ubd_last_error()
    assert call(64, 48, 2, need) == 0                                                 # 16 divides both: accepted
    assert call(64, 64, -1, need) != 0 and b"outside 0..4" in lib.ubd_last_error()
    assert call(64, 64, 5, need) != 0 and b"outside 0..4" in lib.ubd_last_error()
    assert lib.ubd_forward_multiscale_workspace_bytes(base._h, _lib.UBD_IN_F32, 1, 48, 64, 3) == 0
    assert lib.ubd_forward_multiscale_workspace_bytes(base._h, _lib.UBD_IN_F32, 1, 64, 64, 5) == 0
    out.fill_(3.0)
    assert call(64, 64, 3, need - 1) != 0
    torch.cuda.synchronize()
    assert (out == 3.0).all()                                                         # a refused call launches nothing
    assert call(64, 64, 3, need) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ms.predict_on_device(x))
