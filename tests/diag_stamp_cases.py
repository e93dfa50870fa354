"""Not collected by pytest: the workloads of tests/test_gpu_diag_stamps.py, the smallest shapes that reach every stamped kernel
(ubdvss_amd/csrc/stamps.h).  Imported by the test, which runs them on the product library (outputs(), in the test process), and run as
a script in ONE child process on the diagnostic library (bash ubdvss_amd/csrc/build.sh diag, loaded through tools/_diag.py):

    python tests/diag_stamp_cases.py <product outputs .npz>

The child runs every case once with no stamp buffer set, then once per stamp family with that family's buffer set, on identical inputs,
and exits non-zero at the first failed check or HIP error (nothing is retried):
 (a) every output of a stamped run is bit-equal to the run without stamps (same binary, stamps only add stores);
 (b) every family wrote at least one slot group, and within a group the stamps do not decrease in the order the family's tool
     (tools/stamps_*.py) labels them;
 (c) wino6 and sepb16 with 64 words registered inside a larger poisoned allocation leave every word from 64 on untouched;
 (d) against the product outputs: postprocess results equal, fp32 logits within the forward gate of tests/test_gpu_forward.py
     (2e-5 max|product| + 1e-6); for 16-bit and gradient outputs the maximum difference is printed, not asserted."""
import contextlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)


@contextlib.contextmanager
def _env(values):              # the UBD_* switches are read once, when a handle is created
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try: yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def _forward(dtype, env):
    def make():
        from ubdvss_amd import NetConfig, Model, synthetic
        with _env(env): m = Model(NetConfig(grey=False), dtype=dtype, seed=1)
        x = torch.from_numpy(synthetic.noise_images(2, 2, 64, 64, 3)).cuda()
        return lambda: {"logits": m.predict_on_device(x).clone()}
    return make


def _layer(env, layer):       # one dilated layer alone, as tools/stamps_wino6.py launches it: wino / wino6 keep one group of slots per wave, so the
    def make():               # stamps of the six launches of a forward pass would mix in one buffer
        import ctypes
        from ubdvss_amd import NetConfig, Model, _lib
        with _env(env): m = Model(NetConfig(grey=False), seed=1)
        lib = _lib.load()
        a = torch.from_numpy(np.random.default_rng(7).random((2, 16, 16, 24), dtype=np.float32) - 0.3).cuda()
        b = torch.empty_like(a)
        ws = torch.empty(int(lib.ubd_forward_workspace_bytes(m._h, 1, 4, 4)), dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.ubd_pack_weights(m._h, m.params.data_ptr(), ws.data_ptr(), ws.numel(), stream), "ubd_pack_weights")
        def call():
            _lib.check(lib.ubd_dilated_layer(m._h, m.params.data_ptr(), layer, a.data_ptr(), b.data_ptr(), 2, 16, 16, ws.data_ptr(), stream), "ubd_dilated_layer")
            return {"out": b.clone()}
        return call
    return make


def _train(dtype):
    def make():
        from ubdvss_amd import NetConfig, Model, Trainer, Adam, synthetic
        tr = Trainer(Model(NetConfig(grey=False), dtype=dtype, seed=1), Adam())
        lab = synthetic.rectangle_maps(30, 2, 16, 16, side_min=3, side_max=10)
        x = torch.from_numpy(synthetic.textured_images(31, lab, 4, 3).astype(np.float32) / 127.5 - 1.0).cuda()
        y = torch.from_numpy(lab).cuda()
        def call():                                        # forward, loss and backward; no Adam step: the parameters stay what they are
            tr.backward_on_device(x, y)
            return {"grads": tr.grads.clone(), "loss": tr.loss.clone()}
        return call
    return make


def _loss():
    from ubdvss_amd import losses, synthetic
    lab = synthetic.rectangle_maps(30, 2, 16, 16, side_min=3, side_max=10)
    y = torch.from_numpy(lab).cuda()
    logits = torch.from_numpy(synthetic.logits_from_maps(lab, 0, seed=5)).cuda()
    def call():
        loss, grad = losses.loss_and_grad(y, logits)
        return {"loss": loss.clone(), "dlogits": grad.clone()}
    return call


def _postprocess():
    from ubdvss_amd import NetConfig, Model, synthetic
    m = Model(NetConfig(grey=False), seed=1)
    lt = torch.from_numpy(synthetic.logits_from_maps(synthetic.rectangle_maps(3, 2, 16, 16, side_min=3, side_max=10), 0, seed=5)).cuda()
    def call():
        bmap, quads, _, counts = m.postprocess_on_device(lt, 0.0, 4, 5, cap=64)
        listed = torch.arange(64, device="cuda")[None, :] < counts[:, None]           # entries behind a list's end are unspecified (alloc_postprocess_outputs)
        return {"binary_map": bmap.clone(), "quads": quads * listed[:, :, None], "counts": counts.clone()}
    return call


TWO_CUS = {"UBD_TEST_NUM_CUS": "2"}          # every block walks several strips
SEQ8, SEQ10 = list(range(8)), list(range(10))
# stamp families of a case: (family, selectors, buffer shape, label order of the slots in the last axis).  The shapes are the tools' with
# fewer blocks; a slot that was not written is 0.
CASES = {
    "fwd32": (_forward("float32", TWO_CUS), [("stem123", (), (2 * 8 * 16 * 8 + 2 * 32,), None)]),
    **{f"fwd32_layer{k}": (_layer(TWO_CUS, k), [("wino6", (), (512, 8), SEQ8)]) for k in (0, 2, 4)},
    "fwd32_wino32": (_forward("float32", dict(TWO_CUS, UBD_DILCONV="wino32")), []),
    **{f"fwd32_wino32_layer{k}": (_layer(dict(TWO_CUS, UBD_DILCONV="wino32"), k), [("wino", (), (512, 8), SEQ8)]) for k in (0, 2, 4)},
    "fwd32_fused": (_forward("float32", dict(TWO_CUS, UBD_STEM="fused")), [("stem23", (), (64, 8, 16, 8), SEQ8)]),
    "fwd16": (_forward("bfloat16", {}), [("sep123_16", (), (768, 4, 16, 8), SEQ8), ("dilconv16s", (1,), (768, 4, 8, 8), None)]),
    "train16": (_train("bfloat16"), [("sepb16", (24, 1), (256, 4, 8, 12), SEQ10), ("sepb16", (3, 2), (256, 4, 8, 12), SEQ10),
                                     ("sepb16", (24, 2), (256, 4, 8, 12), SEQ10), ("dil_wgrad16", (1,), (256, 4, 8, 8), list(range(6)))]),
    "train32": (_train("float32"), [("sep_bwd", (24, 1), (256, 4, 8, 12), SEQ10), ("sep_bwd", (3, 2), (256, 4, 8, 12), SEQ10),
                                    ("sep_bwd", (24, 2), (256, 4, 8, 12), SEQ10)]),
    "loss": (_loss, [("loss", (), (256, 16), [0, 1, 2, 3, 12, 4, 5, 13, 6, 7, 14, 8, 9, 10])]),
    "postprocess": (_postprocess, [("postprocess", (), (2, 16), list(range(16)))]),
}
BOUNDED = {("wino6", ()), ("sepb16", (24, 1))}      # (c): also run with 64 words registered inside a poisoned allocation
POISON = 0x5A5A5A5A5A5A5A5A


def outputs(name):
    """One call of the case on whatever library the process has loaded: name -> numpy array."""
    call = CASES[name][0]()
    out = {k: v.cpu().numpy() for k, v in call().items()}
    torch.cuda.synchronize()
    return out


def _check_order(what, s, order):
    """s (..., slots): in every group with a written slot, the written slots do not decrease in label order.  Returns the number of such groups."""
    g = s.reshape(-1, s.shape[-1])[:, order]
    g = g[(g != 0).any(axis=1)]
    for row in g:
        w = row[row != 0]
        assert (np.diff(w) >= 0).all(), f"{what}: stamps decrease in label order: {row.tolist()}"
    return len(g)


def _check_family(what, family, s, order):
    if family == "stem123":            # tile stamps (block, wave, tile, 8), behind them the block time lines (block, 32): entry, job done, ring ready, patch landed,
        tiles, blocks = s[:2 * 8 * 16 * 8].reshape(2, 8, 16, 8), s[2 * 8 * 16 * 8:].reshape(2, 32)       # first L1 phase, the strips' starts, end (tools/stamps_stem_blocks.py)
        n = _check_order(what + " tiles", tiles, SEQ8)
        nb = _check_order(what + " block time line", blocks, [0, 1, 3, 29, 30] + list(range(4, 28)) + [2])
        assert nb > 0, f"{what}: no block time line written"
        assert (blocks[:, 5] != 0).any(), f"{what}: no block walked a second strip"
    elif family == "dilconv16s":       # item stamps 0..4; the block time line in slots 5..7 of items 0 (shader clock) and 1 (100-MHz clock) (tools/stamps_d16s.py)
        n = _check_order(what + " items", s[..., :5], list(range(5)))
        assert _check_order(what + " block time line", s[:, :, :2, 5:], [0, 1, 2]) > 0, f"{what}: no block time line written"
    else:
        n = _check_order(what, s, order)
    assert n > 0, f"{what}: no slot written"
    return n


def child_main(product_npz):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import _diag
    lib = _diag.load()
    assert lib.ubd_debug_set_stamps(b"no_such_kernel", None, 0, 0, 0) != 0 and b"no_such_kernel" in lib.ubd_last_error()
    product = np.load(product_npz)
    for name, (make, families) in CASES.items():
        call = make()
        run = lambda: {k: v.cpu().numpy() for k, v in call().items()}
        plain = run()
        torch.cuda.synchronize()
        for k, v in plain.items():                                                           # (d)
            ref = product[f"{name}/{k}"]
            if v.dtype.kind in "iu":
                assert np.array_equal(v, ref), f"{name}/{k}: differs from the product library"
                continue
            diff = float(np.abs(v.astype(np.float64) - ref.astype(np.float64)).max())
            print(f"{name}/{k}: max |diagnostic - product| = {diff:.3e} (max |product| = {float(np.abs(ref).max()):.3e})")
            if name.startswith("fwd32"):
                assert diff <= 2e-5 * float(np.abs(ref).max()) + 1e-6, f"{name}/{k}: {diff} from the product library"
        for family, sel, shape, order in families:
            what = f"{name}: {family}{list(sel)}"
            kept = {}
            s = _diag.stamps(lib, family, shape, lambda: kept.update(run()), sel=sel)
            for k, v in plain.items():                                                       # (a)
                assert np.array_equal(v, kept[k]), f"{what}: {k} changes when stamps are set"
            n = _check_family(what, family, s, order)                                        # (b)
            print(f"{what}: {n} slot groups written, outputs bit-equal")
            if (family, sel) in BOUNDED:                                # (c)
                s = _diag.stamps(lib, family, (4096,), lambda: kept.update(run()), sel=sel, capacity=64, fill=POISON)
                for k, v in plain.items():
                    assert np.array_equal(v, kept[k]), f"{what}: {k} changes when stamps are set"
                assert (s[64:] == POISON).all(), f"{what}: stored beyond the registered capacity of 64 words"
                assert (s[:64] != POISON).any(), f"{what}: nothing stored below the registered capacity"
                print(f"{what}: capacity 64 respected, {int((s[:64] != POISON).sum())} words written below it")
    print("DIAG_STAMPS_CHILD OK")


if __name__ == "__main__":
    child_main(sys.argv[1])
