"""Fuzz of one dilated layer through ubd_dilated_layer: the split-product forms (wino6.hip: two fp16 pieces, the default, and three bf16 pieces,
UBD_DILCONV=split3) against the fp32-MFMA form (UBD_DILCONV=wino32) on random map sizes (1 x 1 .. 70 x 150, any residue), batch sizes and all six
layers (dilations 1, 2, 4, 8, 16, 1).  Bound: 4e-6 of the layer's largest value (the forms differ by rounding only).  FUZZ_CASES scales it (default 300)."""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import NetConfig, Model, _lib
torch.cuda.set_device(0)
lib = _lib.load()
def make(env):
    if env: os.environ["UBD_DILCONV"] = env
    else: os.environ.pop("UBD_DILCONV", None)
    m = Model(NetConfig(grey=False), seed=1)
    ws = torch.empty(int(lib.ubd_forward_workspace_bytes(m._h, 1, 4, 4)), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ubd_pack_weights(m._h, m.params.data_ptr(), ws.data_ptr(), ws.numel(), st), "pack")
    return m, ws, st
A, S, B = make("wino32"), make("split3"), make("")
os.environ.pop("UBD_DILCONV", None)
rng = np.random.default_rng(int(os.environ.get("FUZZ_SEED", 1)))
worst, worst3, bad = 0.0, 0.0, 0
cases = int(os.environ.get("FUZZ_CASES", 300))
for c in range(cases):
    n = int(rng.integers(1, 5)); hh = int(rng.integers(1, 71)); ww = int(rng.integers(1, 151))
    if c % 7 == 0: hh, ww = int(rng.integers(1, 6)), int(rng.integers(1, 6))
    k = int(rng.integers(0, 6))
    x = (torch.rand((n, hh, ww, 24), device="cuda") - 0.3) * float(rng.choice([1.0, 100.0, 1e-3]))
    ys = []
    for m, ws, st in (A, B, S):
        y = torch.full_like(x, float("nan"))
        _lib.check(lib.ubd_dilated_layer(m._h, m.params.data_ptr(), k, x.data_ptr(), y.data_ptr(), n, hh, ww, ws.data_ptr(), st), "dil")
        ys.append(y)
    torch.cuda.synchronize()
    if any(bool(torch.isnan(y).any()) for y in ys):
        bad += 1; print("case", c, (n, hh, ww, k), "NaN / unwritten outputs:", [int(torch.isnan(y).sum()) for y in ys]); continue
    top = max(float(ys[0].abs().max()), 1e-30)
    e, e3 = float((ys[0] - ys[1]).abs().max()) / top, float((ys[0] - ys[2]).abs().max()) / top
    worst, worst3 = max(worst, e), max(worst3, e3)
    if e > 4e-6 or e3 > 4e-6:
        bad += 1; print("case", c, (n, hh, ww, k), "rel diff default", e, "split3", e3)
print(f"{cases} cases, worst relative difference {worst:.2e} (split3: {worst3:.2e}), failures {bad}")
sys.exit(1 if bad else 0)
