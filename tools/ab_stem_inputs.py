"""A/B of two builds of the library inside one box (tools/ab_lib.py's form, builds under tools/_ab/): the fp32 forward pass at batch 32 of
512 x 512 x 3 for each input form the one-kernel stem takes -- uint8 pixels (preprocessing fused), fp32 fed as it is (LDS-DMA) and fp32
at a base that is not 16-byte aligned (registers, like preprocessed input).  usage: ab_stem_inputs.py [old.so new.so ...]"""
import os, sys, subprocess, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == "child":
    import torch
    sys.path.insert(0, ROOT)
    from ubdvss_amd import _lib
    _lib.LIB_PATH = sys.argv[2] if os.path.isabs(sys.argv[2]) else os.path.join(ROOT, "tools", "_ab", sys.argv[2])
    from ubdvss_amd import NetConfig, Model, synthetic
    torch.cuda.set_device(0)
    def timed(fn, reps):
        for _ in range(20): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    m = Model(NetConfig(grey=False), seed=1)
    xu8 = torch.from_numpy(synthetic.noise_images(2, 32, 512, 512, 3, as_float=False)).cuda()
    xf = torch.from_numpy(synthetic.noise_images(2, 32, 512, 512, 3)).cuda()
    flat = torch.empty(xf.numel() + 1, dtype=torch.float32, device="cuda")
    xa = flat[1:].view(xf.shape)                                                  # base 4 bytes past a 16-byte boundary
    xa.copy_(xf)
    out = {"u8_ms": [], "plain_ms": [], "unaligned_ms": []}
    for _ in range(3):
        out["u8_ms"].append(round(timed(lambda: m.predict_on_device(xu8), 200), 4))
        out["plain_ms"].append(round(timed(lambda: m.predict_on_device(xf), 200), 4))
        out["unaligned_ms"].append(round(timed(lambda: m.predict_on_device(xa), 200), 4))
    print(json.dumps(out))
else:
    for rep in range(2):
        for lib in (sys.argv[1:] or ["old.so", "new.so"]):
            r = subprocess.run([sys.executable, __file__, "child", lib], capture_output=True, text=True)
            print(lib, r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-300:], flush=True)
