"""In-kernel phase timing of pp_front_lds_kernel (diagnostic build): s_memtime of thread 0 after every block barrier."""
import numpy as np, torch
import _diag
from ubdvss_amd import NetConfig, Model, synthetic
torch.cuda.set_device(0)
lib = _diag.load()
m = Model(NetConfig(grey=False), seed=1)
labels = synthetic.rectangle_maps(3, 32, 128, 128)
for name, lg in (("rectangle maps", synthetic.logits_from_maps(labels, 0, seed=5)), ("net-like maps (97 % foreground, hundreds of holes)", np.where(np.random.default_rng(2).random((32, 128, 128, 1)) < 0.02, -1.0, 1.0).astype(np.float32)), ("noise maps (p=0.5)", np.where(np.random.default_rng(1).random((32, 128, 128, 1)) < 0.5, 1.0, -1.0).astype(np.float32))):
    lt = torch.from_numpy(lg).cuda()
    for _ in range(200): m.postprocess_on_device(lt, 0.0, 4, 5, cap=1024)
    s = _diag.stamps(lib, "postprocess", (32, 16), lambda: m.postprocess_on_device(lt, 0.0, 4, 5, cap=1024))
    k = int((s[0] > 0).sum())
    seg = np.diff(s[:, :k], axis=1)
    names = ["init", "merge", "flatten", "roots", "owner", "zero area", "area", "keep", "rows init", "extents", "boxes + vote", "emit"]
    print(name, "total cycles median", int(np.median(s[:, k - 1] - s[:, 0])))
    print("   " + "  ".join(f"{names[i] if i < len(names) else i}: {int(np.median(seg[:, i]))}" for i in range(k - 1)))
