"""In-kernel phase timing of sepb16_kernel (diagnostic build): s_memtime of every wave at the phase boundaries of its first
8 tiles, bf16 train step at batch 64.  Usage: stamps_sepb.py [cin stride]  (24 1 = L2, 3 2 = L1, 24 2 = L3)"""
import numpy as np, torch
import _diag
from ubdvss_amd import NetConfig, Model, Trainer, Adam, synthetic
torch.cuda.set_device(0)
lib = _diag.load()
m = Model(NetConfig(grey=False), dtype="bfloat16", seed=1)
tr = Trainer(m, Adam())
lab = synthetic.rectangle_maps(30, 64, 128, 128)
x = torch.from_numpy(synthetic.textured_images(31, lab, 4, 3).astype(np.float32) / 127.5 - 1.0).cuda()
y = torch.from_numpy(lab).cuda()
for _ in range(100): tr.train_step_on_device(x, y)
names = ["top barrier", "stage X / write xf32 / mask loads", "wait DMA + barrier + border fix", "phase 1 (G tile)", "barrier", "next tile: D DMA / x / mask loads", "phase 2a (dDW, depthwise, dpw)", "barrier", "phase 2b (ddw)"]
for cin, stride in ((24, 1), (3, 2), (24, 2)):
    s = _diag.stamps(lib, "sepb16", (1024, 4, 8, 12), lambda: tr.train_step_on_device(x, y), sel=(cin, stride))
    used = s[:, 0, 2, 0] > 0
    s = s[used]
    if not (s[0, 0, 2, 8] > 0): s[:, :, :, 7] = s[:, :, :, 9]; s[:, :, :, 8] = s[:, :, :, 9]   # 1/3-channel kernel: phase 2 in one piece
    seg = np.diff(s[:, :, 1:7, :10], axis=-1)          # (blk, wave, tile 1..6, 7 segments between the 8 stamps)
    nxt = s[:, :, 2:8, 0] - s[:, :, 1:7, 9]          # end of phase 2 -> top of the next tile
    period = s[:, 0, 2:8, 0] - s[:, 0, 1:7, 0]
    print(f"sepb16<{cin},{stride}>: blocks {used.sum()}, tile period median {np.median(period):.0f} cycles")
    for w in range(4):
        print(f"  wave {w}: " + "  ".join(f"{names[k]}: {np.median(seg[:, w, :, k]):.0f}" for k in range(9)) + f"  loop: {np.median(nxt[:, w]):.0f}")
