"""What the epoch loop costs per step: bf16 train step at batch 64 x 512 x 512 (the bench's train shape), STEPS steps timed three
ways in one process, the three alternated over REPEATS rounds:
  (i)   bare Trainer.train_step_on_device;
  (ii)  the same plus loss[0].item() after every step (the loop a user had to write before Trainer.fit);
  (iii) Trainer.fit with steps_per_epoch = STEPS, one epoch, no validation, no callbacks (ubd_epoch_accumulate per step, one read).
Host wall clock around work that ends in a device synchronise (fit ends in its read).  Prints ms per step; not a test.
usage: bench_fit_overhead.py [steps=200] [repeats=3] [dtype=bfloat16]"""
import itertools
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import NetConfig, Model, Trainer, Adam, synthetic  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dtype = sys.argv[3] if len(sys.argv) > 3 else "bfloat16"
torch.cuda.set_device(0)
tr = Trainer(Model(NetConfig(grey=False), dtype=dtype, seed=1), Adam())
lab = synthetic.rectangle_maps(30, 64, 128, 128)
x = torch.from_numpy(synthetic.textured_images(31, lab, 4, 3).astype(np.float32) / 127.5 - 1.0).cuda()
y = torch.from_numpy(lab).cuda()


def bare():
    for _ in range(steps):
        tr.train_step_on_device(x, y)
    torch.cuda.synchronize()


def read_every_step():
    for _ in range(steps):
        tr.train_step_on_device(x, y)[0].item()
    torch.cuda.synchronize()


def fit():
    tr.fit(itertools.repeat((x, y)), steps, 1)


variants = [("bare train_step_on_device", bare), ("+ loss[0].item() per step", read_every_step), ("Trainer.fit", fit)]
for _ in range(60):
    tr.train_step_on_device(x, y)
tr.fit(itertools.repeat((x, y)), 5, 1)
torch.cuda.synchronize()
times = {name: [] for name, _ in variants}
for rep in range(repeats):
    for name, fn in variants:
        t0 = time.perf_counter()
        fn()
        times[name].append((time.perf_counter() - t0) / steps * 1e3)
for name, _ in variants:
    ts = times[name]
    print(f"{dtype} batch 64 x 512 x 512, {steps} steps: {name:28s} {min(ts):.4f} ms/step (best of {repeats}; all: "
          + ", ".join(f"{t:.4f}" for t in ts) + ")", flush=True)
