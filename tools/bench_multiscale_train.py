"""The multi-scale train step (ubd_train_step_multiscale, Trainer around a MultiscaleModel) on one MI355X against the single-scale
step (ubd_train_step) of the same handle, batch and size.

Two legs, timed in ONE process on a ring of fresh uint8 RGB batches with their label maps, per handle precision (--dtypes), --power 3,
at --batch 32 x 512 x 512:
  single      Trainer(model).backward_on_device: forward, loss, backward of the single-scale net;
  multiscale  Trainer(MultiscaleModel(model, power)).backward_on_device: gather, power + 1 training forwards, fuse, loss on the mean
              map, fuse adjoint, power + 1 backward passes, gradient sum.
Neither leg includes Adam.  The legs alternate inside every round; a round times --reps back-to-back steps of a leg between two
device events.  Prints one JSON line per precision: median and minimum over the rounds of the time per step, the ratio
multiscale / single, and the sum of the levels' pixel shares 1 + 1/4 + ... + 1/4^power that the ratio is to be read against.
Usage: python tools/bench_multiscale_train.py [--rounds 20] [--reps 10] [--power 3] [--batch 32] [--side 512] [--dtypes float32,bfloat16]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import Adam, NetConfig, Model, MultiscaleModel, PreprocessingType, Trainer, synthetic  # noqa: E402


def bench_dtype(dtype, n, side, power, rounds, reps, ring):
    cfg = NetConfig(grey=False, preprocessing=PreprocessingType.MOBILENET_LIKE)
    base = Model(cfg, dtype=dtype, seed=0)
    legs = {"single": Trainer(base, Adam(), process_group=False), "multiscale": Trainer(MultiscaleModel(base, power), Adam(), process_group=False)}
    labels = [synthetic.rectangle_maps(3 + k, n, side // 4, side // 4) for k in range(ring)]
    xs = [torch.from_numpy(synthetic.textured_images(4 + k, lab, 4, 3)).cuda() for k, lab in enumerate(labels)]
    ys = [torch.from_numpy(lab).cuda() for lab in labels]
    for tr in legs.values():                                    # every leg before the timed window
        for k in range(2):
            tr.backward_on_device(xs[k], ys[k])
    torch.cuda.synchronize()
    losses = {name: float(tr.loss[0]) for name, tr in legs.items()}
    times = {name: [] for name in legs}
    k = 0
    for _ in range(rounds):
        for name, tr in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                tr.backward_on_device(xs[k % ring], ys[k % ring])
                k += 1
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / reps)
    res = {"shape": [n, side, side, 3], "dtype": dtype, "max_scale_power": power, "rounds": rounds, "reps": reps}
    for name, t in times.items():
        res[f"{name}_ms_median"] = round(float(np.median(t)), 4)
        res[f"{name}_ms_min"] = round(float(np.min(t)), 4)
        res[f"{name}_loss"] = losses[name]
        res[f"{name}_workspace_MiB"] = round(legs[name]._ws.numel() / 2 ** 20, 1)
    res["multiscale_over_single"] = round(res["multiscale_ms_median"] / res["single_ms_median"], 3)
    res["sum_of_level_shares"] = round(sum(0.25 ** s for s in range(power + 1)), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--power", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--dtypes", default="float32,bfloat16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiscale_train needs an MI355X: nothing is measured without one")
    for dtype in args.dtypes.split(","):
        print(json.dumps(bench_dtype(dtype, args.batch, args.side, args.power, args.rounds, args.reps, args.ring)), flush=True)


if __name__ == "__main__":
    main()
