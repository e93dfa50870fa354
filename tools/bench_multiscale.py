"""Multi-scale inference (ubd_forward_multiscale, MultiscaleModel) on one MI355X against what it replaces.

Three ways to get logits from a batch, timed in ONE process on a ring of fresh uint8 RGB input batches (no call sees the batch
of the call before it), fp32 model, --power 3, at 32 x 512 x 512 and at 1 x 512 x 512:
  single      (a) the single-scale pass, Model.predict_on_device: the yardstick the multi-scale cost is a multiple of;
  composed    (b) what the package offered before MultiscaleModel: one Model.predict_on_device per level on
              x[:, ::f, ::f].contiguous(), torch repeat_interleave of every coarser result and the mean of the stack;
  multiscale  (c) MultiscaleModel.predict_on_device (one ubd_forward_multiscale call), eager,
  graph       and the same chain replayed as one captured HIP graph (the replay includes the copy of the batch into the graph's
              static input).
The legs alternate inside every round; a round times --reps back-to-back calls of a leg (five times as many for one image)
between two device events.  Per leg:
median and minimum over the rounds of the time per call.  Prints one JSON line per shape with the four times, the ratios
multiscale / single and multiscale / composed, and whether (c) matched (b)'s result (max |difference|; the two are not bit-equal:
torch's mean adds in another order).
Usage: python tools/bench_multiscale.py [--rounds 30] [--reps 10] [--power 3] [--ring 6]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import NetConfig, Model, MultiscaleModel, PreprocessingType  # noqa: E402


def composed(base, x, power):
    ys = [base.predict_on_device(x)]
    for s in range(1, power + 1):
        f = 2 ** s
        y = base.predict_on_device(x[:, ::f, ::f].contiguous())
        ys.append(y.repeat_interleave(f, dim=1).repeat_interleave(f, dim=2))
    return torch.stack(ys).mean(dim=0)


def bench_shape(base, ms, n, side, power, rounds, reps, ring):
    gen = torch.Generator(device="cuda").manual_seed(n)
    xs = [torch.randint(0, 256, (n, side, side, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(ring)]
    out_a = torch.empty((n, side // 4, side // 4, base.k_out), dtype=torch.float32, device="cuda")
    out_c = torch.empty_like(out_a)
    gf = ms.graphed_forward(n, side, side, torch.uint8)
    legs = {
        "single": lambda x: base.predict_on_device(x, out=out_a),
        "composed": lambda x: composed(base, x, power),
        "multiscale": lambda x: ms.predict_on_device(x, out=out_c),
        "graph": lambda x: gf(x),
    }
    diff = float((legs["multiscale"](xs[0]) - legs["composed"](xs[0])).abs().max())
    graph_equal = bool(torch.equal(legs["graph"](xs[0]), legs["multiscale"](xs[0])))
    for fn in legs.values():                                    # every leg, every shape it uses, before the timed window
        for x in xs[:2]:
            fn(x)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    k = 0
    for _ in range(rounds):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn(xs[k % ring])
                k += 1
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / reps)
    res = {"shape": [n, side, side, 3], "dtype": base.dtype, "max_scale_power": power, "rounds": rounds, "reps": reps}
    for name, t in times.items():
        res[f"{name}_ms_median"] = round(float(np.median(t)), 4)
        res[f"{name}_ms_min"] = round(float(np.min(t)), 4)
    res["multiscale_over_single"] = round(res["multiscale_ms_median"] / res["single_ms_median"], 3)
    res["multiscale_over_composed"] = round(res["multiscale_ms_median"] / res["composed_ms_median"], 3)
    res["graph_over_composed"] = round(res["graph_ms_median"] / res["composed_ms_median"], 3)
    res["max_abs_diff_multiscale_vs_composed"] = diff
    res["graph_bit_equal_to_eager"] = graph_equal
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--power", type=int, default=3)
    ap.add_argument("--ring", type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiscale needs an MI355X: nothing is measured without one")
    cfg = NetConfig(grey=False, preprocessing=PreprocessingType.MOBILENET_LIKE)
    base = Model(cfg, dtype="float32", seed=0)
    ms = MultiscaleModel(base, args.power)
    for n in (32, 1):
        reps = args.reps if n > 1 else 5 * args.reps            # one image is a tenth of a millisecond: a longer window per round
        print(json.dumps(bench_shape(base, ms, n, 512, args.power, args.rounds, reps, args.ring)), flush=True)


if __name__ == "__main__":
    main()
