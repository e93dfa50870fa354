"""bench.py -- headline benchmark of the ubdvss hot path on MI355X.

Metric (BASELINE.json): images/sec at 512x512 for forward + CCL postprocess.
Workload at every N: BASELINE.json configs[1] per GPU -- batch=32 512x512x3 fp32 forward + device
postprocess (threshold -> external components -> quads).  A "step" = one pass of that path over one
synthetic batch already resident in HBM.  Multi-GPU: images shard by rank with no data-path
collective (replicas), weak scaling (32 images per GPU), value = all ranks' images / max-over-ranks
time.  A plain run sets up, settles the clocks, runs W warm-up steps, times exactly K steps (ms_per_step = their time / K)
and prints the headline line; --dump-outputs DIR then also writes the last timed step's results as DIR/<name>.npy.

Extra objects on the JSON line, with --full only (none of them changes the headline):
  ms_per_step_spread -- five more blocks of K steps, and the median of all six
  roofline     -- the dominant kernel (dense dilated 3x3 conv; Winograd with bf16 split products since round 6), timed live with HIP events
  cpu_baseline -- the torch-CPU restatement (oracle/, kind "port") on a bounded sample, rank 0, N=1
  parts        -- net-only / postprocess-only timings of the same step
  latency_batch1 -- the reference's own metric (predict.py:73-78): one timed predict of zeros (1,S,S,1) after one warm-up
  train_step*, forward_fp16_cfg5, pcie_inclusive_host_numpy -- the other configs, precisions and the host path; for N>1 the
                  data-parallel train leg
Launch: python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR].  For N>1 either the driver starts the ranks
(python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...) or, when no WORLD_SIZE is set, this script
starts them itself as child processes BEFORE anything touches the GPU and relays rank 0's JSON line.  Every rank
counts the ranks RCCL really connected (all-reduce of ones -> "n_ranks_rccl") and exits non-zero if that is not N.
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH, SIDE, C_IN = 32, 512, 3
BYTES_PER_IMAGE_FP32 = 50.40e6            # layer-wise compulsory traffic, 512x512x3, n_cls = 0
FLOP_PER_IMAGE = 1.1627e9
PEAK_MFMA_F32 = 157.3                     # TFLOP/s, MI355X_MICROARCH.md (f32-input MFMA = vector peak)
PEAK_HBM = 8000.0                         # GB/s
SETTLE_STEPS = 300                        # untimed steps (settle + warm-up) before EVERY timed region: clock ramp after idle
RING = 4                                  # distinct input batches the timed loops rotate over (4 x 100.7 MB > 256 MB Infinity Cache)


def timed_events(fn, reps, settle=SETTLE_STEPS):
    """Mean time of one call of fn in ms (HIP events on torch's current stream = the launch stream of every call here), after
    `settle` untimed calls: each leg of the line comes after an idle gap (synthetic data generation, allocation), and the chip
    needs a few hundred back-to-back launches before its clocks are where a long run holds them."""
    for _ in range(max(1, settle)):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def csrc_sha16():
    """Fingerprint of the kernel sources the library was built from: the committed profile summaries carry the fingerprint of
    the sources they were measured on (profiles/*_profile_meta.json, tools/profile_meta.py)."""
    import glob
    import hashlib
    hsh = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "ubdvss_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "ubdvss_amd", "csrc", "*.h"))):
        hsh.update(os.path.basename(f).encode())
        hsh.update(open(f, "rb").read())
    return hsh.hexdigest()[:16]


def library_build_id():
    """Fingerprint of the kernel sources the LOADED libubd_hip.so was compiled from (ubd_build_id, written by build.sh): what the
    committed profiles are compared with -- the files on disk may have been edited since the build."""
    from ubdvss_amd import _lib
    return _lib.load().ubd_build_id().decode()


def committed_profile(kernel_prefix):
    """(traffic MB per launch, average launch us, file names, whether the profile was taken on the sources of this build) from
    the NEWEST committed profile set under profiles/ -- values measured in another run and labelled as such on the line."""
    import csv
    traffic = avg_us = None
    files = {}
    meta = {}
    for rnd in ("r06", "r05", "r04", "r03", "r02"):
        if traffic is None:
            try:
                for ln in open(os.path.join(ROOT, "profiles", f"{rnd}_pmc_traffic_fwd_fp32.txt")):
                    if ln.startswith(kernel_prefix):
                        parts = ln.split()
                        traffic = round(float(parts[-2]) + float(parts[-1]), 1)      # read MB (FETCH_SIZE already doubled) + written MB
                        files["traffic"] = f"profiles/{rnd}_pmc_traffic_fwd_fp32.txt"
            except (OSError, ValueError, IndexError):
                pass
        if avg_us is None:
            try:
                with open(os.path.join(ROOT, "profiles", f"{rnd}_bench_kernel_stats.csv")) as f:
                    for row in csv.DictReader(f):
                        if row["Name"].startswith(kernel_prefix):
                            avg_us = round(float(row.get("FullSizeAverageNs") or row["AverageNs"]) / 1e3, 2)   # full-size launches only
                            files["avg"] = f"profiles/{rnd}_bench_kernel_stats.csv"
                            break
            except (OSError, KeyError, ValueError):
                pass
        if not meta:
            try:
                meta = json.load(open(os.path.join(ROOT, "profiles", f"{rnd}_profile_meta.json")))
                meta["round"] = rnd
            except (OSError, ValueError):
                meta = {}
    fresh = bool(meta) and meta.get("csrc_sha16") == library_build_id() and all(v.startswith(f"profiles/{meta['round']}_") for v in files.values())
    return traffic, avg_us, files, fresh


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="ranks (one per GPU); default: WORLD_SIZE or 1")
    ap.add_argument("--dry-run", action="store_true", help="CPU/gloo check of the N-rank launch, barrier and timing plumbing (no GPU work)")
    ap.add_argument("--cpu-child", choices=["forward", "train", "latency"], help=argparse.SUPPRESS)
    ap.add_argument("--cpu-threads", type=int, default=32, help="threads of the CPU baseline (pinned, one per physical core)")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-train", action="store_true", help="skip the extra train-step measurement")
    ap.add_argument("--train-batch", type=int, default=64)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: spread over more blocks, other paths / sizes / precisions, train legs, batch-1 latency, "
                         "PCIe-inclusive host path, parts, roofline, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0), e.g. bench_outputs")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def dump_outputs(path, out):
    """The arrays a caller of the timed path receives from its last step (ModelRunner.predict_on_device, complete after the flush):
    logits, binary map, object counts, and the quads of every image's list up to its count (entries behind a list's end are
    unspecified, so they are not written).  float32 / float64, about 4 MB."""
    logits, bmap, quads, classes, counts = out
    os.makedirs(path, exist_ok=True)
    counts_h = counts.cpu().numpy()
    n_kept = np.minimum(counts_h, quads.shape[1])
    arrays = {"logits": logits.cpu().numpy().astype(np.float32), "binary_map": bmap.cpu().numpy().astype(np.float32),
              "counts": counts_h.astype(np.float64),
              "quads": np.concatenate([q[:k] for q, k in zip(quads.cpu().numpy(), n_kept)]).astype(np.float64).reshape(-1, 8)}
    if classes is not None:
        arrays["classes"] = np.concatenate([c[:k] for c, k in zip(classes.cpu().numpy(), n_kept)]).astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(path, f"{name}.npy"), a)


# ------------------------------------------------------------------------------------------------ CPU baseline
# The CPU legs run in a CHILD process that never touches the GPU: it pins itself to one hardware thread per physical
# core of ONE socket before torch creates its thread pool, so the figure does not depend on where the scheduler puts
# 32 threads on a 256-CPU host (round 1: 145 vs 526 images/s between two runs).  The parent only starts the child
# (a plain subprocess, no exec) and parses its JSON line.

def _pick_cpus(n_threads):
    """One hardware thread per physical core, all on the socket that offers the most allowed cores."""
    allowed = sorted(os.sched_getaffinity(0))
    by_pkg = {}
    for c in allowed:
        try:
            base = f"/sys/devices/system/cpu/cpu{c}/topology/"
            pkg = int(open(base + "physical_package_id").read())
            core = int(open(base + "core_id").read())
        except (OSError, ValueError):
            pkg, core = 0, c
        by_pkg.setdefault(pkg, {}).setdefault(core, c)          # first (lowest) hw thread of every core
    pkg = max(by_pkg, key=lambda k: len(by_pkg[k]))
    cpus = sorted(by_pkg[pkg].values())[:n_threads]
    return cpus, pkg, len(by_pkg[pkg])


def _cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _timed_repeats(step, seconds, min_reps=5, max_reps=60):
    step(); step()                                               # warm-up: oneDNN primitive creation, page faults
    times = []
    t_start = time.perf_counter()
    while len(times) < max_reps and (len(times) < min_reps or time.perf_counter() - t_start < seconds):
        t0 = time.perf_counter(); step(); times.append(time.perf_counter() - t0)
    return times, time.perf_counter() - t_start


def cpu_child(kind, seconds, n_threads):
    """Runs in the child process (bench.py --cpu-child ...).  Prints one JSON object."""
    cpus, pkg, cores_on_pkg = _pick_cpus(n_threads)
    os.sched_setaffinity(0, cpus)
    os.environ["OMP_NUM_THREADS"] = str(len(cpus))
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    import numpy as np
    import torch
    torch.set_num_threads(len(cpus))
    from oracle import net_numpy as onet, net_torch as otorch, cv_post as ocv
    from ubdvss_amd import synthetic
    pin = {"cores": len(cpus), "pinned_to": f"{len(cpus)} physical cores of socket {pkg} (of {cores_on_pkg} allowed there), one thread per core",
           "cpu_model": _cpu_model(), "host_cpus": os.cpu_count()}
    if kind == "forward":
        # the SAME tensor shape as the GPU step: one batch of 32 stripe-textured 512x512x3 images
        w = onet.init_weights(1, C_IN, 0)
        tw = otorch.to_torch_weights(w, torch.float32)
        labels = synthetic.rectangle_maps(3, BATCH, SIDE // 4, SIDE // 4)
        x = torch.from_numpy(synthetic.textured_images(4, labels, 4, C_IN).astype(np.float32) / 127.5 - 1.0)

        def step():
            with torch.no_grad():
                lg = otorch.forward(x, tw).numpy()
            det = (lg[..., 0] > -0.0).astype(np.uint8)
            return [ocv.postprocess(det[i], None, 4, 5) for i in range(BATCH)]
        times, el = _timed_repeats(step, seconds)
        # value = the MEDIAN repeat (BASELINE.md section 3 / SURVEY.md 8(d)); the GPU boxes' hosts are shared (256 CPUs, other
        # tenants) and repeats on pinned cores scatter, so the fastest and slowest repeat are reported beside it
        res = {"value": round(BATCH / float(np.median(times)), 2), "unit": "images/s", "kind": "port", **pin,
               "fastest": round(BATCH / min(times), 2), "slowest": round(BATCH / max(times), 2), "repeats": len(times),
               "spread_images_per_s": {"min": round(BATCH / max(times), 2), "p10": round(BATCH / float(np.percentile(times, 90)), 2),
                                       "median": round(BATCH / float(np.median(times)), 2), "p90": round(BATCH / float(np.percentile(times, 10)), 2),
                                       "max": round(BATCH / min(times), 2)},
               "sample": f"{len(times)} repeats of ONE batch of {BATCH} textured 512x512x3 images (the GPU step's tensor), torch-CPU fp32 "
                         f"forward (oneDNN) + C restatement of the OpenCV postprocess; value = median repeat, {el:.1f} s in all"}
    elif kind == "train":
        nb = 8                                                    # the reference's default batch (train.py:31)
        w = onet.init_weights(1, C_IN, 0)
        labels = synthetic.rectangle_maps(30, nb, SIDE // 4, SIDE // 4)
        x = synthetic.textured_images(31, labels, 4, C_IN).astype(np.float32) / 127.5 - 1.0
        state = {"flat": np.concatenate([a.reshape(-1) for a in w]).astype(np.float64), "t": 0}
        state["m"] = np.zeros_like(state["flat"]); state["v"] = np.zeros_like(state["flat"])

        def step():
            state["t"] += 1
            _, _, _, grads = otorch.loss_and_grads(x, labels[..., None], onet.unflatten_weights(state["flat"].astype(np.float32), C_IN, 0),
                                                   False, True, dtype=torch.float32)
            g = np.concatenate([a.reshape(-1) for a in grads]).astype(np.float64)
            state["flat"], state["m"], state["v"] = otorch.adam_step(state["flat"], g, state["m"], state["v"], state["t"])
        times, el = _timed_repeats(step, seconds)
        res = {"value": round(nb / float(np.median(times)), 2), "unit": "images/s", "kind": "port", **pin,
               "fastest": round(nb / min(times), 2), "slowest": round(nb / max(times), 2), "repeats": len(times),
               "spread_images_per_s": {"min": round(nb / max(times), 2), "p10": round(nb / float(np.percentile(times, 90)), 2),
                                       "median": round(nb / float(np.median(times)), 2), "p90": round(nb / float(np.percentile(times, 10)), 2),
                                       "max": round(nb / min(times), 2)},
               "sample": f"{len(times)} steps of batch {nb} (512x512x3), torch-CPU fp32 forward + loss + autograd backward + Adam; "
                         f"value = median step, {el:.1f} s in all"}
    else:                                                         # "latency": predict.py:73-78 on the CPU stand-in
        res = {**pin}
        for side in (512, 1024):
            w = onet.init_weights(1, 1, 0)
            tw = otorch.to_torch_weights(w, torch.float32)
            x = torch.zeros((1, side, side, 1), dtype=torch.float32)

            def once():
                t0 = time.perf_counter()
                with torch.no_grad():
                    otorch.forward(x, tw)
                return (time.perf_counter() - t0) * 1e3
            once()                                                # the one warm-up predict of predict.py:74
            first = once()                                        # the timed predict of predict.py:75-77
            more = [once() for _ in range(9)]
            res[f"grey_{side}_ms"] = round(first, 2)
            res[f"grey_{side}_ms_median_of_10"] = round(float(np.median([first] + more)), 2)
    print("CPU_CHILD_JSON " + json.dumps(res), flush=True)


def run_cpu_child(kind, seconds, n_threads):
    """Parent side: start the child, return its JSON (or an error record -- the GPU numbers must not be lost to it)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-child", kind, "--cpu-seconds", str(seconds), "--cpu-threads", str(n_threads)]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        env.pop(k, None)
    env["HIP_VISIBLE_DEVICES"] = ""                              # the child is CPU only
    try:
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=max(120.0, 20 * seconds))
        for ln in out.stdout.splitlines():
            if ln.startswith("CPU_CHILD_JSON "):
                return json.loads(ln[len("CPU_CHILD_JSON "):])
        return {"error": (out.stderr or out.stdout)[-400:]}
    except subprocess.TimeoutExpired:
        return {"error": "cpu baseline child timed out"}


# ------------------------------------------------------------------------------------------------ N-rank launch
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N ranks (torch.distributed.run, one per GPU) as a child
    process tree and relay rank 0's JSON line.  Runs before anything in this process has touched the GPU
    (torch.cuda.device_count() does not initialise it on this image); nothing is exec'ed."""
    n = args.gpus
    if not args.dry_run:
        have = torch.cuda.device_count()
        if have < n:
            print(f"bench.py: --gpus {n} requested but only {have} GPU(s) visible; refusing to run fewer ranks than asked", file=sys.stderr)
            return 3
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line, flush=True)                                   # rank 0's line is relayed even when a later leg failed (the reason is in it)
    if proc.returncode != 0 or line is None:
        print(f"bench.py: the {n}-rank run failed (exit code {proc.returncode})", file=sys.stderr)
        return proc.returncode or 4
    return 0


def agree_on_native_comm(dist, device, attach, detach, rank):
    """Every rank tries to create the C-ABI RCCL communicator (`attach`); the MIN over ranks of the outcome decides for ALL of
    them.  If any rank failed, every rank drops what it created (`detach`: ubd_comm_destroy, so that no rank issues collectives
    inside ubd_train_step that the others never join) and the caller falls back to torch.distributed's all-reduce.
    Returns True when the native communicator is in use on every rank."""
    ok = 1
    try:
        attach()
    except Exception as e:                               # noqa: BLE001 -- reported, then decided collectively
        ok = 0
        sys.stderr.write(f"[bench] rank {rank}: native RCCL communicator unavailable ({e}); torch.distributed all-reduce instead\n")
    flag = torch.tensor([ok], dtype=torch.int32, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) == 0:
        detach()
        return False
    return True


def guarded_dp_leg(dist, line, leg, timeout_s):
    """Runs the data-parallel train leg `leg()` (configs[3]) behind a watchdog.  The headline figures in `line` (rank 0; None
    elsewhere) are complete before this is called and must not be lost to a stalled exchange: if the leg has not finished
    within `timeout_s` on a rank, that rank prints the line with the reason in `train_step` (rank 0) and leaves with exit code
    6 WITHOUT the (possibly stuck) teardown.  Exactly one of the watchdog and the main path prints.  Returns the exit code of
    the normal path: 0, or 6 when the leg raised."""
    import threading
    final = threading.Lock()                             # whoever takes it first prints; never both

    def give_up():
        if not final.acquire(blocking=False):
            return                                       # the main path is already printing the complete line
        if line is not None:
            out_line = dict(line)
            out_line["train_step"] = {"error": f"data-parallel train leg did not finish within {timeout_s:.0f} s; skipped"}
            print(json.dumps(out_line), flush=True)
        os._exit(6)                                      # the headline line is out; the run as a whole did NOT succeed

    dog = threading.Timer(timeout_s, give_up)
    dog.daemon = True
    dog.start()
    failed = 0
    try:
        res = leg()
    except Exception as e:                               # noqa: BLE001 -- reported in the JSON line
        res = {"error": f"data-parallel train leg failed: {e}"}
        failed = 1
    dist.barrier()                                       # still under the watchdog: a rank that failed leaves the others in a collective
    if not final.acquire(blocking=False):
        time.sleep(3600)                                 # the watchdog fired a moment ago: it prints and ends the process
    dog.cancel()
    if line is not None:
        line["train_step"] = res
        print(json.dumps(line), flush=True)
    return 6 if failed else 0


def dry_run(args, world, rank):
    """CPU/gloo walk through the N-rank contract: init, count the connected ranks, barrier-bracketed timing of K steps,
    MAX over ranks, one JSON line from rank 0.  No GPU work, value is meaningless."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    ones = torch.ones(1)
    dist.all_reduce(ones)
    n_ranks = int(ones.item())
    x = torch.rand(64, 64)

    def step():
        return (x @ x).sum()
    for _ in range(args.warmup):
        step()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    g = torch.full((8,), float(rank + 1))
    dist.all_reduce(g)                                            # stands for the flat-gradient all-reduce
    ok = n_ranks == args.gpus and float(g[0]) == world * (world + 1) / 2
    line = None
    if rank == 0:
        line = {"metric": "images/sec (512x512) fwd+CCL", "value": round(world * BATCH * args.steps / float(t), 1), "unit": "images/s",
                "n_gpus": world, "n_ranks_rccl": n_ranks, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(float(t) / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": "f32", "data": "synthetic", "dry_run": True,
                "config": {"workload": "DRY RUN on CPU/gloo: launch + collective plumbing only, no GPU work"}}
    if world > 1 and args.full:
        # the N > 1 train leg's control flow with a stubbed trainer (UBD_BENCH_DRY_FAULT injects the failures it must survive):
        #   attach_fail -- the last rank cannot create its native communicator: ALL ranks must drop theirs and fall back together
        #   stall       -- the last rank never arrives: the watchdog prints the line with the reason and the run exits non-zero
        #   leg_fail    -- the leg raises on the last rank: line printed with that rank's... rank 0's result, exit code non-zero there
        fault = os.environ.get("UBD_BENCH_DRY_FAULT", "")
        last = rank == world - 1
        state = {"native": False}

        def attach():
            if fault == "attach_fail" and last:
                raise RuntimeError("injected: no communicator on this rank")
            state["native"] = True

        def detach():
            state["native"] = False

        def leg():
            native = agree_on_native_comm(dist, None, attach, detach, rank)
            assert native == state["native"]             # a rank that attached but lost the vote has been detached
            if fault == "stall" and last:
                time.sleep(3600)
            if fault == "leg_fail" and last:
                raise RuntimeError("injected: train leg failed on this rank")
            gg = torch.full((8,), float(rank + 1))
            dist.all_reduce(gg)                          # the (stub) exchange step of every train step
            return {"parallelism": "native communicator" if native else "torch.distributed fallback", "grad_sum": float(gg[0]),
                    "batch_per_gpu": args.train_batch, "global_batch": args.train_batch * world}

        rc = guarded_dp_leg(dist, line, leg, float(os.environ.get("UBD_BENCH_TRAIN_TIMEOUT_S", "240")))
        dist.destroy_process_group()
        return rc if ok else 5
    if line is not None:
        print(json.dumps(line), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 5


def main():
    args = parse()
    if args.cpu_child:
        cpu_child(args.cpu_child, args.cpu_seconds, args.cpu_threads)
        return 0
    launched = "WORLD_SIZE" in os.environ
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus is None:
        args.gpus = world
    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        return 2
    if not launched and args.gpus > 1:
        return launch_ranks(args)                                 # parent of the N ranks: never touches the GPU
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks", file=sys.stderr)
        return 2
    if args.dry_run:
        return dry_run(args, world, rank)
    n_ranks_rccl = 1
    if world > 1 or os.environ.get("UBD_BENCH_FORCE_DIST") == "1":      # the second: one-rank check of the RCCL path
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if torch.cuda.device_count() <= local_rank:
            print(f"bench.py: rank {rank} has no GPU (local rank {local_rank}, {torch.cuda.device_count()} visible)", file=sys.stderr)
            return 3
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        ones = torch.ones(1, device=f"cuda:{local_rank}")
        dist.all_reduce(ones)                                     # how many ranks did RCCL really connect?
        n_ranks_rccl = int(ones.item())
        if n_ranks_rccl != args.gpus:
            print(f"bench.py: RCCL connected {n_ranks_rccl} ranks, --gpus asked for {args.gpus}", file=sys.stderr)
            return 5
    else:
        dist = None
        torch.cuda.set_device(0)
    dev = torch.device(f"cuda:{torch.cuda.current_device()}")

    from ubdvss_amd import NetConfig, Model, ModelRunner, Trainer, Adam, synthetic, _lib
    cfg = NetConfig(grey=False)
    model = Model(cfg, seed=1)                               # glorot-uniform random init, zero biases
    runner = ModelRunner(cfg, pixel_threshold=0.5, max_objects_per_image=1024, pipelined=True)

    # synthetic batch resident in HBM: stripe-textured rectangles on noise
    # The timed loops walk a RING of distinct input batches (RING x 100.7 MB > the 256 MB Infinity Cache), so a step reads its
    # images from HBM like a real stream of fresh batches would; the figure for ONE re-fed tensor is reported beside it.
    ring_labels = [synthetic.rectangle_maps(3 + rank + 101 * k, BATCH, SIDE // 4, SIDE // 4) for k in range(RING)]
    xs = [torch.from_numpy(synthetic.textured_images(4 + rank + 101 * k, ring_labels[k], 4, C_IN).astype(np.float32) / 127.5 - 1.0).to(dev)
          for k in range(RING)]
    labels, x = ring_labels[0], xs[0]
    input_ring_mb = round(sum(t.numel() * t.element_size() for t in xs) / 1e6, 1)
    step_no = [0]

    def step():
        step_no[0] += 1
        return runner.predict_on_device(model, xs[step_no[0] % RING])

    def timed_wall(fn, k):
        """K calls of fn between barrier + synchronize brackets, wall clock, MAX over ranks -> seconds."""
        sync_all()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        sync_all()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    def sync_all():
        runner.flush()                                            # pipelined runner: the last batch's postprocess is still owed
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # The chip needs a few hundred back-to-back steps after an idle gap before its clocks settle (20 steps: 0.54-0.60 ms,
    # 500: 0.50 ms per step): untimed settle steps in front of the W warm-up steps keep `value` independent
    # of the K / W the caller picks.  Reported as "clock_settle_steps".
    settle = max(0, SETTLE_STEPS - args.warmup)
    for _ in range(settle):
        step()
    for _ in range(args.warmup):
        step()
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    sync_all()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # `ms_per_step` / `value` come from exactly the K timed steps above
    ms_per_step = elapsed / args.steps * 1e3
    value = world * BATCH / (ms_per_step * 1e-3)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)                      # before anything else reuses the runner's result slots
    line = None
    if rank == 0:
        line = {
            "metric": "images/sec (512x512) fwd+CCL", "value": round(value, 1), "unit": "images/s",
            "n_gpus": world, "n_ranks_rccl": n_ranks_rccl, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "clock_settle_steps": settle, "input_ring_MB": input_ring_mb,
            "config": {"workload": "configs[1]: batch=32 512x512x3 fp32 forward + CCL postprocess per GPU "
                                   "(stripe-textured rectangle images, random-init weights)",
                       "batch_per_gpu": BATCH, "image": [SIDE, SIDE, C_IN], "parallelism": f"replicas x{world}, no collective"}}
    if not args.full:
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        if line is not None:
            print(json.dumps(line), flush=True)
        return 0

    # ---- --full only: everything below is reported beside the headline and never changes it
    # The timed region of K steps can be short (20 steps = 7 ms): five more blocks of K steps follow, each with the same brackets
    # (barrier + synchronize on both sides, MAX over ranks); their spread and the median of all six blocks are reported.
    block_ms = [timed_wall(step, args.steps) / args.steps * 1e3 for _ in range(5)]
    # the same step re-fed ONE tensor (rounds 1-3 measured this): x + activations fit the Infinity Cache, the images come from MALL
    single_ms = timed_wall(lambda: runner.predict_on_device(model, x), args.steps) / args.steps * 1e3
    rect_logits = [torch.from_numpy(synthetic.logits_from_maps(ring_labels[k], 0, seed=5 + k)).to(dev) for k in range(2)]
    # the same pipelined step with the in-stem postprocess job fed RECTANGLE maps (1-8 objects per map) instead of
    # the previous batch's logits (random-init weights: one blob per image): forward(batch k) + postprocess(rectangle maps) enqueued
    # together through ubd_forward_postprocess, exactly as the runner does
    runner.flush()
    rect_out = [model.alloc_postprocess_outputs(BATCH, SIDE // 4, SIDE // 4, 1024) for _ in range(2)]
    rect_dst = torch.empty((BATCH, SIDE // 4, SIDE // 4, model.k_out), dtype=torch.float32, device=dev)

    def rect_step():
        step_no[0] += 1
        k = step_no[0] & 1
        job = {"logits": rect_logits[k], "logit_threshold": runner.logit_threshold, "scale": 4, "min_area": cfg.get_min_pixels_for_detection(),
               "cap": 1024, "outputs": rect_out[k]}
        model.predict_on_device(xs[step_no[0] % RING], out=rect_dst, postprocess=job)

    for _ in range(50):
        rect_step()
    rect_ms = timed_wall(rect_step, args.steps) / args.steps * 1e3
    rect_counts = rect_out[0][3].cpu().numpy()
    # ... and with MANY objects per map: a jittered 8 x 8 grid of small rotated rectangles, ~50 separate objects per image
    many_maps = [synthetic.crowded_maps(900 + rank + k, BATCH, SIDE // 4, SIDE // 4) for k in range(2)]
    many_logits = [torch.from_numpy(synthetic.logits_from_maps(many_maps[k], 0, seed=15 + k)).to(dev) for k in range(2)]

    def many_step():
        step_no[0] += 1
        k = step_no[0] & 1
        job = {"logits": many_logits[k], "logit_threshold": runner.logit_threshold, "scale": 4, "min_area": cfg.get_min_pixels_for_detection(),
               "cap": 1024, "outputs": rect_out[k]}
        model.predict_on_device(xs[step_no[0] % RING], out=rect_dst, postprocess=job)

    for _ in range(50):
        many_step()
    many_ms = timed_wall(many_step, args.steps) / args.steps * 1e3
    many_counts = rect_out[0][3].cpu().numpy()

    # ---- extra: train step (fwd + loss + bwd + gradient all-reduce + Adam), batch/GPU = --train-batch:
    #      configs[2] / configs[3] name bf16 activations (fp32 master weights, fp32 accumulation); the fp32
    #      variant is measured beside it
    def time_train(dtype, n_cls=0):
        tb = args.train_batch
        tlabels = [synthetic.rectangle_maps(30 + rank + 101 * k, tb, SIDE // 4, SIDE // 4, n_classes=n_cls) for k in range(RING)]
        txs = [torch.from_numpy(synthetic.textured_images(31 + rank + 101 * k, tlabels[k], 4, C_IN).astype(np.float32) / 127.5 - 1.0).to(dev)
               for k in range(RING)]
        tys = [torch.from_numpy(t).to(dev) for t in tlabels]
        tno = [0]

        def tstep():
            tno[0] += 1
            trainer.train_step_on_device(txs[tno[0] % RING], tys[tno[0] % RING])
        tcfg = cfg if n_cls == 0 else NetConfig(class_names=[f"class{i}" for i in range(n_cls)], grey=False)
        tmodel = Model(tcfg, dtype=dtype, seed=1)
        comm_kind = "single GPU"
        if dist is not None:
            # the handle's own RCCL communicator (include/ubd.h ubd_comm_*): the gradient all-reduce runs inside ubd_train_step,
            # the dilated + head segment on a communication stream under the stem layers' backward pass.  Every rank must take
            # the same path: a rank whose communicator cannot be created makes all of them fall back to torch.distributed's
            # all-reduce of the flat gradient vector (same arithmetic, one more launch) instead of losing the bench line.
            from ubdvss_amd import distributed as ubd_dist
            if agree_on_native_comm(dist, dev, lambda: ubd_dist.attach_native_comm(tmodel, fused=True),
                                    lambda: ubd_dist.detach_native_comm(tmodel), rank):
                comm_kind = (f"dp{world}: per-replica loss, flat-gradient all-reduce per step through the C-ABI RCCL communicator, "
                             f"fused into the train step under the stem backward")
            else:
                comm_kind = f"dp{world}: per-replica loss, flat-gradient all-reduce per step through torch.distributed (RCCL)"
        trainer = Trainer(tmodel, Adam(lr=1e-3))
        trainer.broadcast_weights()
        for _ in range(max(1, args.warmup) + max(0, SETTLE_STEPS - args.warmup)):
            tstep()
        tel = timed_wall(tstep, args.steps)
        tel_single = timed_wall(lambda: trainer.train_step_on_device(txs[0], tys[0]), args.steps)
        params_agree = None
        if dist is not None:
            # data-parallel replicas apply the SAME summed gradient to the same weights: after the timed steps every rank must hold
            # bit-identical parameters -- a lost or half-summed all-reduce segment (an ordering bug between the communication
            # stream and the step's stream) makes the replicas drift apart.  min == max of a checksum over the ranks; checked, not timed.
            cs = tmodel.params.double().sum().reshape(1)
            absum = tmodel.params.double().abs().sum().reshape(1)
            lo, hi, lo2, hi2 = cs.clone(), cs.clone(), absum.clone(), absum.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            dist.all_reduce(lo2, op=dist.ReduceOp.MIN); dist.all_reduce(hi2, op=dist.ReduceOp.MAX)
            params_agree = bool(float(lo) == float(hi) and float(lo2) == float(hi2))
            assert params_agree, f"bench.py: rank {rank}: the replicas' parameters differ after {tno[0]} data-parallel train steps ({float(lo)} .. {float(hi)})"
        bpe = 4.0 if dtype == "float32" else 2.0
        e_fwd = SIDE * SIDE * (C_IN + 45 + (1 + n_cls) / 16.0)                    # E_fwd elements per image
        train_bytes_per_image = (3 * e_fwd - SIDE * SIDE * C_IN) * bpe             # E_train = 3 E_fwd - H W C_in
        res = {"metric": "images/sec (512x512) train step", "value": round(world * tb * args.steps / tel, 1),
               "unit": "images/s", "ms_per_step": round(tel / args.steps * 1e3, 4), "batch_per_gpu": tb, "global_batch": tb * world,
               "dtype": {"float32": "f32", "bfloat16": "bf16"}[dtype], "n_classes": n_cls,
               "parallelism": comm_kind, "replica_parameters_identical_after_the_steps": params_agree,
               "loss_last": round(float(trainer.loss[0]), 5),
               "hbm_frac_algorithmic": round(tb * train_bytes_per_image / (tel / args.steps) / 1e9 / PEAK_HBM, 4),
               "input_ring_MB": round(sum(t.numel() * t.element_size() for t in txs) / 1e6, 1),
               "ms_per_step_single_tensor": round(tel_single / args.steps * 1e3, 4), "clock_settle_steps": max(0, SETTLE_STEPS - args.warmup)}
        del trainer, tmodel, txs, tys
        torch.cuda.empty_cache()
        return res

    train = train_f32 = train_cls8 = None
    if not args.no_train and world == 1 and dist is None:
        train = time_train("bfloat16")                     # configs[2]
        train_cls8 = time_train("bfloat16", n_cls=8)       # configs[2], second run: 8 classes (labels 1..8), detection + classification loss
        train_f32 = time_train("float32")
    # N > 1: the data-parallel train leg (configs[3]: 64 images per GPU, gradient all-reduce) runs LAST, behind a watchdog -- see below

    # ---- extra: configs[4], batch 8 of 1024x1024x3, fp16 activations, forward only ("HBM-bound roofline run")
    def time_cfg5():
        n5, side5 = 8, 1024
        m5 = Model(cfg, dtype="float16", seed=1)
        x5s = [torch.from_numpy(synthetic.noise_images(7 + rank + 101 * k, n5, side5, side5, C_IN)).to(dev) for k in range(RING)]
        no5 = [0]

        def step5():
            no5[0] += 1
            m5.predict_on_device(x5s[no5[0] % RING])

        reps5 = max(5, min(args.steps, 200))
        ms = timed_events(step5, reps5)                    # clock settle inside, like every leg
        ms_single = timed_events(lambda: m5.predict_on_device(x5s[0]), reps5, settle=50)
        # E_fwd = H W (C_in + 45 + K/16) elements of 2 bytes = 100.79 MB per image -- the figure `frac` is quoted on.
        # The image is FED as fp32 here (12.6 MB instead of 6.3 MB per image): the bytes actually moved are given beside it.
        bytes_img = side5 * side5 * (C_IN + 45 + 1 / 16.0) * 2.0
        bytes_img_fed = side5 * side5 * C_IN * 4.0 + side5 * side5 * 45.0 * 2.0 + (side5 // 4) ** 2 * 4.0
        res = {"workload": "configs[4]: batch=8 1024x1024x3 fp16 forward, dilations {1,2,4,8,16,1}", "ms_per_batch": round(ms, 4),
               "images_per_s": round(n5 / ms * 1e3, 1), "dtype": "f16", "clock_settle_steps": SETTLE_STEPS,
               "input_ring_MB": round(sum(t.numel() * t.element_size() for t in x5s) / 1e6, 1), "ms_per_batch_single_tensor": round(ms_single, 4),
               "roofline": {"bound": "hbm", "achieved": round(n5 * bytes_img / (ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM, "unit": "GB/s",
                            "frac": round(n5 * bytes_img / (ms * 1e-3) / 1e9 / PEAK_HBM, 4),
                            "note": "algorithmic bytes per SURVEY 8(d): 100.79 MB per image (every element 2 bytes)",
                            "frac_with_fp32_image_and_logits_as_fed": round(n5 * bytes_img_fed / (ms * 1e-3) / 1e9 / PEAK_HBM, 4)}}
        del m5, x5s
        torch.cuda.empty_cache()
        return res

    cfg5 = None
    if not args.no_train and world == 1:
        cfg5 = time_cfg5()

    # ---- extra: the reference's own metric (predict.py:73-78; README_RU.md:9-10): ONE predict of zeros (1,S,S,1) (grey
    #      model), timed with the wall clock after ONE warm-up predict -- numpy in, numpy out, like keras Model.predict
    def time_latency():
        gcfg = NetConfig(grey=True)
        gm = Model(gcfg, seed=1)
        res = {"protocol": "predict.py:73-78: model.predict(zeros(1,S,S,1)) once as warm-up, second call timed with time.time(); "
                           "numpy in / numpy out (H2D + D2H included; static input / output tensors, seven launches: one stem kernel of cold-started tiles + six dilated layers); "
                           "*_on_device = the image resident in HBM, the pass replayed as ONE captured HIP graph (Model.graphed_forward); *_launch_by_launch = the same seven launches issued one by one",
               "reference_claim_ms": {"512": 50, "1024": 150, "source": "README_RU.md:9-10, 'cpu (4 cores)', unverified"}}
        for side in (512, 1024):
            xz = np.zeros((1, side, side, 1), np.float32)
            xs_ = torch.from_numpy(xz).to(dev)
            for _ in range(SETTLE_STEPS):                             # clock settle (every leg gets it); then the reference's protocol
                gm.predict_on_device(xs_)
            gm.predict(xz)
            torch.cuda.synchronize()
            t0 = time.time(); gm.predict(xz); first = (time.time() - t0) * 1e3
            more = []
            for _ in range(19):
                t0 = time.time(); gm.predict(xz); more.append((time.time() - t0) * 1e3)
            xd = torch.from_numpy(xz).to(dev)
            gm.predict_on_device(xd); torch.cuda.synchronize()
            launches = []                                                  # the seven launches issued one by one
            for _ in range(20):
                t0 = time.time(); gm.predict_on_device(xd); torch.cuda.synchronize(); launches.append((time.time() - t0) * 1e3)
            gf = gm.graphed_forward(1, side, side)                       # the same launches replayed as ONE captured graph
            gf(xd); torch.cuda.synchronize()
            same = bool(torch.equal(gf(xd), gm.predict_on_device(xd)))
            dts = []
            for _ in range(20):
                t0 = time.time(); gf(xd); torch.cuda.synchronize(); dts.append((time.time() - t0) * 1e3)
            res[f"grey_{side}"] = {"latency_ms_batch1": round(first, 4), "median_of_20_ms": round(float(np.median([first] + more)), 4),
                                   "on_device_median_of_20_ms": round(float(np.median(dts)), 4),
                                   "on_device_launch_by_launch_median_of_20_ms": round(float(np.median(launches)), 4),
                                   "graph_bit_equal_to_launches": same}
        del gm
        return res

    latency = time_latency() if (world == 1 and rank == 0) else None

    # ---- extra: the PCIe-inclusive rate -- ModelRunner.predict with HOST numpy input (the reference's calling convention,
    #      model_runner.py:105-138): H2D of the batch, forward, device postprocess, D2H of maps / logits / lists, python lists
    #      of ObjectMarkup.  Never `value` (the bench contract times HBM-resident input); reported so that it is measured.

    def time_host_path():
        """The reference's real seam, PCIe included (model_runner.py:60-67: ModelRunner.predict batch after batch, numpy in, python object
        lists out): per-batch ``predict`` (synchronous pageable copies) and ``predict_stream`` (pinned staging ring, copy-in / compute /
        copy-out streams, the postprocess of batch k inside the stem kernel of batch k + 1).  Never the headline value."""
        res = {"protocol": "numpy batches of 32 x 512 x 512 x 3 (4 distinct arrays in turn, 1-8 objects per image) -> (maps, class logits, object lists); wall clock; "
                           "predict: median of 8 calls after 2 warm-up calls; predict_stream: the median of five pipelines of 48 batches after four untimed 24-batch runs (steady state of a streaming job); stream_thread_ms: consumer thread's wait_staged / enqueue / deliver (of which deliver_wait blocked on the device) and the staging thread's copy",
               "pcie_note": "uint8: 25.2 MB per batch = 0.49 ms at the ~51 GB/s this link sustains (63 GB/s spec) -> <= 65 k img/s; "
                            "float32: 100.7 MB = 1.97 ms -> <= 16.2 k img/s: the float32 stream runs AT the link rate"}
        hr = ModelRunner(cfg, pixel_threshold=0.5, max_objects_per_image=1024)
        x_u8 = [synthetic.textured_images(4 + rank + 7 * k, labels, 4, C_IN) for k in range(4)]
        from ubdvss_amd import PreprocessingType
        # uint8 pixels take the reference's preprocessing (net.py:217-218) fused into the first layer -- raw 0..255 values through
        # random weights give noise maps with hundreds of specks per image, and the leg would time the building of their python objects
        model_u8 = Model(NetConfig(grey=False, preprocessing=PreprocessingType.MOBILENET_LIKE), seed=1)
        model_u8.set_weights(model.get_weights())
        for name, arrs, mdl in (("uint8", x_u8, model_u8), ("float32", [a.astype(np.float32) / 127.5 - 1.0 for a in x_u8], model)):
            for _ in range(2):
                hr.predict(mdl, arrs[0])
            ts = []
            for k in range(8):
                t0 = time.perf_counter(); last = hr.predict(mdl, arrs[k % 4]); ts.append(time.perf_counter() - t0)
            med = float(np.median(ts))
            for _ in range(4):                           # a streaming job's steady state: the first ~100 batches of a process run up to 3 x slower (staging buffers, clocks)
                list(hr.predict_stream(mdl, [arrs[k % 4] for k in range(24)]))
            nb = 48
            runs = []                                    # five pipelines of 48 batches; the median one is reported (the host side shares a 16-CPU quota with whatever else runs on the box)
            for _ in range(5):
                t0 = time.perf_counter()
                n_out = sum(1 for _ in hr.predict_stream(mdl, (arrs[k % 4] for k in range(nb))))
                runs.append(((time.perf_counter() - t0) / nb, dict(hr.last_stream_stats)))
                assert n_out == nb
            runs.sort(key=lambda r: r[0])
            per, stream_stats = runs[2]
            res[name] = {"ms_per_batch": round(med * 1e3, 3), "images_per_s": round(BATCH / med, 1), "h2d_MB": round(arrs[0].nbytes / 1e6, 1),
                         "stream_ms_per_batch": round(per * 1e3, 3), "stream_images_per_s": round(BATCH / per, 1),
                         "stream_host_to_device_GBps": round(arrs[0].nbytes / per / 1e9, 1), "objects_per_image_mean": round(float(np.mean([len(o) for o in last[2]])), 2),
                         "stream_images_per_s_five_runs": [round(BATCH / r[0], 1) for r in runs],
                         "stream_thread_ms_per_batch": {k[:-2]: round(v / nb * 1e3, 3) for k, v in stream_stats.items() if k.endswith("_s")}}
        return res



    host_path = time_host_path() if (world == 1 and rank == 0) else None

    if rank == 0:
        # ---- parts: net only / postprocess only (rectangle maps) -- HIP events on the launch stream
        timed = timed_events                                  # SETTLE_STEPS untimed calls in front of every timed region
        reps = max(5, min(args.steps, 200))
        net_no = [0]

        def net_step():
            net_no[0] += 1
            model.predict_on_device(xs[net_no[0] % RING])

        net_ms = timed(net_step, reps)
        net_single_ms = timed(lambda: model.predict_on_device(x), reps, settle=50)
        logits = model.predict_on_device(x)
        post_ms = timed(lambda: model.postprocess_on_device(logits, runner.logit_threshold, 4, 5, cap=1024), reps)
        post_rect_ms = timed(lambda: model.postprocess_on_device(rect_logits[0], runner.logit_threshold, 4, 5, cap=1024), reps)
        counts = out[4].cpu().numpy()

        # ---- roofline of the dominant kernel: one dense dilated layer on the real L3 activations
        lib = _lib.load()
        n, mh, mw = BATCH, SIDE // 4, SIDE // 4
        act_in = torch.rand((n, mh, mw, 24), device=dev) - 0.3
        act_out = torch.empty_like(act_in)
        ws = torch.empty(int(lib.ubd_forward_workspace_bytes(model._h, 1, 4, 4)), dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.ubd_pack_weights(model._h, model.params.data_ptr(), ws.data_ptr(), ws.numel(), stream), "pack")
        layer_ms = []
        for layer in range(6):
            layer_ms.append(timed(lambda: _lib.check(lib.ubd_dilated_layer(
                model._h, model.params.data_ptr(), layer, act_in.data_ptr(), act_out.data_ptr(), n, mh, mw,
                ws.data_ptr(), stream), "dil"), reps))
        t_layer = float(np.mean(layer_ms)) * 1e-3
        flop_layer = 2.0 * 216 * 24 * n * mh * mw
        bytes_layer = 2.0 * n * mh * mw * 24 * 4
        # HBM traffic per launch and the kernel's average duration in the rocprofv3 summary: NOT measured in this run -- parsed
        # from the newest committed profile set and labelled with its files and with whether those profiles were taken on the
        # kernel sources this library was built from
        traffic, profile_avg_us, profile_files, profile_fresh = committed_profile("void dilconv_wino6_kernel<0")
        # what the matrix pipe is actually given: 192 v_mfma_f32_16x16x32_bf16 per group of 16 tiles (16 points x 2 N tiles x 6 split products)
        groups = n * (mh // 2) * (mw // 32)
        issued_bf16_flop = groups * 192 * 2.0 * 16 * 16 * 32
        roofline = {"bound": "mfma", "kernel": "dilconv_wino6_kernel<0> (Winograd F(2x2,3x3) on the dilation sub-grids; every fp32 product of the 16 transform-domain GEMMs "
                                               "as an EXACT three-way bf16 split: 6 v_mfma_f32_16x16x32_bf16 with fp32 accumulation per fp32 MFMA step, results of fp32 "
                                               "quality (1.7e-7 of max|y| against fp64); `achieved` counts the FLOPs of the direct fp32 convolution against the fp32 "
                                               "matrix peak, `matrix_pipe` what is issued against the bf16 peak)", "achieved": round(flop_layer / t_layer / 1e12, 3),
                    "peak": PEAK_MFMA_F32, "unit": "TFLOP/s", "frac": round(flop_layer / t_layer / 1e12 / PEAK_MFMA_F32, 4),
                    "frac_profile": (round(flop_layer / (profile_avg_us * 1e-6) / 1e12 / PEAK_MFMA_F32, 4) if profile_avg_us else None),
                    "traffic": traffic, "traffic_unit": "MB/launch (PMC FETCH_SIZE x 2 + WRITE_SIZE; algorithmic 100.7 MB)", "avg_launch_us": round(t_layer * 1e6, 2),
                    "profile_avg_us": profile_avg_us,
                    "from_committed_profile": {"fields": ["traffic", "profile_avg_us", "frac_profile"], "files": profile_files,
                                               "taken_on_the_sources_of_this_build": profile_fresh},
                    "clock_settle_launches": SETTLE_STEPS,
                    "per_dilation_us": [round(v * 1e3, 2) for v in layer_ms],
                    "matrix_pipe": {"issued_bf16_tflops": round(issued_bf16_flop / t_layer / 1e12, 1), "peak_bf16_dense": 2500.0,
                                    "frac": round(issued_bf16_flop / t_layer / 1e12 / 2500.0, 4),
                                    "note": "PMC (profiles/r06_pmc_wino6.txt): matrix pipe busy 44 % of the launch, vector ALU 66 %, both together 16 %: the kernel is "
                                            "bound by vector + matrix ISSUE on the SIMD, not by the matrix pipe's rate"},
                    "algorithmic_gbps": round(bytes_layer / t_layer / 1e9, 1)}
        fwd_hbm = {"bound": "hbm", "achieved": round(BATCH * BYTES_PER_IMAGE_FP32 / (net_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM,
                   "unit": "GB/s", "frac": round(BATCH * BYTES_PER_IMAGE_FP32 / (net_ms * 1e-3) / 1e9 / PEAK_HBM, 4),
                   "note": "whole forward pass, algorithmic bytes 50.40 MB/image (SURVEY 8(d))",
                   "mfma_frac": round(BATCH * FLOP_PER_IMAGE / (net_ms * 1e-3) / 1e12 / PEAK_MFMA_F32, 4)}

        cpu = None
        if world == 1 and not args.no_cpu_baseline:
            cpu = run_cpu_child("forward", args.cpu_seconds, args.cpu_threads)
            if train is not None:
                train["cpu_baseline"] = run_cpu_child("train", max(4.0, args.cpu_seconds * 0.75), args.cpu_threads)
            if latency is not None:
                latency["cpu_baseline_4_threads"] = run_cpu_child("latency", 0, 4)

        line.update({
            "ms_per_step_median_of_six_blocks": round(float(np.median([ms_per_step] + block_ms)), 4),
            "ms_per_step_spread": {"blocks_of_K_steps_after_the_timed_one": [round(v, 4) for v in block_ms],
                                   "min": round(min(block_ms), 4), "median": round(float(np.median(block_ms)), 4), "max": round(max(block_ms), 4)},
            "ms_per_step_single_tensor": round(single_ms, 4),
            "ms_per_step_rect_maps": round(rect_ms, 4), "ms_per_step_many_object_maps": round(many_ms, 4),
            "roofline": roofline, "roofline_forward_pass": fwd_hbm, "cpu_baseline": cpu, "train_step": train, "train_step_8_classes": train_cls8, "train_step_f32": train_f32, "forward_fp16_cfg5": cfg5, "latency_batch1": latency, "pcie_inclusive_host_numpy": host_path,
            "parts": {"net_ms": round(net_ms, 4), "net_ms_single_tensor": round(net_single_ms, 4), "postprocess_ms_on_net_maps": round(post_ms, 4),
                      "postprocess_ms_on_rectangle_maps": round(post_rect_ms, 4),
                      "objects_found_mean": float(counts.mean()), "objects_found_max": int(counts.max()),
                      "rect_maps_objects_found_mean": float(rect_counts.mean()), "rect_maps_objects_found_max": int(rect_counts.max()),
                      "many_object_maps_objects_found_mean": float(many_counts.mean()), "many_object_maps_objects_found_max": int(many_counts.max()),
                      "clock_settle_launches": SETTLE_STEPS},
        })
    if dist is not None and not args.no_train:
        # configs[3].  The headline number above must not depend on this leg: if the multi-rank exchange stalls (it cannot be
        # exercised before the run on a one-GPU development box), every rank gives up after TRAIN_DP_TIMEOUT_S, rank 0 prints the
        # line with the reason in place of the train figures, and the processes leave without the (possibly stuck) teardown.
        TRAIN_DP_TIMEOUT_S = float(os.environ.get("UBD_BENCH_TRAIN_TIMEOUT_S", "240"))
        rc = guarded_dp_leg(dist, line, lambda: time_train("bfloat16"), TRAIN_DP_TIMEOUT_S)
        dist.destroy_process_group()
        return rc
    elif dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if line is not None:
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
