#!/usr/bin/env python3
"""Benchmark of the MI355X YOLOv3 hot path (BASELINE.json metric: frames/sec at 608x608).

One "step" = one pass of the whole path over one batch of synthetic frames that start in PINNED HOST
memory: upload of the uint8 BGR frames -> fused preprocess + Darknet-53 convs (HIP MFMA kernels) -> 3 YOLO heads decode ->
threshold/scale/int/tlbr + per-class NMS on device -> padded detection records (for N > 1 ranks ONE RCCL all-gather of
those records per step, on a side stream) -> records back in pinned host memory.  The loop that is timed is the package's
own (yolov3/pipeline.py: Pipeline, three batches in flight), the one `yolov3 --video` and stream.detect_in_frames run.

  python bench.py --gpus N --steps K --warmup W

With N > 1 and no torchrun environment the process starts its N ranks itself (``python -m torch.distributed.run``,
one process per GPU, rendezvous on 127.0.0.1) before anything touches a GPU, relays rank 0's JSON line and exits
non-zero if a rank fails or fewer than N GPUs are visible.  Launched under torchrun it is one rank of the job.

Rank 0 prints ONE JSON line.  `value` = frames of all ranks / max-over-ranks wall time of exactly K steps (PCIe inclusive).
The timed loop runs exactly K steps after max(W, --streams) warm-up steps (--repeats R: R such windows back to back, the median counts).
--dump-outputs DIR then writes the detections the last timed step returned as DIR/<name>.npy (frames and weights are
procedural and seeded: the same arguments give the same inputs, so two builds can be compared output for output).
That is all a plain run does: set up, warm up, time, dump, print.  With --full it also measures and reports, in that line:
  roofline        dominant kernel and per-kernel times (`kernels`), dispatch-bound HIP events on the launch stream
                  (serial passes after --sustain seconds of load; rank 0, at any N)
and at N = 1:
  resident        the same steps with the frames already in HBM and the records left there (the kernels alone; r01-r03's `value`)
  cpu_baseline    the CPU oracle (the reference's "-d cpu" op sequence) on the host cores, SURVEY.md 8(d) protocol
  other_configs   BASELINE.json's other single-GPU configurations (parity cases, each with its own roofline)
  detection_regimes  the headline workload at the reference test's thresholds (0.2 / 0.3) and with ~4000 candidates per frame
                  (the cost of NMS depends on the data)
  bf16_agreement  bf16 detections against the reference's float32 detections on the golden frames (tests/golden)
  f16_agreement   the same for the fp16 storage mode (same kernels on the f16 MFMA; `other_configs` has its rate)
  latency         batch-1 inference() wall time and the package's batched loops
--no-cpu-baseline, --no-extras and --no-latency leave sections out of a --full run.  --dump-ops FILE runs the per-kernel passes
(and reports `roofline` / `kernels`) without --full as well: the table is made from them.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

# RCCL between processes on this driver stack needs dmabuf IPC (already exported on the pool's boxes; kept here so a
# bare environment behaves the same)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# The number of hardware queues HIP maps this process's streams onto (GPU_MAX_HW_QUEUES) is left to the environment: a
# card's queues are shared by every process on it.  The line records what was in effect (`gpu_max_hw_queues`).

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HEAVY_OBJ_BIAS = -6.9          # objectness bias of the procedural weights that leaves ~4000 candidates / frame at threshold 0.05
PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "float32": 157.3}   # MI355X dense MFMA peaks (F16 = BF16 rate)
MODEL_FLOPS_PER_FRAME = {("yolov3", 608): 140.692e9, ("yolov3-tiny", 416): 5.565e9, ("yolov3-spp", 608): 141.449e9}
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r06_traffic.json")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="yolov3")
    ap.add_argument("--dim", type=int, default=608)
    ap.add_argument("--batch", type=int, default=16, help="frames per GPU per step")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "float32"])
    ap.add_argument("--obj-bias", type=float, default=-8.5,
                    help="objectness bias of the procedural weights (sets candidates/frame)")
    ap.add_argument("--kmax", type=int, default=512, help="detection records per frame in the gather")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: per-kernel roofline, and at N = 1 the CPU baseline, the "
                         "resident rate, the other configurations, detection regimes, latency and detection agreement")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-baseline-child", action="store_true", help="(internal) run only the CPU baseline and print its JSON object")
    ap.add_argument("--repeats", type=int, default=1,
                    help="timed windows of --steps steps each, back to back (default 1: exactly --steps timed steps); value / "
                         "ms_per_step = the MEDIAN window, the line carries min / median / max (`repeats`)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the detections the last timed step returned (what "
                         "Pipeline.results hands a caller) as DIR/<name>.npy, float32 / float64 (dump_outputs)")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip resident / other_configs / detection_regimes / latency / agreement (A/B runs, profiling)")
    ap.add_argument("--cpu-budget", type=float, default=30.0, help="seconds of CPU-baseline work (bounded sample)")
    ap.add_argument("--profile-passes", type=int, default=24,
                    help="serial passes of the per-kernel report (median per op), right after --sustain seconds of the timed loop")
    ap.add_argument("--sustain", type=float, default=2.0, help="seconds of sustained load before the per-kernel passes")
    ap.add_argument("--no-latency", action="store_true", help="with --full: skip the batch-1 latency / video-loop section")
    ap.add_argument("--dump-ops", default=None,
                    help="write the per-op timing table (text) to this file (runs the per-kernel passes, with or without --full)")
    ap.add_argument("--streams", type=int, default=3,
                    help="batches in flight per GPU: step i runs on HIP stream i %% streams with its own arena, so "
                         "one batch's kernel tails overlap the next batch's ramp-up (1 = strictly serial steps)")
    ap.add_argument("--resident", action="store_true",
                    help="A/B runs of kernels: time the steps with the frames already in HBM and the records left there "
                         "(not the headline: `value` is PCIe inclusive, frames from pinned host memory, records back to it)")
    ap.add_argument("--h2d", action="store_true", help="(accepted for old command lines: PCIe inclusive is the default now)")
    ap.add_argument("--tuning", default="", help="A/B runs: comma-separated y3_set_tuning knobs, e.g. auto_mask=15")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak [default]: --batch frames per GPU whatever N (BASELINE.json configs[4]: 16 per GPU); strong: "
                         "--total-frames frames per step split over the N GPUs (SURVEY.md 8(d): 128 total)")
    ap.add_argument("--total-frames", type=int, default=128, help="frames per step of the whole job with --scaling strong")
    ap.add_argument("--launch-timeout", type=float, default=1500.0,
                    help="wall-clock limit (s) of the N-rank child job that `--gpus N` starts; on expiry its process group is "
                         "killed and the exit code is 124")
    ap.add_argument("--graph", default="auto", choices=["auto", "0", "1"],
                    help="replay each forward as one captured hipGraph (0.07 instead of ~0.75 ms of host time per step): auto = "
                         "eager on one GPU (the headline is always measured the same way); with N > 1 ranks only when a rank "
                         "has fewer than two usable CPUs.  The line says which (`use_graph`)")
    return ap.parse_args(argv)


def frames_per_rank(args, rank, world):
    """Frames this rank processes per step: --batch (weak scaling) or its contiguous share of --total-frames (strong)."""
    if args.scaling == "weak":
        return args.batch
    from yolov3.dist import shard_range
    lo, hi = shard_range(args.total_frames, rank, world)
    return hi - lo


def usable_cpus():
    """CPUs this process may really use: affinity mask capped by the cgroup CPU quota (the GPU
    boxes expose 256 hardware threads but grant a 16-CPU quota; 256 torch threads would thrash)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            quota, period = fh.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def _read(path, default=None):
    try:
        with open(path) as fh:
            return fh.read().strip()
    except OSError:
        return default


def _parse_cpulist(text):
    cpus = set()
    for part in (text or "").split(","):
        part = part.strip()
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def cpu_topology():
    """{cpu: (numa node, (package, core id))} of the CPUs this process may run on (sysfs; node -1 when unknown)."""
    allowed = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else set(range(os.cpu_count() or 1))
    node_of = {}
    base = "/sys/devices/system/node"
    try:
        for name in os.listdir(base):
            if name.startswith("node") and name[4:].isdigit():
                for c in _parse_cpulist(_read(os.path.join(base, name, "cpulist"))):
                    node_of[c] = int(name[4:])
    except OSError:
        pass
    topo = {}
    for c in allowed:
        t = "/sys/devices/system/cpu/cpu%d/topology/" % c
        topo[c] = (node_of.get(c, -1), (int(_read(t + "physical_package_id", "0") or 0), int(_read(t + "core_id", str(c)) or c)))
    return topo


def _cpu_busy(interval=0.3):
    """Per-CPU busy share over ``interval`` seconds (/proc/stat), {} if unreadable."""
    def snap():
        out = {}
        for ln in (_read("/proc/stat", "") or "").splitlines():
            if ln.startswith("cpu") and ln[3:4].isdigit():
                f = ln.split()
                v = [int(x) for x in f[1:9]]
                out[int(f[0][3:])] = (sum(v), v[3] + v[4])      # total, idle + iowait
        return out
    a = snap()
    time.sleep(interval)
    b = snap()
    return {c: 1.0 - (b[c][1] - a[c][1]) / max(1, b[c][0] - a[c][0]) for c in b if c in a}


def pick_quiet_cpus(n):
    """``n`` CPUs for the CPU baseline: distinct physical cores of ONE NUMA node, dealt ROUND-ROBIN OVER THE NODE'S L3 DOMAINS
    (an EPYC 9575F socket is eight CCDs of eight cores with 32 MB of L3 each: sixteen threads then always get two cores of
    every CCD -- the SAME share of cache and memory links in every run, whichever cores happen to be idle; three consecutive
    runs: 10.3 / 11.2 / 9.5 frames/s, profiles/r05_cpu_baseline.txt), inside a domain the cores that were least busy over the
    last 0.3 s (the pool's hosts are shared: 256 hardware threads, a 16-CPU quota per tenant; rounds 1-4 ran unpinned and read
    2.9 .. 14.9).  Falls back to the first ``n`` allowed CPUs."""
    topo = cpu_topology()
    busy = _cpu_busy()
    cores = {}
    for c, (node, core) in topo.items():
        cores.setdefault((node, core), []).append(c)
    by_node = {}
    for (node, core), cpus in cores.items():
        first = min(cpus)
        l3 = _read("/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list" % first, "all")
        by_node.setdefault(node, {}).setdefault(l3, []).append((max(busy.get(c, 0.0) for c in cpus), first))
    best = None
    for node, domains in by_node.items():
        if sum(len(v) for v in domains.values()) < n:
            continue
        queues = [sorted(v) for _, v in sorted(domains.items(), key=lambda kv: min(c for _, c in kv[1]))]
        picked = []
        while len(picked) < n:
            for q in queues:
                if q and len(picked) < n:
                    picked.append(q.pop(0))
        cost = sum(b for b, _ in picked)
        if best is None or cost < best[0]:
            best = (cost, node, [c for _, c in picked])
    if best is None:
        return sorted(topo)[:n], -1
    return sorted(best[2]), best[1]


def gpu_numa_nodes():
    """NUMA node and PCI address of every GPU in HIP's enumeration order, from sysfs only (NO GPU call: the ranks bind their
    threads before the runtime starts any).  KFD topology nodes with SIMDs are the GPUs, in the order the runtime enumerates
    them; numeric HIP_/ROCR_/CUDA_VISIBLE_DEVICES lists are honoured.  [] when the topology cannot be read."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    gpus = []
    try:
        ids = sorted(int(n) for n in os.listdir(base) if n.isdigit())
    except OSError:
        return []
    for n in ids:
        props = {}
        for ln in (_read(os.path.join(base, str(n), "properties"), "") or "").splitlines():
            k, _, v = ln.partition(" ")
            props[k] = v.strip()
        try:
            if int(props.get("simd_count", "0")) <= 0:
                continue
            loc, dom = int(props.get("location_id", "0")), int(props.get("domain", "0"))
        except ValueError:
            continue
        bdf = "%04x:%02x:%02x.%d" % (dom, (loc >> 8) & 0xFF, (loc >> 3) & 0x1F, loc & 7)
        node = _read("/sys/bus/pci/devices/%s/numa_node" % bdf)
        cpus = _parse_cpulist(_read("/sys/bus/pci/devices/%s/local_cpulist" % bdf))
        gpus.append({"bdf": bdf, "numa_node": int(node) if node not in (None, "") else -1, "local_cpus": cpus})
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        val = os.environ.get(var)
        if val and all(p.strip().isdigit() for p in val.split(",")):
            gpus = [gpus[int(p)] for p in val.split(",") if int(p) < len(gpus)]
    return gpus


def bind_rank_to_gpu_node(local_rank):
    """Before any GPU call: restrict this rank (and every thread it will start: the HIP runtime's, torch's) to the CPUs of its
    GPU's NUMA node, so that pinned frame / record buffers (first touch) and the enqueue thread sit on the socket the GPU hangs
    off.  The headline is PCIe inclusive: on a two-socket node a rank on the wrong socket pulls every frame over the
    inter-socket link.  Returns what it did for the JSON line (``per_rank.placement``)."""
    info = {"numa_node": None, "gpu_bdf": None, "cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
            "bound": False}
    if os.environ.get("Y3_BENCH_NO_BIND") == "1" or not hasattr(os, "sched_setaffinity"):
        return info
    gpus = gpu_numa_nodes()
    if local_rank >= len(gpus):
        return info
    g = gpus[local_rank]
    info["gpu_bdf"], info["numa_node"] = g["bdf"], g["numa_node"]
    allowed = os.sched_getaffinity(0)
    want = g["local_cpus"] & allowed
    if g["numa_node"] >= 0 and not want:
        want = {c for c, (node, _) in cpu_topology().items() if node == g["numa_node"]}
    if want and want != allowed:
        try:
            os.sched_setaffinity(0, want)
            info["bound"] = True
        except OSError:
            pass
    info["cpus"] = len(os.sched_getaffinity(0))
    return info


class GpuTelemetry(object):
    """Shader clock and socket power of ONE GPU, sampled from a side thread while a measurement runs: plain reads of the amdgpu
    hwmon files of the PCI device (``freq1_input`` = sclk in Hz, ``power1_input`` = PPT in microwatts; found with
    tools/smi_probe.py) -- no other program is started, nothing is re-executed.  The MI355X holds ~2.0-2.15 GHz under this
    load at its 1.4 kW cap, not the 2.4 GHz the 2.5 PFLOP/s peak is quoted at (profiles/r05i_power_bf16_vs_fp16.txt), and how
    far it sags differs by box and by what ran in the seconds before: a roofline fraction without the clock it was measured
    at cannot be compared between runs."""

    def __init__(self, bdf, interval=0.002):
        import glob
        self.interval = interval
        self.freq = self.power = None
        for hw in sorted(glob.glob("/sys/bus/pci/devices/%s/hwmon/hwmon*" % bdf)) if bdf else []:
            if os.path.exists(os.path.join(hw, "freq1_input")):
                self.freq = os.path.join(hw, "freq1_input")
            for name in ("power1_input", "power1_average"):
                if self.power is None and os.path.exists(os.path.join(hw, name)):
                    self.power = os.path.join(hw, name)
        self.samples = []
        self._stop = None
        self._thread = None

    @property
    def available(self):
        return self.freq is not None

    def _read(self):
        try:
            f = int(_read(self.freq)) / 1e6 if self.freq else None
            w = int(_read(self.power)) / 1e6 if self.power else None
            return f, w
        except (TypeError, ValueError):
            return None, None

    def __enter__(self):
        import threading
        self.samples = []
        if not self.available:
            return self
        self._stop = threading.Event()

        def loop():
            while not self._stop.is_set():
                self.samples.append(self._read())
                self._stop.wait(self.interval)
        self._thread = threading.Thread(target=loop, daemon=True)
        self._thread.start()
        return self

    def __exit__(self, *exc):
        if self._thread is not None:
            self._stop.set()
            self._thread.join()
            self._thread = None
        return False

    def summary(self):
        """{"sclk_mhz": median, "sclk_mhz_min" / "_max", "power_w": median, "samples": n} of the last ``with`` block."""
        f = [a for a, _ in self.samples if a]
        w = [b for _, b in self.samples if b]
        if not f:
            return {"sclk_mhz": None, "power_w": None, "samples": 0}
        return {"sclk_mhz": round(float(np.median(f)), 1), "sclk_mhz_min": round(min(f), 1), "sclk_mhz_max": round(max(f), 1),
                "power_w": round(float(np.median(w)), 1) if w else None, "samples": len(f)}


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for ln in fh:
                if ln.lower().startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


# ------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` without torchrun
# ------------------------------------------------------------------------------------------------

def _tail(path, n=12):
    try:
        with open(path, errors="replace") as fh:
            return fh.read().splitlines()[-n:]
    except OSError:
        return []


def self_launch(args, argv):
    """Start N ranks as a child torch.distributed.run job.  Runs BEFORE this process has made any GPU call (a
    process that has initialised the GPU must not exec / is not what gets replaced here: the job is a child).
    The parent is the watchdog: the job runs in its own process group under a wall-clock limit (--launch-timeout); on
    expiry the whole group is killed (a rank stuck in RCCL init would otherwise burn the caller's limit); on any failure
    every rank's last stderr lines are printed and the exit code is non-zero.  It only starts and kills children."""
    import shutil
    import signal
    import tempfile
    plumbing = os.environ.get("Y3_BENCH_PLUMBING")
    if not plumbing:
        visible = torch.cuda.device_count()        # counts devices without initialising the GPU runtime
        if visible < args.gpus:
            sys.stderr.write("bench.py: %d GPUs requested, %d visible -- refusing to run fewer ranks than asked for\n" % (
                args.gpus, visible))
            return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    logdir = tempfile.mkdtemp(prefix="y3_bench_ranks_")
    # --tee 3: every rank's stdout / stderr goes to the console AND to <logdir>/.../<rank>/std{out,err}.log
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "--log-dir", logdir, "--tee", "3",
           os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", str(max(1, usable_cpus() // args.gpus)))
    limit = float(os.environ.get("Y3_BENCH_LAUNCH_TIMEOUT", args.launch_timeout))
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                            start_new_session=True)
    timed_out = False
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        timed_out = True
        for sig in (signal.SIGTERM, signal.SIGKILL):       # the whole process group: torchrun, its ranks, their children
            try:
                os.killpg(proc.pid, sig)
            except (ProcessLookupError, PermissionError):
                break
            try:
                out, err = proc.communicate(timeout=10)
                break
            except subprocess.TimeoutExpired:
                continue
        else:
            out, err = proc.communicate()
    # rank 0's JSON line arrives tee'd as "[default0]:{...}"
    lines = []
    for ln in out.splitlines():
        i = ln.find("{")
        if i >= 0 and ln[:i].strip() in ("", "[default0]:") and ln.rstrip().endswith("}"):
            lines.append(ln[i:])
    ok = (not timed_out) and proc.returncode == 0 and len(lines) == 1
    if not ok:
        sys.stderr.write(err[-4000:])
        for root, _, files in sorted(os.walk(logdir)):
            if "stderr.log" in files:
                tail = _tail(os.path.join(root, "stderr.log"))
                sys.stderr.write("\n---- rank %s, last stderr lines ----\n%s\n" % (os.path.basename(root), "\n".join(tail) or "(empty)"))
        if timed_out:
            sys.stderr.write("\nbench.py: the %d-rank job did not finish within %.0f s (--launch-timeout): process group killed\n" % (
                args.gpus, limit))
        else:
            sys.stderr.write("\nbench.py: the %d-rank job failed (exit code %s, %d JSON lines)\n" % (
                args.gpus, proc.returncode, len(lines)))
    shutil.rmtree(logdir, ignore_errors=True)
    if not ok:
        return 124 if timed_out else (proc.returncode or 1)
    print(lines[0], flush=True)
    return 0


def init_group(backend, dev=None):
    """Process group with a BOUNDED rendezvous (a rank that never arrives must not hang the others for the default ten
    minutes), then one real collective: every rank contributes its rank, and the job fails unless ranks 0 .. N-1 are seen."""
    import datetime
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    world = int(os.environ["WORLD_SIZE"])
    timeout = datetime.timedelta(seconds=float(os.environ.get("Y3_BENCH_INIT_TIMEOUT", "180")))
    if dev is not None:
        dist.init_process_group(backend=backend, device_id=dev, timeout=timeout)
    else:
        dist.init_process_group(backend=backend, timeout=timeout)
    mine = torch.tensor([dist.get_rank()], dtype=torch.int64, device=dev if dev is not None else "cpu")
    seen = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(seen, mine)
    seen = sorted(int(t.item()) for t in seen)
    if seen != list(range(world)):
        raise SystemExit("bench.py: the collective saw ranks %s, expected 0 .. %d" % (seen, world - 1))
    return len(seen)


def rank_stats(elapsed, host_enqueue, steps, world, dev):
    """Per-rank wall and host-enqueue time of the timed region, gathered to every rank (one small all_gather AFTER the
    timed region): a slow rank or a rank starved of host cores shows up in the line instead of only in the maximum."""
    import torch.distributed as dist
    mine = torch.tensor([elapsed, host_enqueue], dtype=torch.float64, device=dev if dev is not None else "cpu")
    if world > 1 or (dist.is_available() and dist.is_initialized()):
        allr = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
        dist.all_gather(allr, mine)
        vals = torch.stack(allr).cpu().numpy()
    else:
        vals = mine.cpu().numpy()[None]
    ms = vals[:, 0] / steps * 1e3
    he = vals[:, 1] / steps * 1e3
    return {"ms_per_step_min": round(float(ms.min()), 4), "ms_per_step_max": round(float(ms.max()), 4),
            "ms_per_step_by_rank": [round(float(v), 4) for v in ms],
            "host_enqueue_ms_per_step_max": round(float(he.max()), 4),
            "host_enqueue_ms_per_step_by_rank": [round(float(v), 4) for v in he], "usable_cpus_per_rank": usable_cpus() // max(1, world)}


def plumbing_main(args, backend):
    """Y3_BENCH_PLUMBING=gloo: no GPU work.  The same rank / shard / barrier / one-all-gather-per-step / max-over-ranks
    skeleton as the real run, over gloo on CPU tensors: what tests/test_dist_gloo.py uses to check the launcher."""
    import torch.distributed as dist
    from yolov3.dist import all_gather_records, counts_of, pack_records_host
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if os.environ.get("Y3_BENCH_FAIL_RANK") == str(rank):
        raise SystemExit(3)
    if os.environ.get("Y3_BENCH_HANG_RANK") == str(rank):      # tests: a rank that never reaches the rendezvous
        time.sleep(1e6)
    # (the same pre-GPU placement step as the real run: on a box without a KFD topology it reports "not bound")
    placement = bind_rank_to_gpu_node(int(os.environ.get("LOCAL_RANK", "0")))
    ranks_seen = init_group(backend)
    if os.environ.get("Y3_BENCH_DIE_AFTER_INIT") == str(rank):  # tests: a rank that dies once the group exists
        sys.stderr.write("rank %d: dying after init (test hook)\n" % rank)
        os._exit(5)
    b = frames_per_rank(args, rank, world)
    bmax = max(frames_per_rank(args, r, world) for r in range(world))
    rs = np.random.RandomState(rank)
    dets = []
    for _ in range(bmax):                 # ranks with a smaller share pad with empty frames: one fixed-size collective
        k = int(rs.randint(0, 9)) if len(dets) < b else 0
        dets.append([rs.randint(0, 600, size=(k, 4)), rs.rand(k).astype(np.float32), rs.randint(0, 80, size=k),
                     rs.randint(0, 22743, size=k)])
    rec = torch.from_numpy(pack_records_host(dets, args.kmax))
    for _ in range(args.warmup):
        all_gather_records(rec, world)
    # gloo's own barrier: dist.barrier() asks for the machine's accelerator first, which starts the GPU runtime in every rank
    # of this no-GPU mode
    windows = []                              # R windows of exactly K steps, each between barriers; max over ranks; the median counts
    for _ in range(max(1, args.repeats)):
        dist.monitored_barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = all_gather_records(rec, world)
        host_enqueue = time.perf_counter() - t0
        dist.monitored_barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        windows.append((float(t.item()), host_enqueue))
    order = sorted(range(len(windows)), key=lambda k: windows[k][0])
    elapsed, host_enqueue = windows[order[(len(order) - 1) // 2]]
    stats = rank_stats(elapsed, host_enqueue, args.steps, world, None)
    allp = [None] * world
    dist.all_gather_object(allp, placement)
    stats["placement"] = allp
    if rank == 0:
        total = sum(frames_per_rank(args, r, world) for r in range(world))
        print(json.dumps({"metric": "frames/sec (608x608)", "value": None, "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "plumbing_only": True, "scaling": args.scaling,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 4),
                          "repeats": {"windows": len(windows), "ms_per_step_min": round(min(w[0] for w in windows) / args.steps * 1e3, 4),
                                      "ms_per_step_max": round(max(w[0] for w in windows) / args.steps * 1e3, 4)},
                          "ranks_seen_by_collective": ranks_seen,
                          "frames_gathered_per_step": int(counts_of(out).shape[0]), "per_rank": stats,
                          "config": {"global_batch": total, "frames_per_gpu": [frames_per_rank(args, r, world) for r in range(world)],
                                     "parallelism": "dp%d" % world}}), flush=True)
    dist.monitored_barrier()
    dist.destroy_process_group()
    return 0


# ------------------------------------------------------------------------------------------------
# one workload on this rank's GPU
# ------------------------------------------------------------------------------------------------

class Workload(object):
    """model x input size x batch x dtype on one GPU: net, the package's Pipeline, host (pinned) and resident frames."""

    def __init__(self, model, dim, batch, dtype, params, dev, rank, world, kmax, nstream, options=None, prob_thresh=0.05,
                 nms_iou_thresh=0.3):
        import yolov3
        from yolov3.pipeline import Pipeline
        from yolov3.synthdata import synth_frames
        self.model, self.dim, self.batch, self.dtype, self.dev, self.nstream = model, dim, batch, dtype, dev, nstream
        cfg = os.path.join(ROOT, "pytorch-yolov3_amd", "models", model + ".cfg")
        self.cfg = cfg
        self.net = yolov3.Darknet(cfg, device=str(dev), dtype=dtype).eval()
        self.net.set_params(params)
        # explicit options (hipGraph replay) replace the pipeline's own choice, which is the throughput tile choice
        # (Y3_AM_HALO_TILE256) whenever more than one batch is in flight
        self.prob_thresh = prob_thresh
        self.pipe = Pipeline(self.net, batch, dim, dim, in_flight=nstream, prob_thresh=prob_thresh, nms_iou_thresh=nms_iou_thresh,
                             kmax=kmax, world=world, options=options)
        self.options = self.pipe.options
        self.rows = self.pipe.rows
        self.frames_np = synth_frames(123 + rank, batch, dim, dim)
        # distinct frames per rank (data-parallel shards): in pinned host memory (the headline) and resident in HBM
        self.host_frames = torch.from_numpy(self.frames_np).pin_memory()
        self.host_warm = torch.from_numpy(synth_frames(1000 + rank, batch, dim, dim)).pin_memory()
        self.frames = torch.from_numpy(self.frames_np).to(dev)
        self.warm_frames = self.host_warm.to(dev)
        torch.cuda.synchronize()

    def step(self, i, resident=False, warm=False):
        if resident:
            return self.pipe.submit(self.warm_frames if warm else self.frames, to_host=False)
        return self.pipe.submit(self.host_warm if warm else self.host_frames)

    def timed(self, steps, warmup, distributed=False, resident=False, repeats=1):
        """`warmup` untimed steps, then ``repeats`` back-to-back windows of EXACTLY `steps` steps, each bracketed by barrier +
        synchronize on both sides and reduced to the max over ranks.  Returns the MEDIAN window's time (every rank picks the
        same window: the list is identical on all ranks after the all-reduce); ``self.windows_s`` keeps all of them, and
        ``rank_elapsed_s`` / ``host_enqueue_s`` are those of the median window."""
        import torch.distributed as dist
        for i in range(max(warmup, self.nstream)):
            self.step(i, resident, warm=True)
        torch.cuda.synchronize()
        if os.environ.get("Y3_BENCH_DEBUG_AFTER_WARMUP"):      # diagnostic libraries only (the product library rejects the key)
            from yolov3 import _hip
            _hip.check(_hip.lib().y3_set_tuning(b"debug", int(os.environ["Y3_BENCH_DEBUG_AFTER_WARMUP"])))
        windows, mine = [], []
        for _ in range(max(1, repeats)):
            if distributed:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                self.step(i, resident)
            host_enqueue = time.perf_counter() - t0          # host time to enqueue the K steps (the GPU runs behind it)
            torch.cuda.synchronize()
            rank_elapsed = time.perf_counter() - t0          # this rank alone, before the closing barrier
            if distributed:
                dist.barrier()
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            if distributed:
                t = torch.tensor([elapsed], dtype=torch.float64, device=self.dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                elapsed = float(t.item())
            windows.append(elapsed)
            mine.append((rank_elapsed, host_enqueue))
        order = sorted(range(len(windows)), key=lambda k: windows[k])
        med = order[(len(order) - 1) // 2]                    # lower median: an actually measured window
        self.windows_s = windows
        self.rank_elapsed_s, self.host_enqueue_s = mine[med]
        return windows[med]

    def kept_per_frame(self):
        return int(self.pipe.dets[0].count.cpu().numpy().mean())

    def candidates_per_frame(self):
        """Boxes at or above the probability threshold per frame, before NMS (the detection tail's cost follows this number)."""
        out = self.net.forward_frames(self.frames, fresh=False)
        return int((out["class_prob"] >= self.prob_thresh).sum().item()) // self.batch

    def kernel_report(self, passes, dump_ops=None, telemetry=None, sustain_steps=0):
        """Per-kernel device time, serial passes on the launch stream (inside the timed region several batches overlap and a
        launch's duration would include its neighbours').

        Protocol: ``sustain_steps`` steps of the timed loop itself first (>= 2 s: the chip is at the
        clock it HOLDS under this load, not at the boost clock of a cold start), then at once ``passes`` serial passes
        back to back; per op the MEDIAN over the passes counts (the minimum is carried alongside), and ``telemetry``
        samples sclk / power during the passes.  Two timings per pass type:
          kernel   y3_plan_run_profiled: a start / stop event pair bound to every DISPATCH (hipExtLaunchKernel) -- the
                   kernel's own begin -> end on the device, the figure rocprofv3's kernel trace reports;
          bracket  y3_plan_run_timed: an event recorded on the stream before and after every launch (rounds 1-5) -- that
                   interval also holds the dispatch and the two barrier packets, ~5 us per launch (the whole 52.5 us by
                   rocprofv3 against 57.6-60.6 us by events of round 5: profiles/r06_timing_methods.txt)."""
        net = self.net
        if self.pipe.world > 1 or self.pipe.gathers[0].collective:
            # N ranks: a pipeline step holds a collective (the record all-gather) and this report runs on rank 0 alone -- the
            # sustained load is plain forwards here (one batch in flight instead of three: the same kernels back to back)
            for i in range(sustain_steps):
                net._run(self.frames, "u8", fresh=False, options=self.options)
        else:
            for i in range(sustain_steps):
                self.step(i, resident=True)
        torch.cuda.synchronize()
        kern, brack = [], []
        tel = telemetry if telemetry is not None else GpuTelemetry(None)
        with tel:
            for k in range(passes):
                net._run(self.frames, "u8", timed="kernel", fresh=False, options=self.options)   # the plan the timed steps ran
                kern.append(np.array(net.last_op_ms))
                if k % 3 == 2:
                    net._run(self.frames, "u8", timed=True, fresh=False, options=self.options)
                    brack.append(np.array(net.last_op_ms))
        per_op = np.median(np.stack(kern), axis=0)
        per_op_min = np.min(np.stack(kern), axis=0)
        per_op_brk = np.median(np.stack(brack), axis=0) if brack else per_op
        plan = net.plan_report()
        by_kernel = {}
        for op, ms, ms_min, ms_b in zip(plan, per_op, per_op_min, per_op_brk):
            k = by_kernel.setdefault(op["kernel"], dict(ms=0.0, ms_min=0.0, ms_bracket=0.0, flops=0.0, bytes=0.0, launches=0))
            k["ms"] += float(ms)
            k["ms_min"] += float(ms_min)
            k["ms_bracket"] += float(ms_b)
            k["flops"] += op["flops"]
            k["bytes"] += op["bytes"]
            k["launches"] += 1
        by_kernel.pop("(fused into the previous op)", None)
        if dump_ops:
            desc = net._last_plan.desc["ops"]
            with open(dump_ops, "w") as fh:
                fh.write("%4s %5s %-28s %-34s %9s %9s %9s %9s\n" % ("op", "block", "kernel", "shape", "ms", "TFLOP/s", "GB/s", "bracket"))
                for i, (op, ms, od, mb) in enumerate(zip(plan, per_op, desc, per_op_brk)):
                    ti, to = od["inp"], od.get("out")
                    shape = "%dx%dx%d" % (ti.h, ti.w, ti.c) + ("->%dx%dx%d k%d s%d" % (to.h, to.w, to.c, od.get("ksize", 0), od.get("stride", 0)) if to is not None else "")
                    fh.write("%4d %5d %-28s %-34s %9.4f %9.1f %9.1f %9.4f\n" % (
                        i, op["block"], op["kernel"], shape, ms, op["flops"] / max(ms, 1e-9) / 1e9, op["bytes"] / max(ms, 1e-9) / 1e6, mb))
        dominant = max(by_kernel, key=lambda k: by_kernel[k]["ms"])
        return dict(by_kernel=by_kernel, dominant=dominant, plan_ms=float(per_op.sum()), plan_ms_bracket=float(per_op_brk.sum()),
                    passes=len(kern), bracket_passes=len(brack), sustain_steps=sustain_steps, telemetry=tel.summary())

    def roofline(self, report, traffic_table=None):
        dk = report["by_kernel"][report["dominant"]]
        achieved = dk["flops"] / (dk["ms"] * 1e-3) / 1e12
        peak = PEAK_TFLOPS[self.dtype]
        traffic = rocprof_us = None
        if traffic_table:                                 # per workload: a kernel's mean traffic depends on the layers it runs
            key = "%s_%d_b%d_%s" % (self.model, self.dim, self.batch, self.dtype)
            kern = traffic_table.get("workloads", {}).get(key, {}).get("kernels", {})
            traffic = kern.get(report["dominant"], {}).get("traffic_bytes_per_launch")
            rocprof_us = kern.get(report["dominant"], {}).get("rocprof_avg_us")
        tel = report.get("telemetry") or {}
        sclk = tel.get("sclk_mhz")
        out = {"bound": "mfma", "kernel": report["dominant"], "achieved": round(achieved, 2), "peak": peak,
               "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic,
               "algorithmic_bytes_per_launch": round(dk["bytes"] / dk["launches"]),
               "algorithmic_flops_per_launch": round(dk["flops"] / dk["launches"]),
               "timing": "HIP events bound to every dispatch (hipExtLaunchKernel start / stop: the kernel's own begin -> end, what "
                         "rocprofv3 reports), %d serial passes on the launch stream right after %d steps of sustained load; MEDIAN "
                         "per op" % (report.get("passes", 0), report.get("sustain_steps", 0)),
               "launches_per_step": dk["launches"], "kernel_ms_per_step": round(dk["ms"], 4),
               "avg_us": round(dk["ms"] / dk["launches"] * 1e3, 2), "min_us": round(dk["ms_min"] / dk["launches"] * 1e3, 2),
               "frac_from_min": round(dk["flops"] / (dk["ms_min"] * 1e-3) / 1e12 / peak, 4),
               # the same launches bracketed by two stream events (the method of rounds 1-5): + dispatch / barrier packets
               "event_bracket_avg_us": round(dk["ms_bracket"] / dk["launches"] * 1e3, 2),
               # mean of the same kernel in the committed rocprofv3 kernel trace of this binary (hash-checked like `traffic`)
               "rocprof_avg_us": rocprof_us,
               "sclk_mhz": sclk, "sclk_mhz_range": [tel.get("sclk_mhz_min"), tel.get("sclk_mhz_max")] if sclk else None,
               "power_w": tel.get("power_w"), "telemetry_samples": tel.get("samples", 0),
               # the peak is quoted at 2400 MHz; the chip holds less under this load (power cap): the share of the matrix
               # pipes' rate AT THE CLOCK THEY RAN AT
               "frac_at_held_clock": round(achieved / (peak * sclk / 2400.0), 4) if sclk else None,
               "all_kernels_ms_per_step": round(report["plan_ms"], 4),
               "all_kernels_ms_per_step_event_bracket": round(report["plan_ms_bracket"], 4)}
        return out


DUMP_LIMIT_BYTES = 64 << 20


def last_step_detections(wl, resident):
    """Per-frame ``[tlbr int64 (K, 4), prob float32 (K,), cls int64 (K,)]`` of the last timed step, as a caller of the timed
    path receives them: ``Pipeline.results`` of its ticket (under a process group that is a collective -- every rank calls
    it -- and the frames of all ranks come back in rank order).  With --resident the records stayed on the device: the
    detector of that ticket is read instead (this rank's frames)."""
    last = wl.pipe._n - 1
    if not resident:
        return wl.pipe.results(last)
    torch.cuda.synchronize(wl.dev)
    with torch.cuda.device(wl.dev):
        return wl.pipe.dets[last % wl.pipe.max_open].fetch()


def dump_outputs(out_dir, dets, limit=DUMP_LIMIT_BYTES):
    """Write per-frame detections as flat arrays in the caller's order (frame by frame, within a frame as returned):
      frame.npy (N,) float64            frame index of every detection
      boxes_tlbr.npy (N, 4) float64     integer pixel corners x1, y1, x2, y2
      scores.npy (N,) float32
      classes.npy (N,) float64
      count_per_frame.npy (F,) float64
    Beyond ``limit`` bytes in all, a fixed, seeded sample of the detections is written instead, and sample_index.npy holds
    their positions in the full list.  Returns {name: shape}."""
    counts = np.array([len(d[1]) for d in dets], dtype=np.int64)
    arrays = {
        "frame": np.repeat(np.arange(len(dets)), counts).astype(np.float64),
        "boxes_tlbr": np.concatenate([np.asarray(d[0], dtype=np.int64).reshape(-1, 4) for d in dets]).astype(np.float64),
        "scores": np.concatenate([np.asarray(d[1], dtype=np.float32).reshape(-1) for d in dets]),
        "classes": np.concatenate([np.asarray(d[2], dtype=np.int64).reshape(-1) for d in dets]).astype(np.float64),
    }
    n = int(counts.sum())
    per_detection = sum(a.itemsize * (a.size // max(1, n)) for a in arrays.values()) + 8     # + its sample_index entry
    cap = max(0, (limit - 4096 - 8 * len(dets)) // per_detection)      # 4096: the six .npy headers
    os.makedirs(out_dir, exist_ok=True)
    stale = os.path.join(out_dir, "sample_index.npy")
    if n > cap:
        idx = np.sort(np.random.default_rng(0).choice(n, size=cap, replace=False))
        arrays = {name: a[idx] for name, a in arrays.items()}
        arrays["sample_index"] = idx.astype(np.float64)
    elif os.path.exists(stale):
        os.remove(stale)
    arrays["count_per_frame"] = counts.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def lib_sha256():
    from yolov3 import _hip
    with open(os.path.abspath(_hip.LIB_PATH), "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def _elf_sections(elf):
    """(name, type, bytes) of every section of an ELF64 image."""
    import struct
    shoff = struct.unpack_from("<Q", elf, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    hdrs = [elf[shoff + k * shentsize:shoff + (k + 1) * shentsize] for k in range(shnum)]
    so, ss = struct.unpack_from("<QQ", hdrs[shstrndx], 0x18)
    names = elf[so:so + ss]
    for h in hdrs:
        nm, typ = struct.unpack_from("<II", h, 0)
        off, size = struct.unpack_from("<QQ", h, 0x18)
        yield names[nm:names.index(b"\0", nm)].decode(), typ, (b"" if typ == 8 else elf[off:off + size])


def device_code_sha256(path=None):
    """sha256 over the gfx950 code objects inside the library (the clang offload bundles' device entries, in file order):
    of each, the sections that ARE the kernels -- .text (instructions), .rodata (kernel descriptors, constants), .data and
    .note (the kernels' metadata: names, registers, LDS).  Kernel traffic depends on the device code only: host-side edits (a
    comment shifts the __LINE__ of an error message) change the file's hash but not this one, and neither does the directory
    the objects were compiled in -- hipcc derives a per-translation-unit id (``__hip_cuid_<hash>``) from the source PATH, which
    lands in the symbol / string / hash tables of every code object (38-103 differing bytes per object between two
    checkouts: VERDICT r04 item 9) and is left out here.  tests/test_code_object.py builds one source in two directories."""
    import struct
    if path is None:
        from yolov3 import _hip
        path = os.path.abspath(_hip.LIB_PATH)
    with open(path, "rb") as fh:
        data = fh.read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    h = hashlib.sha256()
    pos, found = 0, 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            break
        nent = struct.unpack_from("<Q", data, i + 24)[0]
        off = i + 32
        for _ in range(nent):
            o, sz, tl = struct.unpack_from("<QQQ", data, off)
            triple = data[off + 24:off + 24 + tl]
            off += 24 + tl
            if sz and not triple.startswith(b"host"):
                for name, _, body in _elf_sections(data[i + o:i + o + sz]):
                    if name in (".text", ".rodata", ".data", ".note"):
                        h.update(name.encode() + b":%d:" % len(body))
                        h.update(body)
                found += 1
        pos = i + 24
    return h.hexdigest() if found else None


def load_traffic_table():
    """HBM-side traffic per launch comes from separate rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE cannot share a
    pass and counters cannot be read from inside this process): tools/profile_gpu.sh -> TRAFFIC_FILE (profiles/r06_traffic.json),
    which records the sha256 of the library it measured and of its device code objects.  A table measured on other
    kernels is not used."""
    try:
        with open(TRAFFIC_FILE) as fh:
            table = json.load(fh)
    except (OSError, ValueError):
        return None, "no traffic table"
    same = table.get("device_code_sha256") == device_code_sha256() if table.get("device_code_sha256") else \
        table.get("lib_sha256") == lib_sha256()
    if not same:
        return None, "traffic table is from another build of libyolov3_hip.so's kernels (stale): null"
    return table, "HBM bytes per launch, rocprofv3 PMC FETCH_SIZE x2 + WRITE_SIZE in separate passes (%s, same binary)" % (
        os.path.relpath(TRAFFIC_FILE, ROOT))


def cpu_baseline_in_child(args):
    """The CPU baseline as a NUMBER: a fresh child process, started before this process makes any GPU
    call (no runtime threads, no pinned memory, nothing else of this job running), confined to ``cores`` quiet physical cores
    of one NUMA node with as many OpenMP threads; load average recorded on both sides.  Returns the child's JSON object."""
    cores = usable_cpus()
    cpus, node = pick_quiet_cpus(cores)
    env = dict(os.environ)
    # (the process is confined to those cores, one OpenMP thread per core; NOT OMP_PROC_BIND: with torch's thread pools bound
    # thread by thread the same run took 3.5x longer here, 60 % of it in the kernel)
    env.update({"OMP_NUM_THREADS": str(len(cpus)), "MKL_NUM_THREADS": str(len(cpus)), "Y3_CPU_BASELINE_CHILD": "1"})
    env.pop("OMP_PROC_BIND", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", "--model", args.model, "--dim", str(args.dim),
           "--obj-bias", str(args.obj_bias), "--cpu-budget", str(args.cpu_budget)]
    load0 = os.getloadavg()
    t0 = time.perf_counter()

    def pin():
        try:
            os.sched_setaffinity(0, cpus)
        except OSError:
            pass
    try:
        proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                              preexec_fn=pin, timeout=max(120.0, 6 * args.cpu_budget))
    except subprocess.TimeoutExpired:
        return {"error": "cpu baseline child timed out"}
    out = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{"):
            out = json.loads(ln)
    if proc.returncode != 0 or out is None:
        return {"error": "cpu baseline child failed (rc %s): %s" % (proc.returncode, proc.stderr[-400:])}
    out["process"] = "fresh child process, started and finished before this process made any GPU call"
    out["pinned_cpus"] = cpus
    out["numa_node"] = node
    out["loadavg_before"] = [round(v, 2) for v in load0]
    out["loadavg_after"] = [round(v, 2) for v in os.getloadavg()]
    # a host whose run queue is longer than the cores this job may use: the wall-clock `value` is then a statement about the
    # neighbours; `value_cpu_time` is the figure to compare between runs
    out["noisy"] = bool(load0[0] > cores)
    out["wall_s"] = round(time.perf_counter() - t0, 1)
    return out


def cpu_baseline_child_main(args):
    """``bench.py --cpu-baseline-child``: only the CPU baseline, one JSON line (see cpu_baseline_in_child)."""
    from yolov3 import weights as W
    from yolov3.cfgparse import parse_config
    cfg = os.path.join(ROOT, "pytorch-yolov3_amd", "models", args.model + ".cfg")
    blocks, net_info = parse_config(cfg)
    params = W.synth_params(blocks, net_info, seed=0, obj_bias=args.obj_bias, calib=W.load_calibration(args.model))
    print(json.dumps(cpu_baseline(cfg, params, args.model, args.dim, args.cpu_budget)), flush=True)
    return 0


def cpu_baseline(cfg, params, model, dim, budget_s):
    """the reference's "-d cpu" op sequence (oracle/: torch-CPU Conv2d -> BN -> LeakyReLU as separate
    float32 ops, NCHW, numpy greedy NMS) on the host cores.  Two legs inside ``budget_s`` seconds of CPU work: batch 1 -- what
    the reference's command line runs (one frame per ``inference()`` call, /root/reference/yolov3/__main__.py:159-165) --
    gets up to 60 % of the budget for the protocol's 3 warm-up + 10 timed iterations, batch 16 what is left; a leg that
    cannot hold 3 + 10 is cut short and says so (``truncated``).  Every leg reports min / median / max of its timed
    iterations: the spread between runs of this baseline on the pool's hosts is +-40 %, the line must show it.
    ``value`` is the BETTER leg's median rate (``value_kind``): batch 16 is slower per frame on these hosts (every early
    layer materialises 0.4-0.8 GB float32 tensors, freshly allocated and page-faulted by each op), so the fair CPU baseline
    is the frame-at-a-time rate."""
    from oracle import darknet_oracle as orc
    from yolov3.synthdata import synth_frames
    cores = usable_cpus()
    if os.environ.get("Y3_CPU_BASELINE_CHILD") == "1" and hasattr(os, "sched_getaffinity"):
        cores = min(cores, len(os.sched_getaffinity(0)))      # the parent pinned this process to that many quiet cores
    torch.set_num_threads(cores)
    onet = orc.OracleDarknet(cfg).set_params(params)
    frames = [f for f in synth_frames(123, 16, dim, dim)]
    legs = {}
    spent = 0.0
    for batch, share in ((1, 0.6), (16, 1.0)):
        leg_budget = budget_s * share - spent          # batch 16: everything batch 1 left
        t_leg = 0.0
        times, cpus, warm = [], [], 0
        want_warm, want_timed = 3, 10
        while len(times) < want_timed:
            c0, p0 = time.perf_counter(), time.process_time()
            orc.inference(onet, frames[:batch], 0.05, 0.3)
            dt, dcpu = time.perf_counter() - c0, time.process_time() - p0
            spent += dt
            t_leg += dt
            if warm == 1 and not times and (leg_budget - t_leg) / dt < want_warm - 2 + want_timed:
                want_warm = 1                     # (judged on the SECOND call: the first pays one-time set-up) the leg's budget
                                                  # cannot hold 3 + 10 iterations: 1 warm-up, as many timed as fit
            if warm < want_warm:
                warm += 1
                continue
            times.append(dt)
            cpus.append(dcpu)
            if t_leg + dt > leg_budget and len(times) >= 2:
                break
        med = float(np.median(times))
        cpu_med = float(np.median(cpus))
        legs[batch] = dict(fps=round(batch / med, 3), fps_min=round(batch / max(times), 3), fps_max=round(batch / min(times), 3),
                           median_s=round(med, 4), min_s=round(min(times), 4), max_s=round(max(times), 4), warmup=warm,
                           timed=len(times), truncated=bool(warm < 3 or len(times) < 10),
                           # CPU seconds (user + system, all threads of the process) per call: what a neighbour on the same
                           # host cannot take away -- wall time it can (2.6 .. 15.6 frames/s by wall
                           # clock over seven runs of one protocol)
                           cpu_s_median=round(cpu_med, 4), cpu_s_min=round(min(cpus), 4), cpu_s_max=round(max(cpus), 4),
                           frames_per_core_second=round(batch / max(cpu_med, 1e-9), 4),
                           busy_cores=round(cpu_med / max(med, 1e-9), 2))
    best = max(legs, key=lambda b_: legs[b_]["fps"])
    fpcs = legs[best]["frames_per_core_second"]
    return dict(value=legs[best]["fps"], unit="frames/s", cores=cores, cpu_model=cpu_model(), kind="port",
                # contention-proof companion of `value`: frames per CPU-second of the process (time.process_time: user + system
                # over all threads), and that rate on `cores` fully owned cores.  `value` is wall clock and moves with the
                # neighbours' load on the shared host; this one does not (much: shared caches and SMT siblings still count)
                frames_per_core_second=fpcs, value_cpu_time=round(fpcs * cores, 3),
                value_cpu_time_kind="frames per process CPU-second x cores (best leg)",
                value_kind="best_of_batch1_batch16_median", value_min=legs[best]["fps_min"], value_max=legs[best]["fps_max"],
                best_batch=best, batch1=legs[1], batch16=legs[16], truncated=legs[best]["truncated"],
                sample="%s %dx%d float32, torch-CPU conv/BN/leaky + numpy NMS (oracle/), %d threads; batch 1 (the reference CLI's "
                       "mode): %d warm-up + %d timed%s; batch 16: %d warm-up + %d timed%s; median (min / max alongside); value = the "
                       "better leg (batch %d); %.0f s of CPU work in a %.0f s budget" % (
                           model, dim, dim, cores, legs[1]["warmup"], legs[1]["timed"],
                           " (truncated to its share of the budget)" if legs[1]["truncated"] else "", legs[16]["warmup"],
                           legs[16]["timed"], " (truncated to the budget)" if legs[16]["truncated"] else "", best, spent, budget_s))


def lowp_agreement(dev, dtype="bf16"):
    """bf16 / fp16 HIP detections against the reference's float32 ``inference()`` lists on the golden frames
    (tests/golden/inference_yolov3.npz, produced by the reference; floors from the oracle emulating that storage type in
    tests/golden/bf16_agreement.json / f16_agreement.json).  Keep-set Jaccard by prediction row and score differences on
    common rows; at the bench regime also how many (frame, threshold) pairs -- and how many of the AUDITED-CLEAN ones, where
    no float32 deviation below 6e-5 can move an integer -- come out EXACTLY as the reference's lists (rows, classes, boxes)."""
    emu = {"bf16": "bf16", "fp16": "f16"}[dtype]
    ideal_key = "ideal_%s_jaccard" % emu
    import yolov3
    from yolov3 import weights as W
    from yolov3.synthdata import synth_frames
    from PIL import Image
    gdir = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(gdir, "inference_yolov3.npz"))
    with open(os.path.join(gdir, "%s_agreement.json" % emu)) as fh:
        floor_table = json.load(fh)
    floors = floor_table["yolov3"]

    def jpeg(name):
        return np.ascontiguousarray(np.asarray(Image.open(os.path.join(gdir, "images", name)).convert("RGB"))[:, :, ::-1])

    frames = [jpeg("000000229358.jpg"), synth_frames(9, 1, 608, 608)[0], jpeg("000000393569.jpg")]
    cfg = os.path.join(ROOT, "pytorch-yolov3_amd", "models", "yolov3.cfg")
    net = yolov3.Darknet(cfg, device=str(dev), dtype=dtype).eval()
    net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-5.0, calib=W.load_calibration("yolov3")))
    out = {}
    for tag in ("a", "b"):
        pth, ith = g[tag + "_thresholds"]
        res = yolov3.inference(net, frames, device=str(dev), prob_thresh=float(pth), nms_iou_thresh=float(ith), return_rows=True)
        jac, ideal, dps, kept, ref_kept = [], [], [], 0, 0
        for f in range(len(frames)):
            key = "%s_f%d_" % (tag, f)
            rows = set(int(r) for r in res[f][3])
            want = set(g[key + "rows"].tolist())
            gp = dict(zip(g[key + "rows"].tolist(), g[key + "prob"].tolist()))
            mine = {int(r): k for k, r in enumerate(res[f][3])}
            jac.append(len(rows & want) / len(rows | want) if rows | want else 1.0)
            ideal.append(floors["%s_f%d" % (tag, f)]["jaccard"])
            dps += [abs(float(res[f][1][mine[r]]) - gp[r]) for r in rows & want]
            kept += len(rows)
            ref_kept += len(want)
        dps = np.array(dps) if dps else np.zeros(1)
        out["thr_%.2f_iou_%.1f" % (pth, ith)] = dict(
            keep_set_jaccard=[round(j, 4) for j in jac], **{ideal_key: ideal}, kept=kept, reference_kept=ref_kept,
            score_abs_diff=dict(median=float(np.median(dps)), p90=float(np.percentile(dps, 90)),
                                p99=float(np.percentile(dps, 99)), max=float(dps.max())))
    # the BENCHMARKED regime (objectness bias -8.5, tens of kept boxes per frame): all nine sample images and the procedural
    # frames of tests/golden/inference_bench_regime_yolov3.npz, one image per call, pooled over frames
    g2 = np.load(os.path.join(gdir, "inference_bench_regime_yolov3.npz"))
    floors2 = floor_table["bench_regime"]["yolov3"]
    obj_bias = float(g2["obj_bias"])
    net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=obj_bias, calib=W.load_calibration("yolov3")))
    regime = {"obj_bias": obj_bias, "frames": len(g2["names"])}
    for tag in ("a", "b"):
        pth, ith = g2[tag + "_thresholds"]
        common = union = kept = ref_kept = pairs = exact = clean = clean_exact = 0
        dps = []
        for name in (str(n) for n in g2["names"]):
            frame = jpeg("000000%s.jpg" % name[3:]) if name.startswith("img") else synth_frames(int(name[5:]), 1, 608, 608)[0]
            res = yolov3.inference(net, frame, device=str(dev), prob_thresh=float(pth), nms_iou_thresh=float(ith), return_rows=True)[0]
            key = "%s_%s_" % (name, tag)
            rows, want = set(int(r) for r in res[3]), set(g2[key + "rows"].tolist())
            gp = dict(zip(g2[key + "rows"].tolist(), g2[key + "prob"].tolist()))
            mine = {int(r): k for k, r in enumerate(res[3])}
            common += len(rows & want)
            union += len(rows | want)
            kept += len(rows)
            ref_kept += len(want)
            dps += [abs(float(res[1][mine[r]]) - gp[r]) for r in rows & want]
            # exactly the reference's list: same prediction rows, and on them the same class and integer box
            ref_at = {int(r): k for k, r in enumerate(g2[key + "rows"])}
            same = rows == want and all(int(res[2][k]) == int(g2[key + "cls"][ref_at[int(r)]]) and
                                        np.array_equal(res[0][k], g2[key + "tlbr"][ref_at[int(r)]]) for k, r in enumerate(res[3]))
            is_clean = bool(g2[key + "audit"][4])
            pairs += 1
            exact += int(same)
            clean += int(is_clean)
            clean_exact += int(is_clean and same)
        dps = np.array(dps) if dps else np.zeros(1)
        regime["thr_%.2f_iou_%.1f" % (pth, ith)] = dict(
            keep_set_jaccard=round(common / max(union, 1), 4), **{ideal_key: floors2["all_" + tag]["jaccard"]}, kept=kept,
            reference_kept=ref_kept, score_abs_diff=dict(median=float(np.median(dps)), p99=float(np.percentile(dps, 99)), max=float(dps.max())),
            frames=pairs, frames_exactly_as_reference=exact, audited_clean_frames=clean, audited_clean_frames_exact=clean_exact)
    out["bench_regime"] = regime
    # PLANTED parameters (tools/make_planted.py): the procedural backbone with a 19 x 19 head fitted on the nine sample images
    # so that each has a handful of confident detections with margins (kept scores >= 0.6, class margins ~1, everything else
    # below 0.01) -- the regime real weights are in.  Reference lists: tests/golden/inference_planted_yolov3.npz.
    g3 = np.load(os.path.join(gdir, "inference_planted_yolov3.npz"))
    floors3 = floor_table["planted"]["yolov3"]
    net.set_params(W.planted_params(net.blocks, net.net_info))
    planted = {"frames": len(g3["names"])}
    from yolov3.preprocess import resize_bilinear_u8
    for tag in ("a", "b"):
        pth, ith = g3[tag + "_thresholds"]
        common = union = kept = ref_kept = same_cls = box_max = 0
        dps = []
        for name in (str(n) for n in g3["names"]):
            frame = resize_bilinear_u8(jpeg("000000%s.jpg" % name), 608, 608)
            res = yolov3.inference(net, frame, device=str(dev), prob_thresh=float(pth), nms_iou_thresh=float(ith), return_rows=True)[0]
            key = "%s_%s_" % (name, tag)
            want = g3[key + "rows"].tolist()
            ref_by_row = {r: k for k, r in enumerate(want)}
            rows = [int(r) for r in res[3]]
            common += len(set(rows) & set(want))
            union += len(set(rows) | set(want))
            kept += len(rows)
            ref_kept += len(want)
            for k, r in enumerate(rows):
                if r in ref_by_row:
                    j = ref_by_row[r]
                    same_cls += int(int(res[2][k]) == int(g3[key + "cls"][j]))
                    dps.append(abs(float(res[1][k]) - float(g3[key + "prob"][j])))
                    box_max = max(box_max, int(np.abs(res[0][k] - g3[key + "tlbr"][j]).max()))
        dps = np.array(dps) if dps else np.zeros(1)
        planted["thr_%.2f_iou_%.1f" % (pth, ith)] = dict(
            keep_set_jaccard=round(common / max(union, 1), 4), **{ideal_key: floors3["all_" + tag]["jaccard"]}, kept=kept,
            reference_kept=ref_kept, common=common, same_class_on_common=same_cls, box_abs_diff_px_max=box_max,
            score_abs_diff=dict(median=float(np.median(dps)), p99=float(np.percentile(dps, 99)), max=float(dps.max())))
    out["planted"] = planted
    out["note"] = ("yolov3 608 %s HIP path vs the reference's float32 inference() on 3 golden frames, procedural weights "
                   "(thousands of overlapping near-threshold boxes per frame); %s = the oracle emulating that storage type "
                   "on the same frames (tests/golden/%s_agreement.json); bench_regime = the same at the objectness "
                   "bias the throughput is measured at, pooled over the nine sample images + procedural frames; planted = a fitted "
                   "head that gives every sample image a handful of confident detections with margins (tools/make_planted.py)"
                   % (dtype, ideal_key, emu))
    return out


def latency_report(dev, model, dim, params, n_calls=200, n_video=300):
    """The mode a drop-in user hits first (VERDICT r05 missing item 4): the reference's command line runs ONE frame per
    ``inference()`` call (/root/reference/yolov3/__main__.py:157-165, "TODO: batch images") and its video loop one frame per
    iteration (inference.py:527-530).  Reported here: wall time of ``yolov3.inference(net, one net-sized uint8 frame)`` --
    upload, 75 launches, detect, records back, unpack: p50 / p99 / mean over ``n_calls`` calls per storage type, eager and with
    the plan replayed as one hipGraph (use_graph=1 on a non-default stream) -- and frames/s of the package's batched loops over
    ``n_video`` frames at --batch-size 1 and 16: ``detect_in_frames`` on decoded frames in memory (the loop itself) and
    ``detect_in_video`` on a YUV4MPEG2 file (the same loop + the numpy 4:2:0 decoder + draw_boxes: host-bound)."""
    import tempfile
    import yolov3
    from yolov3 import stream as ystream
    from yolov3 import videoio
    from yolov3.synthdata import synth_frames
    cfg = os.path.join(ROOT, "pytorch-yolov3_amd", "models", model + ".cfg")
    frame = synth_frames(321, 1, dim, dim)[0]
    out = {"what": "%s %dx%d, one frame per call: yolov3.inference() wall time in ms (upload + forward + detect + records back "
                   "+ unpack), %d calls after 10 warm-up" % (model, dim, dim, n_calls), "inference_ms": {}}
    side = torch.cuda.Stream(device=dev)
    nets = {}
    for dtype in ("float32", "fp16", "bf16"):
        for graph in (0, 1):
            net = yolov3.Darknet(cfg, device=str(dev), dtype=dtype, options={"use_graph": 1} if graph else None).eval()
            net.set_params(params)
            ts = []
            with torch.cuda.stream(side if graph else torch.cuda.current_stream(dev)):
                for _ in range(10):
                    yolov3.inference(net, frame, device=str(dev))
                for _ in range(n_calls):
                    t0 = time.perf_counter()
                    yolov3.inference(net, frame, device=str(dev))
                    ts.append((time.perf_counter() - t0) * 1e3)
            ts = np.array(ts)
            out["inference_ms"]["%s%s" % (dtype, "_graph" if graph else "")] = {
                "p50": round(float(np.percentile(ts, 50)), 3), "p99": round(float(np.percentile(ts, 99)), 3),
                "mean": round(float(ts.mean()), 3), "frames_per_s": round(1e3 / float(ts.mean()), 1)}
            if not graph:
                nets[dtype] = net
            else:
                del net
    # the batched loops, bf16 (the benchmarked storage type)
    net = nets["bf16"]
    frames = synth_frames(555, n_video, dim, dim)
    loops = {}
    for bs in (1, 16):
        # one untimed pass over ALL frames first: the pipeline, its plans and -- lazily, one per host buffer it cycles through --
        # its six pinned staging buffers of 17.7 MB are set up by the first pass (pinning costs ~10 ms each: timed, a 300-frame
        # loop read 930 instead of ~6000 frames/s, profiles/r06_latency.txt)
        sum(1 for _ in ystream.detect_in_frames(net, (f for f in frames), batch_size=bs))
        t0 = time.perf_counter()
        n = sum(1 for _ in ystream.detect_in_frames(net, (f for f in frames), batch_size=bs))
        dt = time.perf_counter() - t0
        loops["detect_in_frames_batch%d" % bs] = {"frames": n, "frames_per_s": round(n / dt, 1), "ms_per_frame": round(dt / n * 1e3, 3)}
    with tempfile.TemporaryDirectory(prefix="y3_bench_video_") as tmp:
        path = os.path.join(tmp, "clip.y4m")
        videoio.write_y4m(path, (f for f in frames), fps=25)
        t0 = time.perf_counter()
        n = sum(1 for _ in videoio.open_video(path)[1])
        decode_ms = (time.perf_counter() - t0) / max(n, 1) * 1e3
        for bs in (1, 16):
            ystream.detect_in_video(net, path, device=str(dev), batch_size=bs)      # untimed pass (set-up, as above)
            t0 = time.perf_counter()
            res = ystream.detect_in_video(net, path, device=str(dev), batch_size=bs)
            dt = time.perf_counter() - t0
            loops["detect_in_video_y4m_batch%d" % bs] = {"frames": len(res), "frames_per_s": round(len(res) / dt, 1),
                                                         "ms_per_frame": round(dt / max(len(res), 1) * 1e3, 3)}
        loops["y4m_decode_alone_ms_per_frame"] = round(decode_ms, 3)
    out["loops_bf16"] = loops
    out["note"] = ("one frame per call: the 16-bit modes' time is the frame's 75 kernels (0.59 ms of kernel time + ~2 us of dispatch gap "
                   "behind each, profiles/r06_per_op_dispatch_times_batch1*.txt) plus one synchronising copy; *_graph = use_graph=1, the "
                   "forward replayed as one hipGraph launch (no faster: the gaps are the GPU's, not the host's); detect_in_video's rate "
                   "is the numpy YUV decoder's and draw_boxes' (host), compare y4m_decode_alone_ms_per_frame")
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.cpu_baseline_child:
        return cpu_baseline_child_main(args)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    t_start = time.perf_counter()
    phases = {}
    # (Y3_BENCH_FORCE_LAUNCH=1: go through the launcher with one rank as well -- the only way to exercise it, RCCL included, on
    # a box with one GPU: tests/test_callers.py)
    if (args.gpus > 1 or os.environ.get("Y3_BENCH_FORCE_LAUNCH") == "1") and "WORLD_SIZE" not in os.environ:
        return self_launch(args, argv)
    plumbing = os.environ.get("Y3_BENCH_PLUMBING")
    if plumbing and "WORLD_SIZE" in os.environ:
        return plumbing_main(args, plumbing)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d\n" % (args.gpus, world))
        return 2
    import torch.distributed as dist
    # Y3_BENCH_FORCE_DIST=1 (under torchrun with one process): run the RCCL plumbing -- init, barrier, all-gather,
    # all-reduce -- with a single rank, so the multi-GPU code path can be exercised on a one-GPU box
    distributed = world > 1 or os.environ.get("Y3_BENCH_FORCE_DIST") == "1" or os.environ.get("Y3_BENCH_FORCE_LAUNCH") == "1"
    if torch.cuda.device_count() <= local_rank:
        sys.stderr.write("bench.py: rank %d needs GPU %d, %d visible\n" % (rank, local_rank, torch.cuda.device_count()))
        return 2
    # ---- everything that must happen BEFORE this process touches the GPU (device_count above does not) ----------------
    # (1) the CPU baseline, in a fresh pinned child process, on an otherwise idle job (rank 0 at N = 1 only, --full)
    cpu_base = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu_base = cpu_baseline_in_child(args)
        phases["cpu_baseline_s"] = round(time.perf_counter() - t_start, 1)
    # (2) this rank's threads onto the CPUs of its GPU's NUMA node (pinned buffers are allocated after this)
    placement = bind_rank_to_gpu_node(local_rank)
    t_gpu0 = time.perf_counter()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # was the sysfs guess the GPU this rank really runs on?  (torch exposes the PCI address once the device is initialised.)  If
    # not -- an enumeration order this code does not know -- bind again, to the node of the GPU the runtime reports, before any
    # pinned buffer is allocated
    try:
        pr = torch.cuda.get_device_properties(local_rank)
        real = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        placement["gpu_bdf_runtime"] = real
        placement["gpu_bdf_verified"] = (placement.get("gpu_bdf") == real) if placement.get("gpu_bdf") else None
        if placement["gpu_bdf_verified"] is False and os.environ.get("Y3_BENCH_NO_BIND") != "1":
            cpus = _parse_cpulist(_read("/sys/bus/pci/devices/%s/local_cpulist" % real))
            node = _read("/sys/bus/pci/devices/%s/numa_node" % real)
            if cpus:
                os.sched_setaffinity(0, cpus)
                placement.update(numa_node=int(node) if node not in (None, "") else -1, cpus=len(os.sched_getaffinity(0)), bound=True,
                                 rebound_after_init=True)
    except Exception:
        placement.setdefault("gpu_bdf_verified", None)
    ranks_seen = 1
    if distributed:
        ranks_seen = init_group("nccl", dev)

    from yolov3 import _hip, weights as W
    from yolov3.cfgparse import parse_config

    for kv in filter(None, args.tuning.split(",")):
        key, val = kv.split("=")
        _hip.check(_hip.lib().y3_set_tuning(key.encode(), int(val)))

    def params_for(model, obj_bias):
        blocks, net_info = parse_config(os.path.join(ROOT, "pytorch-yolov3_amd", "models", model + ".cfg"))
        return W.synth_params(blocks, net_info, seed=0, obj_bias=obj_bias, calib=W.load_calibration(model))

    nstream = max(1, args.streams)
    params = params_for(args.model, args.obj_bias)
    my_frames = frames_per_rank(args, rank, world)
    all_frames = [frames_per_rank(args, r, world) for r in range(world)]
    if args.scaling == "strong" and len(set(all_frames)) != 1:
        sys.stderr.write("bench.py: --scaling strong needs --total-frames divisible by the number of GPUs (one fixed-size collective)\n")
        return 2
    # Host side: ~80 launches per forward cost ~0.75 ms of one core per step (profiles/r02l_host_enqueue_probe.txt); N ranks
    # on a box that grants fewer than two cores per rank replay each forward as one captured hipGraph instead (0.07 ms).
    use_graph = {"auto": world > 1 and usable_cpus() < 2 * world, "0": False, "1": True}[args.graph]
    options = None                    # the Pipeline's own choice (throughput tiles when several batches are in flight)
    if use_graph:
        options = {"auto_mask": _hip.options().auto_mask | (_hip.AM_HALO_TILE256 if nstream > 1 else 0), "use_graph": 1}
    wl = Workload(args.model, args.dim, my_frames, args.dtype, params, dev, rank, world, args.kmax, nstream, options=options)
    phases["init_s"] = round(time.perf_counter() - t_gpu0, 1)          # process group, weights, plans, pinned buffers
    t_timed0 = time.perf_counter()
    elapsed = wl.timed(args.steps, args.warmup, distributed, resident=args.resident, repeats=args.repeats)
    phases["warmup_and_timed_s"] = round(time.perf_counter() - t_timed0, 1)
    dumped = None
    if args.dump_outputs:            # before anything else runs on the pipeline; every rank takes part (results() may gather)
        dets = last_step_detections(wl, args.resident)
        if rank == 0:
            dumped = dump_outputs(args.dump_outputs, dets)
    windows_ms = sorted(w / args.steps * 1e3 for w in wl.windows_s)
    kept = wl.kept_per_frame()
    gathered = [placement]
    if distributed:      # every rank's placement in rank 0's line (best effort: a diagnostic must not cost the run)
        try:
            allp = [None] * dist.get_world_size()
            dist.all_gather_object(allp, placement)
            gathered = allp
        except Exception as exc:
            gathered = [dict(placement, gather_error=repr(exc))]

    per_rank = rank_stats(wl.rank_elapsed_s, wl.host_enqueue_s, args.steps, world, dev) if distributed else \
        rank_stats(wl.rank_elapsed_s, wl.host_enqueue_s, args.steps, 1, None)
    per_rank["placement"] = gathered
    per_rank["cpus_per_rank"] = [p.get("cpus") for p in gathered]
    per_rank["numa_node"] = [p.get("numa_node") for p in gathered]
    extras = rank == 0 and world == 1 and args.full and not args.no_extras and not args.resident and args.scaling == "weak"
    line = None
    if rank == 0:
        report = roof = traffic_table = None
        if args.full or args.dump_ops:        # the per-kernel passes: runs of their own after the timed windows
            traffic_table, traffic_note = load_traffic_table()
            telemetry = GpuTelemetry(placement.get("gpu_bdf_runtime") or placement.get("gpu_bdf"))
            sustain_steps = int(args.sustain / max(elapsed / args.steps, 1e-4)) if args.sustain > 0 else 0
            report = wl.kernel_report(args.profile_passes, args.dump_ops, telemetry=telemetry, sustain_steps=sustain_steps)
            roof = wl.roofline(report, traffic_table)
            roof["traffic_unit"] = traffic_note
        b, dim = my_frames, args.dim
        fps = sum(all_frames) * args.steps / elapsed
        flops_frame = MODEL_FLOPS_PER_FRAME.get((args.model, dim))
        line = {
            "metric": "frames/sec (608x608)" if dim == 608 else "frames/sec (%dx%d)" % (dim, dim),
            "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            # R back-to-back windows of exactly `steps` steps each; value / ms_per_step are the median window's
            "repeats": {"windows": len(windows_ms), "ms_per_step_min": round(windows_ms[0], 4),
                        "ms_per_step_median": round(elapsed / args.steps * 1e3, 4), "ms_per_step_max": round(windows_ms[-1], 4),
                        "value_min": round(sum(all_frames) / windows_ms[-1] * 1e3, 1), "value_max": round(sum(all_frames) / windows_ms[0] * 1e3, 1)},
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "full": bool(args.full),
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "%s %dx%d batch=%d/GPU %s, procedural weights, uint8 frames %s -> "
                                   "detections (thr 0.05, NMS IoU 0.3), ~%d kept/frame" % (
                                       args.model, dim, dim, b, args.dtype,
                                       "resident in HBM, records left on the device (--resident: NOT the headline "
                                       "configuration)" if args.resident else
                                       "in pinned host memory, upload + records back to pinned host memory inside every step "
                                       "(PCIe inclusive, SURVEY.md 8(d)), yolov3.pipeline.Pipeline", kept),
                       "frames_per_gpu": b, "global_batch": sum(all_frames), "parallelism": "dp%d" % world,
                       "batches_in_flight_per_gpu": nstream, "ranks_seen_by_collective": ranks_seen,
                       "plan_options": wl.options or "library defaults", "timed_loop": "yolov3.pipeline.Pipeline.submit",
                       "collective": ("1 x all_gather_into_tensor(%d x %d x 8 int32 records) per step, side stream" % (
                           b, args.kmax)) if distributed else "none"},
            "use_graph": bool(use_graph),
            # hardware queues the HIP runtime maps this rank's five streams onto (the environment's setting, else the runtime's
            # default; yolov3/_hip.py: hw_queues)
            "gpu_max_hw_queues": {"value": _hip.hw_queues()[0], "certain": _hip.hw_queues()[1]},
            # a library other than the in-tree product build (Y3_HIP_LIB: stamps / experiment variants) or a debug knob:
            # the line then is a diagnostic, not a result
            "diagnostic_build": bool(os.environ.get("Y3_HIP_LIB") or os.environ.get("Y3_BENCH_DEBUG_AFTER_WARMUP")),
            "per_rank": per_rank,
            "cpu_baseline": None,
            "cpu_baseline_why": None if world == 1 and args.full and not args.no_cpu_baseline else (
                "measured with --full only" if not args.full else "--no-cpu-baseline" if world == 1 else
                "measured on rank 0 at N = 1 only (the host cores are busy feeding N ranks; see the N = 1 line)"),
            "lib_sha256": lib_sha256()[:16],
            "device_code_sha256": (device_code_sha256() or "")[:16],
        }
        if dumped is not None:
            line["dump_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "arrays": dumped,
                                    "what": "detections of the last timed step (Pipeline.results of its ticket)"}
        if flops_frame:
            line["end_to_end_tflops"] = round(fps * flops_frame / 1e12, 2)
            line["end_to_end_frac_of_peak"] = round(fps * flops_frame / 1e12 / (PEAK_TFLOPS[args.dtype] * world), 4)
        if report is not None:
            line["roofline"] = roof
            line["kernels"] = {k: {"ms": round(v["ms"], 4), "ms_min": round(v["ms_min"], 4), "ms_event_bracket": round(v["ms_bracket"], 4),
                                   "launches": v["launches"],
                                   "tflops": round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 2),
                                   "GBps": round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1)}
                               for k, v in report["by_kernel"].items()}

    phases["report_s"] = abs(round(time.perf_counter() - t_timed0 - phases["warmup_and_timed_s"], 1))
    t_extras0 = time.perf_counter()
    if extras:
        # ---- the same steps with the frames already in HBM and the records left there (the kernels alone) ----------
        e2 = wl.timed(args.steps, min(args.warmup, 5), False, resident=True)
        line["resident"] = {
            "value": round(my_frames * args.steps / e2, 2), "unit": "frames/s", "ms_per_step": round(e2 / args.steps * 1e3, 4),
            "what": "same pipeline, frames resident in HBM and records left on the device (rounds 1-3 reported this as `value`); "
                    "the headline adds, inside every step, y3_copy_bytes on a copy stream (8 workgroups read the pinned frames over "
                    "PCIe into one of six device buffers) and 4 workgroups writing the records back (`gpu_max_hw_queues`: "
                    "whether the copy stream has a hardware queue of its own)"}
        # ---- the other single-GPU configurations of BASELINE.json (parity cases; each with its own roofline) -----
        others = []
        for model, dim, batch, dtype in (("yolov3-tiny", 416, 8, "float32"), ("yolov3-spp", 608, 16, "bf16"),
                                         ("yolov3", 608, 16, "fp16"), ("yolov3", 608, 16, "bf16"), ("yolov3", 608, 16, "float32")):
            if (model, dim, batch, dtype) == (args.model, args.dim, args.batch, args.dtype):
                continue
            p = params if model == args.model else params_for(model, args.obj_bias)
            w2 = Workload(model, dim, batch, dtype, p, dev, 0, 1, args.kmax, nstream)
            # enough steps for a steady state: a step of yolov3-tiny is 0.6 ms (filling and draining three streams would be a
            # quarter of a 20-step run), one of float32 yolov3 18 ms
            steps = 100 if model == "yolov3-tiny" else max(6, min(args.steps, 20 if dtype == "float32" else args.steps))
            e = w2.timed(steps, 2 * nstream, False, repeats=3)             # median of three windows, like the headline's five
            e_res = w2.timed(steps, 2 * nstream, False, resident=True)      # rounds 1-3 reported this one
            rep = w2.kernel_report(9, telemetry=GpuTelemetry(placement.get("gpu_bdf_runtime") or placement.get("gpu_bdf")),
                                   sustain_steps=int(0.5 / max(e / steps, 1e-4)))
            f = batch * steps / e
            ff = MODEL_FLOPS_PER_FRAME.get((model, dim))
            others.append({"workload": "%s %dx%d batch=%d %s" % (model, dim, dim, batch, dtype), "value": round(f, 2),
                           "unit": "frames/s", "steps": steps, "ms_per_step": round(e / steps * 1e3, 4),
                           "resident": round(batch * steps / e_res, 2), "kept_per_frame": w2.kept_per_frame(),
                           "end_to_end_frac_of_peak": round(f * ff / 1e12 / PEAK_TFLOPS[dtype], 4) if ff else None,
                           "roofline": w2.roofline(rep, traffic_table)})
            del w2
            torch.cuda.empty_cache()
        line["other_configs"] = others
        # ---- NMS cost is data dependent -- the headline workload at the reference test's thresholds
        # (/root/reference/tests/test_inference.py:26-87: 0.2 / 0.3) and in a heavy regime (~4000 candidates per frame; kmax
        # raised so that the records still hold every kept box)
        regimes = []
        for what, ob, pth, ith, kmax2 in (("thresholds of the reference's accuracy test", args.obj_bias, 0.2, 0.3, args.kmax),
                                          ("heavy: about 4000 candidates per frame", HEAVY_OBJ_BIAS, 0.05, 0.3, 2048)):
            p = params if ob == args.obj_bias else params_for(args.model, ob)
            w2 = Workload(args.model, args.dim, args.batch, args.dtype, p, dev, 0, 1, kmax2, nstream, prob_thresh=pth,
                          nms_iou_thresh=ith)
            e = w2.timed(args.steps, 2 * nstream, False, repeats=3)
            regimes.append({"what": what, "obj_bias": ob, "prob_thresh": pth, "nms_iou_thresh": ith, "kmax": kmax2,
                            "value": round(args.batch * args.steps / e, 2), "unit": "frames/s",
                            "ms_per_step": round(e / args.steps * 1e3, 4), "kept_per_frame": w2.kept_per_frame(),
                            "candidates_per_frame": w2.candidates_per_frame()})
            del w2
            torch.cuda.empty_cache()
        line["detection_regimes"] = regimes
        if not args.no_latency:
            t_lat = time.perf_counter()
            try:
                line["latency"] = latency_report(dev, args.model, args.dim, params)
            except Exception as exc:         # a diagnostic section must not void the bench line
                line["latency"] = {"error": repr(exc)}
            phases["latency_s"] = round(time.perf_counter() - t_lat, 1)
        for key, dt in (("bf16_agreement", "bf16"), ("f16_agreement", "fp16")):
            try:
                line[key] = lowp_agreement(dev, dt)
            except Exception as exc:    # the golden files are test data: their absence must not void the bench line
                line[key] = {"error": repr(exc)}
        phases["extras_s"] = round(time.perf_counter() - t_extras0, 1)

    # ---- CPU baseline: the oracle (reference "-d cpu" op sequence) timed on the host cores, measured in a child process
    # BEFORE this process touched the GPU (top of main)
    if rank == 0 and cpu_base is not None:
        if "error" in cpu_base:
            # the child could not run (no fork, a sandbox without sched_setaffinity ...): measure in this process, after the GPU
            # work, as rounds 1-4 did -- a noisier number is better than none -- and say so
            why = cpu_base["error"]
            cpu_base = cpu_baseline(wl.cfg, params, args.model, args.dim, args.cpu_budget)
            cpu_base["process"] = "in-process fallback AFTER the GPU work (the pinned child process failed: %s)" % why
        line["cpu_baseline"] = cpu_base

    if rank == 0:
        phases["total_s"] = round(time.perf_counter() - t_start, 1)
        line["phases_s"] = phases
        print(json.dumps(line), flush=True)
    if distributed:
        dist.barrier()          # ranks > 0 wait for rank 0's profiling passes before the group goes away
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
