#!/usr/bin/env python3
"""Benchmark: efvitcp RX per-frame transform on MI355X (device-resident).

One step = one pn_classify launch over this rank's batch of RX-ring slots already
resident in HBM (parse + IP/TCP checksum verification + conn-table probe +
payload off/len, one 16-B record per frame).  Default workload at one GPU = BASELINE
configs[1] (C2: 1 Mi x 1514-B IPv4/TCP frames, 1 flow); at N>1 GPUs = configs[3]
(C4: 16 Mi x 1514-B frames over 1024 flows sharded by index across 8 GPUs, i.e.
2 Mi frames per GPU, rank r owning global frames [r*2Mi, (r+1)*2Mi)): weak scaling,
no collective on the data path (the frames shard by index and nothing is exchanged,
SURVEY §8e).  With --full every rank sha256-gates its own shard against the committed
oracle digest.  torch.distributed over gloo (host-side, no RCCL) carries only the start/stop
barriers, the reductions of the timing and the gathered gates; the aggregate is timed
over one common barrier-to-barrier window.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config 2|3|4|5] [--frames N] [--dump-outputs DIR]
  python bench.py --full ...       (the same, with everything listed under "--full" below)
  python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...

A plain run does what the headline needs and no more: it generates the resident batches, warms up,
times the K steps and prints the line (metric, value, unit, ms_per_step, the kernel's roofline).
--dump-outputs DIR then also writes the records of the last timed step (the generator is seeded: the
same arguments give the same frames in every run, so two builds can be compared record for record).
--full adds the correctness gate, the same-run ceilings, the secondary workloads, the end-to-end legs
and the CPU baseline described below.

Without torchrun, --gpus N > 1 spawns the N ranks itself (spawn start method, before
anything touches a GPU in the parent); rank r uses device r % device_count, so on a
box with fewer GPUs than ranks the same flow runs as a rehearsal (ranks share a GPU,
"ranks_per_device" in the line).

Rank 0 prints ONE JSON line: metric = wire Gbit/s = 8*sum(14+tot_len)/t plus
Mframes/s and the roofline of the kernel; with --full also the correctness gate (full-batch sha256
against tests/golden/full_digests.json), and at N=1 the secondary workloads (C3, C5, a packed
C3 capture through pn_classify_indexed, the TX checksum fill at frame_off 2 and 14),
the CPU baseline and the pinned-host end-to-end rates.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
STRIDE, FRAME_OFF = 2048, 2  # RecvBufSize (Core.h:45); IP header 16-B aligned
METRIC = "device-resident Gbit/s + Mframes/s, 1500 B IPv4/TCP frames, 1/2/4/8 MI355X"

WORKLOADS = {
    2: "C2: 1514-B IPv4/TCP frames (tot_len 1500), 1 flow, 2048-B slots",
    3: "C3: 64-1514-B mixed frames, 1024 flows (32 TIME_WAIT, 1/64 miss), 2048-B slots",
    4: "C4: 1514-B frames over 1024 flows, 2048-B slots (16 Mi frames over 8 GPUs)",
    5: "C5: IPv4 options + odd lengths + bad-checksum + adversarial probe cluster, 2048-B slots",
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, default=0, choices=[0, 2, 3, 4, 5],
                    help="workload (default: C2 at one GPU, C4 = BASELINE configs[3] at N>1)")
    ap.add_argument("--frames", type=int, default=0, help="frames per GPU (default: 1 Mi; C4: 2 Mi)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: the correctness gate against the oracle and the committed "
                         "digests, the same-run ceilings, the secondary workloads, the end-to-end legs and the CPU "
                         "baseline (the options below choose among them); without it: set up, warm up, time the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the records of the last timed step to DIR/records.npy "
                         "(float64, one column per record field; at N>1 each rank its records_rank<r>.npy)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="no end-to-end legs (host ring in, records out)")
    ap.add_argument("--e2e", action="store_true",
                    help="the headline and the end-to-end host-ring leg only (no secondary legs, no CPU baseline)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the C3/C5/packed/TX sub-measurements")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget for the CPU baseline leg")
    ap.add_argument("--stream-ceiling-only", action="store_true",
                    help="PMC passes (scripts/gpu_pmc.sh): only the stream-read calibration, no ablated kernel "
                         "(its dispatches share the RX kernel's name)")
    ap.add_argument("--batches", type=int, default=4,
                    help="distinct resident batches the steps rotate over (defeats reuse of a fixed slice of "
                         "the 256 MiB memory-side cache across launches)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full and (args.e2e or args.stream_ceiling_only):
        ap.error("--e2e and --stream-ceiling-only choose among the legs of --full: add --full")
    return args


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ----------------------------------------------------------------------------- CPU side
def cgroup_cpu_quota():
    """CPUs the cgroup grants this process (cgroup v2 cpu.max / v1 cfs quota), None if unlimited."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        if q != "max":
            return max(1, -(-int(q) // int(per)))
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = int(f.read())
        if q > 0:
            return max(1, -(-q // per))
    except (OSError, ValueError):
        pass
    return None


def cpu_threads():
    """The cores this process may actually run on: its CPU affinity, capped by the cgroup's CPU
    quota (a GPU box's share of the host's cores; more threads than that only time-slice)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    q = cgroup_cpu_quota()
    return min(n, q) if q else n


def cpu_baseline(slots, n, entries, mask, max_conn, budget_s, gpu_records=None):
    """The reference's own per-frame code, compiled from /root/reference into oracle/_ref/libref_core.so
    (kind "reference"), on this host's cores:
      - the headline: the debug build's work per frame (Core::checksum + connHashKey + findConnEntry + the
        TIME_WAIT test + TcpConn::onPack's head, oracle/ref_core.cc ref_bench_batch), beside the GPU's
        verified classify;
      - release_path: the release build's (the same without Core::checksum, ref_release_batch), beside the
        GPU's pn_set_verify(ctx, 0) figures;
    each at the fastest thread count of its own sweep, and one thread.  Every figure is the median of 5
    timed passes with their min / max; a headline that disagrees with its own sweep point at the same
    thread count by more than 15 % is re-measured (both) instead of published as is.  The oracle's C port
    of the same paths ("port", oracle/pn_oracle.c) is timed beside it and is the headline only when
    libref_core.so is absent.  The reference's digests over the sample are compared with the same digests
    of the GPU's records for those frames."""
    import pollnet_amd as pa
    from oracle import pyoracle as orc

    threads = cpu_threads()
    sample = min(n, 1 << 18)  # 256 Ki frames (~0.4 GB of frame bytes)
    # a private copy of the sample: numpy backs a large array with transparent huge pages (madvise), where the
    # shared ring's shard is tmpfs with 4-KiB pages; on the pool's EPYC hosts the reference's own code reads that
    # 1.7-2.1x slower, the port 1.1-1.3x (scripts/cpu_placement_probe.py, profiles/r05/cpu_placement.json) -- the
    # baseline takes the placement that is fastest for the reference
    slots = np.array(slots[:sample], copy=True)
    wire = pa.wire_bytes(slots, STRIDE, FRAME_OFF, sample)
    ref = None
    try:
        ref = orc.RefBench(entries) if orc.ref_core() is not None else None
    except (OSError, AttributeError):
        ref = None

    def port(th, release=False):
        orc.classify_batch(slots, STRIDE, FRAME_OFF, sample, entries, mask, max_conn, threads=th, release=release,
                           ref_only=not release)

    def reference(th):
        ref.batch(slots, STRIDE, FRAME_OFF, sample, th)

    def reference_release(th):
        ref.release(slots, STRIDE, FRAME_OFF, sample, th)

    def one_pass(fn, th, secs):
        t0 = time.perf_counter()
        passes = 0
        while True:
            fn(th)
            passes += 1
            el = time.perf_counter() - t0
            if el >= secs:
                return passes * sample / el, passes * wire * 8 / el / 1e9, passes

    def stats(runs, th):
        gb = sorted(r[1] for r in runs)
        fr = sorted(r[0] for r in runs)
        return {"value": round(statistics.median(gb), 2), "unit": "Gbit/s",
                "mframes_per_s": round(statistics.median(fr) / 1e6, 3), "cores": th,
                "min": round(gb[0], 2), "max": round(gb[-1], 2), "reps": len(runs), "passes": sum(r[2] for r in runs)}

    def interleaved(legs, reps):
        """legs: {name: (fn, threads, seconds)}; the reps of all legs round-robin (rep 1 of every leg, then rep 2,
        ...), so a change in the host's load over the leg lands on every figure alike; median / min / max each"""
        runs = {k: [] for k in legs}
        for _ in range(reps):
            for k, (fn, th, secs) in legs.items():
                runs[k].append(one_pass(fn, th, secs))
        return {k: stats(runs[k], legs[k][1]) for k in legs}

    counts = sorted({c for c in (8, 16, 32, 64, threads) if c <= threads})
    head_fn = reference if ref is not None else port
    kind = "reference" if ref is not None else "port"
    rel_fn = reference_release if ref is not None else (lambda th: port(th, True))
    c1 = c1_socket_loopback()

    def sweep_of(fn, secs):
        # the box's share of a large host can be smaller than its affinity mask: probe a few thread counts up to
        # the available cores and measure at the fastest (stated in the line)
        r = interleaved({t: (fn, t, secs) for t in counts}, 3)
        return {t: v["value"] for t, v in r.items()}

    sweep, sweep_rel = sweep_of(head_fn, budget_s * 0.02), sweep_of(rel_fn, budget_s * 0.01)
    best, best_rel = max(sweep, key=sweep.get), max(sweep_rel, key=sweep_rel.get)
    legs = {"head": (head_fn, best, budget_s * 0.06), "single": (head_fn, 1, budget_s * 0.025),
            "rel": (rel_fn, best_rel, budget_s * 0.04), "rel_1": (rel_fn, 1, budget_s * 0.02)}
    if ref is not None:
        legs.update({"port": (port, best, budget_s * 0.012), "port_1": (port, 1, budget_s * 0.012),
                     "port_rel_1": (lambda th: port(th, True), 1, budget_s * 0.01)})
    m = interleaved(legs, 5)
    remeasured = False
    for key, sw, b, fn, secs in (("head", sweep, best, head_fn, budget_s * 0.06),
                                 ("rel", sweep_rel, best_rel, rel_fn, budget_s * 0.04)):
        if abs(m[key]["value"] - sw[b]) > 0.15 * max(m[key]["value"], sw[b]):  # re-measure both, once
            remeasured = True
            r = interleaved({"sweep_point": (fn, b, secs / 3), key: (fn, b, secs)}, 5)
            sw[b] = r["sweep_point"]["value"]
            m[key] = r[key]
    for key, sw, b in (("head", sweep, best), ("rel", sweep_rel, best_rel)):
        m[key].update({"thread_sweep_gbit_per_s": sw, "sweep_point_at_cores": sw[b], "remeasured": remeasured,
                       "consistent_with_sweep": abs(m[key]["value"] - sw[b]) <= 0.15 * max(m[key]["value"], sw[b])})
    head, single, rel, rel_1 = m["head"], m["single"], m["rel"], m["rel_1"]
    code = ("the reference's own Core.h / TcpConn.h code (oracle/ref_core.cc ref_bench_batch, compiled from "
            "/root/reference by oracle/ref.mk, g++ -O3 -march=x86-64-v3)" if ref is not None else
            "'ref parse + checksum' port (oracle/pn_oracle.c orc_refsum_batch, -O3 -march=x86-64-v3)")
    out = dict(head)
    out.update({
        "kind": kind,
        "sample": f"Core::checksum + pollNet's key/probe/TIME_WAIT test + onPack's payload head per frame, {code}, "
                  f"over {sample} frames of the same workload (a private, huge-page-backed copy); median of {head['reps']} timed passes (min/max beside "
                  f"it), the passes of every CPU figure interleaved round-robin; contiguous index shards over {head['cores']} threads, the fastest of a sweep up to this "
                  f"process's {cpu_threads()} available cores (CPU affinity {len(os.sched_getaffinity(0))}, cgroup "
                  f"CPU quota {cgroup_cpu_quota()}, machine {os.cpu_count()})",
        "single_thread": single,
        "release_path": dict(rel, kind=kind, single_thread=rel_1,
                             code=("the reference's release build per frame: the same lines without Core::checksum "
                                   "(oracle/ref_core.cc ref_release_batch)" if ref is not None else
                                   "oracle/pn_oracle.c orc_release_batch"),
                             note="beside the GPU's release-path figures (pn_set_verify(ctx, 0): c2_release_path, "
                                  "e2e_zero_copy_pinned_host_release_path)"),
        "host_cpu": _cpu_model(),
        "c1_socket_loopback_ref": c1,
    })
    if ref is not None:
        p_mt, p_1, p_rel1 = m["port"], m["port_1"], m["port_rel_1"]
        out["port"] = {"value": p_mt["value"], "min": p_mt["min"], "max": p_mt["max"], "unit": "Gbit/s",
                       "mframes_per_s": p_mt["mframes_per_s"], "cores": head["cores"],
                       "single_thread_gbit_per_s": p_1["value"], "release_path_single_thread_gbit_per_s": p_rel1["value"],
                       "code": "oracle/pn_oracle.c orc_refsum_batch / orc_release_batch (the oracle's restatement of "
                               "the same paths)"}
        if gpu_records is not None:
            digest, n_valid = ref.batch(slots, STRIDE, FRAME_OFF, sample, head["cores"])
            rec = np.ascontiguousarray(gpu_records[: sample * 16]).view(pa.RESULT_DTYPE)
            out["reference_agrees_with_gpu_records"] = digest == orc.records_digest(rec)
            out["reference_frames_verified"] = n_valid
            out["release_path"]["reference_agrees_with_gpu_records"] = (
                ref.release(slots, STRIDE, FRAME_OFF, sample, rel["cores"]) == orc.records_digest(rec, release=True))
    return out


def c1_socket_loopback(seconds=1.5):
    """BASELINE config C1 beside it: the reference's own Socket.h server + client
    (oracle/_ref/ref_socket_c1, built from /root/reference by oracle/ref.mk) echoing
    1500-B messages over 127.0.0.1, window 1 (ping-pong RTT) and 8."""
    import subprocess

    exe = os.path.join(ROOT, "oracle", "_ref", "ref_socket_c1")
    if not os.path.exists(exe):
        return {"error": "oracle/_ref/ref_socket_c1 not built"}
    out = {}
    for w, port in ((1, 23411), (8, 23412)):
        try:
            r = subprocess.run([exe, str(seconds), str(w), str(port)], capture_output=True, text=True, timeout=30)
            out[f"window_{w}"] = json.loads(r.stdout.strip().splitlines()[-1])
        except Exception as ex:  # measured extra; never blocks the bench line
            out[f"window_{w}"] = {"error": str(ex)}
    return out


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


# ----------------------------------------------------------------------------- GPU legs
def e2e_rate(torch, ctx, slots, n, chunk=1 << 16, passes=3, stride=STRIDE):
    """Host ring -> GPU -> host records: pinned H2D of each chunk, kernel, D2H of
    its records, double-buffered over 2 streams (copy/compute overlap).  stride < 2048:
    the same frames re-laid in tighter slots (less PCIe per frame)."""
    import pollnet_amd as pa

    nchunks = (n + chunk - 1) // chunk
    if stride != STRIDE:  # the 1514-B frames of the 2-KiB slots re-laid at `stride` (pad byte included)
        slots = np.ascontiguousarray(slots[:n, :stride])
    host = torch.from_numpy(slots.reshape(-1)[: n * stride]).pin_memory()
    host_res = torch.empty(n * 16, dtype=torch.uint8).pin_memory()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dev = [torch.empty(chunk * stride, dtype=torch.uint8, device="cuda") for _ in range(2)]
    dres = [torch.empty(chunk * 16, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    best = None
    for _ in range(passes):
        t0 = time.perf_counter()
        for c in range(nchunks):
            b = c & 1
            s = streams[b]
            lo = c * chunk
            m = min(chunk, n - lo)
            with torch.cuda.stream(s):
                dev[b][: m * stride].copy_(host[lo * stride:(lo + m) * stride], non_blocking=True)
                ctx.classify(dev[b], stride, FRAME_OFF, m, dres[b], s)
                host_res[lo * 16:(lo + m) * 16].copy_(dres[b][: m * 16], non_blocking=True)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    wire = pa.wire_bytes(slots, stride, FRAME_OFF, n)
    return {"gbit_per_s": round(wire * 8 / best / 1e9, 2), "mframes_per_s": round(n / best / 1e6, 3),
            "h2d_gb_per_s": round(n * stride / best / 1e9, 2), "chunk_frames": chunk,
            "note": f"pinned hipMemcpyAsync H2D of whole {stride}-B slots + kernel + D2H records, 2 streams"}, host_res


def e2e_zero_copy(torch, ctx, slots, n, passes=3):
    """Host ring in place: the kernel reads the pinned host slots over PCIe (only each frame's
    lines cross the link) and writes the records into pinned host memory; one launch per pass."""
    import pollnet_amd as pa

    host = torch.from_numpy(slots.reshape(-1)[: n * STRIDE]).pin_memory()
    host_res = torch.empty(n * 16, dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream()
    ctx.classify(host, STRIDE, FRAME_OFF, n, host_res, stream)
    torch.cuda.synchronize()
    best = None
    for _ in range(passes):
        t0 = time.perf_counter()
        ctx.classify(host, STRIDE, FRAME_OFF, n, host_res, stream)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    wire = pa.wire_bytes(slots, STRIDE, FRAME_OFF, n)
    return {"gbit_per_s": round(wire * 8 / best / 1e9, 2), "mframes_per_s": round(n / best / 1e6, 3),
            "note": "pn_classify on pinned host 2048-B slots (zero copy), records to pinned host memory"}, host_res


def ceilings(torch, ctx, bufs, n, res, stream, steps=20, rounds=7, stream_only=False):
    """Same-run ceilings (kernels of the measurement-only tuning library, never the product path):
    the plain front-to-back stream read of one resident batch, and the tight one -- the production
    kernel with the conn-table probe and the lane reduction ablated (same window and stream loads,
    record stores, occupancy and workgroup order; pn_calib_classify_ablated).  The product and the
    ablated kernel are timed alternately over the same rotating batches (time_launches, HIP events);
    kernel_vs_ablated_ceiling = ablated / product <= 1 measures what the arithmetic and the probe cost."""
    from pollnet_amd import tuning as tn  # measurement-only library, never the product path

    sink = torch.zeros(4096, dtype=torch.int32, device=bufs[0].device)
    scratch = torch.empty_like(res)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    tn.calib_stream_read(ctx, bufs[0], bufs[0].numel(), sink, stream)
    ev[0].record(stream)
    for _ in range(10):
        tn.calib_stream_read(ctx, bufs[0], bufs[0].numel(), sink, stream)
    ev[1].record(stream)
    torch.cuda.synchronize()
    ts = ev[0].elapsed_time(ev[1]) / 10 * 1e-3
    if stream_only:
        return {"stream_read_gbs": round(bufs[0].numel() / ts / 1e9, 1)}
    prod, abl = [], []
    for _ in range(rounds):
        prod.append(time_launches(torch, lambda d: ctx.classify(d, STRIDE, FRAME_OFF, n, res, stream), bufs, steps,
                                  stream))
        abl.append(time_launches(torch, lambda d: tn.calib_classify_ablated(ctx, d, STRIDE, FRAME_OFF, n, scratch, stream),
                                 bufs, steps, stream))
    p_ms, a_ms = statistics.median(prod), statistics.median(abl)
    # the rounds' spread: a ratio within it of 1 is "at the ceiling" (when the probe and the reduction cost
    # nothing measurable, as on C2's one-connection table, the two kernels time equal up to noise)
    spread = (max(prod) - min(prod)) / p_ms
    return {"note": "tuning-library kernels (libpollnet_amd_tuning.so): stream read of one batch; the production "
                    "kernel with probe + lane reduction ablated, timed alternately with the product",
            "stream_read_gbs": round(bufs[0].numel() / ts / 1e9, 1),
            "product_ms_alternating": round(p_ms, 5), "ablated_kernel_ms": round(a_ms, 5),
            "kernel_vs_ablated_ceiling": round(a_ms / p_ms, 4),
            "product_round_spread": round(spread, 4),
            "at_ceiling_within_spread": abs(1 - a_ms / p_ms) <= max(spread, 0.002)}


def load_pmc(workload_key, sub=None):
    """The committed rocprofv3 --pmc summary for a workload (profiles/pmc_traffic.json, scripts/pmc_refresh.sh), with
    whether the built library still holds the kernel code the counters were taken on: each entry records the code
    hash of every kernel it summed over, compared here with the same hash of the library this run loads
    (pollnet_amd/codehash.py)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            e = json.load(f).get(workload_key)
    except (OSError, ValueError):
        return None
    if e is not None and sub is not None:
        e = e.get(sub)
    if e is None:
        return None
    from pollnet_amd import codehash

    try:
        ok, why = codehash.check_entry(e)
    except Exception as ex:  # a library or tool that cannot be read: never report the bytes as current
        ok, why = False, f"code identity not checked: {ex!r}"
    return dict(e, code_current=ok, code_check=why)


def pmc_fields(pmc, ms=None):
    """The traffic keys of a bench object: the committed bytes per launch only while the code is the measured
    code; otherwise null with traffic_stale true (a changed kernel needs a PMC refresh, scripts/pmc_refresh.sh)."""
    if pmc is None:
        return {"traffic": None, "traffic_over_algorithmic": None, "traffic_stale": None,
                "traffic_code_check": "no committed PMC entry for this workload"}
    cur = pmc["code_current"]
    out = {"traffic": pmc["hbm_bytes_per_launch"] if cur else None,
           "traffic_over_algorithmic": pmc.get("traffic_over_algorithmic") if cur else None,
           "traffic_stale": not cur, "traffic_code_check": pmc["code_check"]}
    if ms is not None:
        out["traffic_gbs"] = round(pmc["hbm_bytes_per_launch"] / (ms * 1e-3) / 1e9, 1) if cur else None
    return out


def golden_digest(cfg, first=0, n=None):
    """The committed oracle digest over config cfg's global frames [first, first+n) (tests/golden/
    make_golden.py): C2/C3/C5 [0, 1 Mi) and C4's 8 shards of 2 Mi; None when none covers that range."""
    try:
        with open(os.path.join(ROOT, "tests", "golden", "full_digests.json")) as f:
            full = json.load(f)
    except (OSError, ValueError):
        return None
    cands = [dict(full[f"c{cfg}"], first_index=0)] if f"c{cfg}" in full else []
    cands += full.get(f"c{cfg}_shards", [])
    for d in cands:
        if d.get("first_index", 0) == first and (n is None or d["n"] == n):
            return d
    return None


def time_launches(torch, fn, bufs, steps, stream, warmup=2, settle_s=0.04):
    """Average ms per launch of fn(buf) rotating over bufs, HIP events on `stream`.  Before
    timing, back-to-back launches run for at least `settle_s` of wall time: after an idle
    stretch (the host generating the next workload) a mixed-size workload such as C3 runs up
    to 15 % slow for its first ~100 launches (~16 ms) while the device's power state settles
    (scripts/warmup_probe.py, profiles/r02/s3/warmup_probe_c{2,3}.json; C2 shows no ramp)."""
    t0 = time.perf_counter()
    k = 0
    while k < warmup or time.perf_counter() - t0 < settle_s:
        fn(bufs[k % len(bufs)])
        k += 1
        if k % 8 == 0:
            torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for k in range(steps):
        fn(bufs[k % len(bufs)])
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def secondary_rx(torch, pa, cfg, n, steps, stream, packed=False):
    """C3 / C5 (and a packed C3 capture through pn_classify_indexed) at 1 Mi frames: kernel
    time over 2 rotating resident batches, algorithmic bytes = frame bytes + 16-B records,
    the frame-lines read ceiling of the same ring, the committed PMC traffic, and the
    full-batch sha256 against the committed digest."""
    p = pa.rx.GenParams.for_config(cfg)
    table = pa.gen_conn_table(p)
    ctx = pa.RxContext(torch.cuda.current_device())
    ctx.set_conn_table(table)
    host = np.empty((n, STRIDE), dtype=np.uint8)
    bufs, wires = [], []
    for b in range(2):
        pa.gen_frames(p, n, STRIDE, FRAME_OFF, first_index=b * n, threads=min(16, cpu_threads()), out=host)
        wires.append(pa.wire_bytes(host, STRIDE, FRAME_OFF, n))
        bufs.append(torch.from_numpy(host.reshape(-1)).cuda())
        if b == 0:
            slots0 = host.copy()
    res = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    ctx.classify(bufs[0], STRIDE, FRAME_OFF, n, res, stream)
    torch.cuda.synchronize()
    ref = res.cpu().numpy()
    gd = golden_digest(cfg)
    sha_ok = gd is not None and gd["n"] == n and hashlib.sha256(ref.tobytes()).hexdigest() == gd["records_sha256"]
    kern = time_launches(torch, lambda d: ctx.classify(d, STRIDE, FRAME_OFF, n, res, stream), bufs, steps, stream)
    algo = int(sum(wires) / 2) + 16 * n
    c = ceilings(torch, ctx, bufs, n, res, stream, steps=steps)
    pmc = load_pmc(f"c{cfg}_n{n}")
    out = {"workload": WORKLOADS[cfg], "frames": n, "resident_batches": 2, "kernel_ms": round(kern, 5),
           "gbit_per_s": round(8 * sum(wires) / 2 / (kern * 1e-3) / 1e9, 1),
           "mframes_per_s": round(n / (kern * 1e-3) / 1e6, 1),
           "algorithmic_bytes_per_launch": algo, "achieved_gbs": round(algo / (kern * 1e-3) / 1e9, 1),
           "frac": round(algo / (kern * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "ablated_kernel_ms": c["ablated_kernel_ms"], "kernel_vs_ablated_ceiling": c["kernel_vs_ablated_ceiling"],
           "at_ceiling_within_spread": c["at_ceiling_within_spread"], "stream_read_gbs": c["stream_read_gbs"],
           **pmc_fields(pmc, kern), "records_sha256_matches_golden": bool(sha_ok)}
    # the mixed-size workloads read sparse, variable-length runs of lines in 2-KiB slots: their ceiling is the
    # box's stream read at their line traffic, not 8 TB/s at their algorithmic bytes
    if out.get("traffic_gbs"):
        out["traffic_rate_over_stream_read"] = round(out["traffic_gbs"] / c["stream_read_gbs"], 4)
    if packed:
        # packed capture: each frame (+ its pad byte) back to back, every Ethernet header at 2 mod 16
        # (the slots' alignment class): frame i+1 starts ((len_i + 17) & ~15) after frame i
        tl = (slots0[:, FRAME_OFF + 16].astype(np.int64) << 8) | slots0[:, FRAME_OFF + 17]
        ln = 14 + tl + 1
        step = (ln + 17) & ~15
        starts = FRAME_OFF + np.concatenate(([0], np.cumsum(step[:-1])))
        total = int(starts[-1] + step[-1] + STRIDE)
        packed_h = np.zeros(total, np.uint8)
        for i in range(n):  # ~1 s for 1 Mi frames
            packed_h[starts[i]:starts[i] + ln[i]] = slots0[i, FRAME_OFF:FRAME_OFF + ln[i]]
        pk = torch.from_numpy(packed_h).cuda()
        offs = torch.from_numpy(starts.astype(np.uint64).view(np.int64)).cuda()
        out_i = torch.empty_like(res)
        ctx.classify_indexed(pk, offs, FRAME_OFF, n, STRIDE - FRAME_OFF, out_i, stream)
        torch.cuda.synchronize()
        same = bool(np.array_equal(out_i.cpu().numpy(), ref))
        kp = time_launches(torch, lambda d: ctx.classify_indexed(d, offs, FRAME_OFF, n, STRIDE - FRAME_OFF, out_i,
                                                                 stream), [pk], steps, stream)
        algo_p = int(wires[0]) + 16 * n + 8 * n  # + the u64 offsets the kernel reads
        out["packed_indexed"] = {
            "note": "the same batch-0 frames packed back to back (a capture / packet-mmap block), pn_classify_indexed "
                    "over their offsets; one resident buffer",
            "packed_bytes": total, "kernel_ms": round(kp, 5),
            "gbit_per_s": round(8 * wires[0] / (kp * 1e-3) / 1e9, 1),
            "algorithmic_bytes_per_launch": algo_p, "frac": round(algo_p / (kp * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "records_equal_strided": same}
    ctx.close()
    return out


def secondary_streams(torch, pa, ctx, frames_b, slots, n, stream):
    """pn_match_streams (TcpStream::filterPacket on the GPU) over the
    resident C2 batches, rotating (their header lines exceed the memory-side cache): 8 wildcard filters,
    the frames' flow matching only the last; HIP events on the launch stream.  Algorithmic bytes per
    frame: the 64-B header window read + the 4-B stream id written.  The first 65,536 ids are checked
    against the numpy restatement of filterPacket (tests/streams_np.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from streams_np import match_streams_np

    flt = np.zeros(8, pa.STREAM_FILTER_DTYPE)
    for k in range(7):  # flows that are not in the batch
        flt[k] = (int.from_bytes(bytes([10, 9, k, 1]), "little"), 0, int.from_bytes((5000 + k).to_bytes(2, "big"), "little"), 0, 0)
    flt[7] = (0, 0, 0, int.from_bytes((1234).to_bytes(2, "big"), "little"), 0)  # dst port 1234: every frame
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.match_streams(frames_b[0], STRIDE, FRAME_OFF, n, flt, ids, stream)
    torch.cuda.synchronize()
    k = min(n, 65536)
    ok = bool(np.array_equal(ids[:k].cpu().numpy().view(np.uint32), match_streams_np(slots[:k], FRAME_OFF, flt)))
    from pollnet_amd import tuning as tn  # measurement-only library: the same-pattern ceiling

    R = len(frames_b)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    sink = torch.empty_like(ids)

    def timed(fn):
        ev[0].record(stream)
        for r in range(20):
            fn(frames_b[r % R])
        ev[1].record(stream)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / 20

    ts, tg, tw = [], [], []
    for _ in range(5):  # the product, its loads + tile round trip alone (tuning variant 18), and the same with the
        # required id stores but no filter compare (variant 34), alternately
        ts.append(timed(lambda d: ctx.match_streams(d, STRIDE, FRAME_OFF, n, flt, ids, stream)))
        tg.append(timed(lambda d: tn.match_streams_variant(ctx, d, STRIDE, FRAME_OFF, n, flt, sink, 18, stream)))
        tw.append(timed(lambda d: tn.match_streams_variant(ctx, d, STRIDE, FRAME_OFF, n, flt, sink, 34, stream)))
    ms, mg, mw = statistics.median(ts), statistics.median(tg), statistics.median(tw)
    pmc = load_pmc(f"match_streams_c2_n{n}")
    return {"kernel": "match_streams_mask_kernel", "frames": n, "resident_batches": R, "filters": 8, "kernel_ms": round(ms, 5),
            "mframes_per_s": round(n / (ms * 1e-3) / 1e6, 1),
            "algorithmic_bytes_per_launch": n * (64 + 4),
            "achieved_gbs": round(n * (64 + 4) / (ms * 1e-3) / 1e9, 1),
            "frac": round(n * (64 + 4) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            **pmc_fields(pmc, ms),
            "gather_loads_only_ms": round(mg, 5), "kernel_vs_gather_ceiling": round(mg / ms, 4),
            "loads_and_id_stores_ms": round(mw, 5), "kernel_vs_loads_and_stores_ceiling": round(mw / ms, 4),
            # HBM rate against the gather's: the kernel moves one 128-B line per frame AND its 4-B id, the
            # gather only the line (the ids are 3 % of the traffic)
            "kernel_vs_gather_hbm_rate": round(mg / ms * (128 + 4) / 128, 4),
            "first_65536_ids_vs_numpy": ok,
            "note": "one 128-B line per 2-KiB slot (PMC: every request 128 B); ceilings: the same kernel's loads and LDS "
                    "tile round trip alone, no compare or store (tuning variant 18), and the same with the 4-B id "
                    "stores the output needs but no filter compare (variant 34) (DESIGN §11)"}


def median_legs(rows):
    """Rounds of one bench_tcp_server mode -> one line: each leg (a dict with mframes_per_s) from its median round,
    with the rounds' rates as `rounds_mframes_per_s`; other keys from the first round; `delivered_ok` over all."""
    out = dict(rows[0])
    for k, v in rows[0].items():
        if isinstance(v, dict) and "mframes_per_s" in v and all(isinstance(r.get(k), dict) for r in rows):
            legs = sorted((r[k] for r in rows), key=lambda d: d.get("mframes_per_s", 0.0))
            out[k] = dict(legs[len(legs) // 2], rounds_mframes_per_s=[r[k].get("mframes_per_s") for r in rows])
    if any("delivered_ok" in r for r in rows):
        out["delivered_ok"] = all(r.get("delivered_ok") is True for r in rows)
    errs = [r["error"] for r in rows if "error" in r]
    if errs:
        out["error"] = errs[0]
    out["rounds"] = len(rows)
    return out


def server_poll():
    """The drop-in server itself (bench/bench_tcp_server quick): GpuTcpServer::poll over
    256 connections receiving in-order 1514-B segments from a pinned host ring (handshake, RX, the
    server's ACKs), GPU backend at RxBatch 512 and pipelined at 16384; at 512 also pipelined, through the
    resident classify service (Conf::RxResident, pn_service_*: a post per poll, no launch) and both; each
    with the checksum discard off too (the reference's release path: the kernel reads each frame's header
    lines only, pn_set_verify), the same server on the sequential CPU backend (the oracle classifying each
    frame on one core), and the reference's own server (pollnet's EfviTcpServer over efvitcp, compiled from
    /root/reference at build time, oracle/ref_server.hpp) on one core: 64 events per pollNet, the release
    build pollnet ships, no RX checksum (the NIC's job).  PCIe-bound: with checksums verified every frame
    crosses it whole."""
    import subprocess

    exe = os.path.join(ROOT, "bench", "bench_tcp_server")
    if not os.path.exists(exe):
        return {"error": "bench/bench_tcp_server not built"}
    try:
        r = subprocess.run([exe, "256", "400", "quick"], capture_output=True, text=True, timeout=120)
        line = json.loads(r.stdout.strip().splitlines()[-1])
        if r.returncode != 0:
            line["error"] = f"exit {r.returncode}: {r.stderr[-300:]}"
        # the best GPU leg beside the reference with the frames where a NIC leaves them: written by
        # another core of the CCD (resident_pair_l3: DDIO / cache injection, L3 or a neighbour's L2), and flushed from
        # the CPU caches after the link writes them (resident_pair_cold: DMA to DRAM); server-only rates drop the
        # link's time (its writes, flushes, the hand-off to the writer core)
        # Three interleaved rounds of each placement, hot (as the link leaves the frames) included; each leg reported
        # from its median round, with every round's rate beside it (one round can catch a neighbour's burst).
        modes = (("hot", "resident_pair"), ("l3", "resident_pair_l3"), ("cold", "resident_pair_cold"))
        rounds = {key: [] for key, _ in modes}
        for _ in range(3):
            for key, mode in modes:
                rc = subprocess.run([exe, "256", "1000", mode], capture_output=True, text=True, timeout=120)
                one = json.loads(rc.stdout.strip().splitlines()[-1])
                if rc.returncode != 0:
                    one["error"] = f"exit {rc.returncode}: {rc.stderr[-300:]}"
                rounds[key].append(one)
        for key, rows in rounds.items():
            line[key] = median_legs(rows)
        return line
    except Exception as ex:  # measured extra; never blocks the bench line
        return {"error": repr(ex)}


def sniffer_streams():
    """The sniffer path end to end (bench/bench_streams): 1 Mi captured frames in pinned host
    memory, 8 watched TCP streams (every 16th frame) among other TCP traffic; GpuTcpStreams::poll
    (pn_match_streams over PCIe, host reassembly of the watched frames) against every stream's
    filterPacket + handlePacket on one core; per-stream bytes and a checksum of them must agree."""
    import subprocess

    exe = os.path.join(ROOT, "bench", "bench_streams")
    if not os.path.exists(exe):
        return {"error": "bench/bench_streams not built"}
    try:
        r = subprocess.run([exe, str(1 << 20), "8", "16", "3"], capture_output=True, text=True, timeout=90)
        line = json.loads(r.stdout.strip().splitlines()[-1])
        if r.returncode != 0:
            line["error"] = f"exit {r.returncode}: {r.stderr[-300:]}"
        return line
    except Exception as ex:  # measured extra; never blocks the bench line
        return {"error": repr(ex)}


def small_batch_latency():
    """Host-visible round trip of one small batch (bench/bench_signal): pn_classify +
    stream sync against pn_classify_notify + a spin on the pinned completion word against a post to the
    resident classify service (pn_service_post + pn_service_wait), 64 / 512 / 1024 C2 frames,
    device-resident and zero-copy, verified and release path; median host wall clock, records compared."""
    import subprocess

    exe = os.path.join(ROOT, "bench", "bench_signal")
    if not os.path.exists(exe):
        return {"error": "bench/bench_signal not built"}
    try:
        r = subprocess.run([exe, "200"], capture_output=True, text=True, timeout=60)
        line = json.loads(r.stdout.strip().splitlines()[-1])
        if r.returncode != 0:
            line["error"] = f"exit {r.returncode}: {r.stderr[-300:]}"
        return line
    except Exception as ex:  # measured extra; never blocks the bench line
        return {"error": repr(ex)}


def secondary_tx(torch, pa, n, steps, stream, rounds=6):
    """TX checksum fill (pn_tx_fill, PN_TX_TCP) over C2 batches with both checksum fields
    scrambled, at the ring layout (frame_off 2) and efvitcp's SendBuf layout (frame_off 14 =
    offsetof(SendBuf, eth_hdr), Core.h:147-156).  Algorithmic bytes per frame = tot_len read
    + 4 B written (1,504).  Both layouts run on the SAME four resident buffers: the frames are moved
    between the offsets in place (the HBM pages stay), and the timing alternates the layouts over
    `rounds` rounds (order reversed every round), so their ratio is the layout's cost alone, not
    where a batch landed in HBM.  Correctness: the first 4096 frames equal the oracle's fill, and
    every filled frame equals the generator's original except the ones it built with a flipped
    payload bit (every 1024th)."""
    from oracle import pyoracle as orc
    from pollnet_amd import tuning as tn  # measurement-only library

    ctx = pa.RxContext(torch.cuda.current_device())
    out = {}
    p = pa.rx.GenParams.for_config(2)
    host = np.empty((n, STRIDE), dtype=np.uint8)
    bufs = []
    for b in range(4):  # four placements in HBM, rotated: one batch's placement does not set the figure
        pa.gen_frames(p, n, STRIDE, 2, first_index=b * n, threads=min(16, cpu_threads()), out=host)
        bufs.append(torch.from_numpy(host.reshape(-1)).cuda())
    del host
    span = 1514 + 8  # the frame and its pad byte, moved as one piece
    cur = [2]

    def place(off):  # the frames of both buffers to frame_off `off`, in place
        if off != cur[0]:
            for d in bufs:
                v = d.view(n, STRIDE)
                v[:, off:off + span] = v[:, cur[0]:cur[0] + span].clone()
            cur[0] = off
            torch.cuda.synchronize()

    def fill(d, off):
        ctx.tx_fill(d, STRIDE, off, n, None, pa.PN_TX_TCP, stream)

    checks = {}
    for off in (2, 14):
        place(off)
        v = bufs[0].view(n, STRIDE)
        orig = bufs[0].clone()
        exp = v[:4096].cpu().numpy().copy()
        v[:, off + 24:off + 26] = 0x5A  # ip checksum
        v[:, off + 50:off + 52] = 0xA5  # tcp checksum
        fill(bufs[0], off)
        torch.cuda.synchronize()
        diff = (bufs[0].view(n, STRIDE) != orig.view(n, STRIDE)).any(dim=1)
        bad = torch.nonzero(diff).flatten().cpu().numpy()
        got = v[:4096].cpu().numpy()
        exp[:, off + 24:off + 26] = 0x5A
        exp[:, off + 50:off + 52] = 0xA5
        orc.tx_fill_batch(exp, STRIDE, off, 4096, None, orc.TX_TCP)
        checks[off] = {"first_4096_vs_oracle": bool(np.array_equal(got, exp)),
                       "frames_changed_vs_valid_original": int(len(bad)),
                       "only_corrupted_frames_differ": bool(len(bad) == n // 1024 and np.all(bad % 1024 == bad[0] % 1024))}
        del orig
    ks = {2: [], 14: []}
    abl = {2: [], 14: []}
    for r in range(rounds):  # product and ablated ceiling alternately (the ceiling's fields are garbage; the fill
        # recomputes both from the frame bytes, so the product's timing is unaffected)
        for off in ((2, 14) if r % 2 == 0 else (14, 2)):
            place(off)
            ks[off].append(time_launches(torch, lambda d: fill(d, off), bufs, steps, stream))
            abl[off].append(time_launches(torch, lambda d: tn.calib_tx_ablated(ctx, d, STRIDE, off, n, stream), bufs,
                                          steps, stream))
    for off in (2, 14):
        kern, kabl = statistics.median(ks[off]), statistics.median(abl[off])
        algo = 1504 * n
        tr = load_pmc("tx_c2_n1048576", f"frame_off_{off}")
        out[f"frame_off_{off}"] = {
            "kernel": "tx_fill_kernel + tx_patch_kernel (one pn_tx_fill call)", "frames": n, "resident_batches": 4,
            "kernel_ms": round(kern, 5), "kernel_ms_rounds": [round(x, 5) for x in ks[off]],
            "gbit_per_s": round(8 * 1514 * n / (kern * 1e-3) / 1e9, 1),
            "algorithmic_bytes_per_launch": algo, "achieved_gbs": round(algo / (kern * 1e-3) / 1e9, 1),
            "frac": round(algo / (kern * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "ablated_kernel_ms": round(kabl, 5), "kernel_vs_ablated_ceiling": round(kabl / kern, 4),
            "at_ceiling_within_spread": abs(1 - kabl / kern) <= max((max(ks[off]) - min(ks[off])) / kern, 0.002),
            **pmc_fields(tr),
            "write_requests_per_frame": None if not (tr and tr["code_current"]) else tr.get("ea_write_requests_per_frame"),
            "write_64B_per_frame": None if not (tr and tr["code_current"]) else tr.get("ea_write_64B_per_frame"),
            **checks[off]}
    r14 = [a / b for a, b in zip(ks[14], ks[2])]
    out["same_buffers_off14_over_off2"] = {
        "ratio_median": round(statistics.median(r14), 4), "ratio_per_round": [round(x, 4) for x in r14],
        "write_requests_per_frame_off2_off14": [out["frame_off_2"]["write_requests_per_frame"],
                                               out["frame_off_14"]["write_requests_per_frame"]],
        "note": "the same four resident buffers at both layouts (frames moved in place), rounds alternating the order"}
    del bufs
    torch.cuda.empty_cache()
    ctx.close()
    return out


def secondary_release_path(torch, pa, ctx, frames_b, res, n, steps, stream):
    """C2 through the release path (pn_set_verify(ctx, 0): Core::checksum is debug-only in the reference,
    Core.h:448-478): the kernel reads each frame's 128-B header line instead of the whole frame.  Same rotating
    resident batches; batch 0's records must equal the full path's (already oracle-gated) with the TCP verdict
    taken out.  Algorithmic bytes per frame: the 64-B header window read + the 16-B record."""
    F = pa.rx.F
    ctx.classify(frames_b[0], STRIDE, FRAME_OFF, n, res, stream)
    torch.cuda.synchronize()
    full = res.cpu().numpy().view(pa.RESULT_DTYPE).copy()
    ctx.set_verify(False)
    try:
        ctx.classify(frames_b[0], STRIDE, FRAME_OFF, n, res, stream)
        torch.cuda.synchronize()
        got = res.cpu().numpy().view(pa.RESULT_DTYPE)
        exp = full.copy()
        exp["flags"] = (exp["flags"] & ~np.uint16(F.TCP_OK | F.RFC_TCP_OK)) | np.uint16(F.TCP_UNCHECKED)
        exp["tcp_fold"] = 0xFFFF
        ok = bool(np.array_equal(got, exp))
        kern = time_launches(torch, lambda d: ctx.classify(d, STRIDE, FRAME_OFF, n, res, stream), frames_b, steps, stream)
    finally:
        ctx.set_verify(True)
    algo = n * (64 + 16)
    pmc = load_pmc(f"c2_release_path_n{n}")
    return {"kernel_ms": round(kern, 5), "mframes_per_s": round(n / (kern * 1e-3) / 1e6, 1),
            **pmc_fields(pmc),
            "algorithmic_bytes_per_launch": algo, "achieved_gbs": round(algo / (kern * 1e-3) / 1e9, 1),
            "frac": round(algo / (kern * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "line_traffic_gbs": round(n * (128 + 16) / (kern * 1e-3) / 1e9, 1),
            "records_equal_full_path_less_tcp_verdict": ok,
            "note": "pn_set_verify(ctx, 0) on the rotating C2 batches: one 128-B header line read per frame (the "
                    "64-B window block inside it), no TCP checksum; DESIGN §4"}


def secondary_service_large_post(torch, pa, ctx, frames_b, res, n, stream, reps=15):
    """A 1-Mi-frame post to the resident classify service (pn_service_*) against pn_classify on the same
    rotating device-resident C2 batches, verified and release path: host wall clock from the post (launch) to the
    records being complete (pn_service_wait / stream sync), median of `reps`.  The service as opened by default
    (the latency tier + helper waves launched with a large post) and with the latency tier alone (large_waves 64,
    the round-5 service).  Every post's records must equal pn_classify's."""
    out = {"frames": n, "reps": reps,
           "note": "host wall clock post -> complete (service) vs launch -> stream sync (pn_classify), device memory"}
    out_b = torch.empty_like(res)
    for verify in (True, False):
        ctx.set_verify(verify)
        try:
            leg = {}

            def classify_once(k):
                t = time.perf_counter()
                ctx.classify(frames_b[k % len(frames_b)], STRIDE, FRAME_OFF, n, res, stream)
                torch.cuda.synchronize()
                return time.perf_counter() - t

            for k in range(3):
                classify_once(k)
            leg["pn_classify_ms"] = round(statistics.median(classify_once(k) for k in range(reps)) * 1e3, 4)
            for name, lw in (("service_default", 0), ("service_latency_tier_only", pa.PN_SERVICE_WAVES)):
                svc = pa.RxService(ctx, STRIDE, FRAME_OFF, idle_ms=1000, large_waves=lw)
                try:
                    def post_once(k):
                        t = time.perf_counter()
                        svc.post(frames_b[k % len(frames_b)], n, out_b)
                        svc.wait()
                        return time.perf_counter() - t

                    for k in range(3):
                        post_once(k)
                    ms = statistics.median(post_once(k) for k in range(reps)) * 1e3
                    ctx.classify(frames_b[0], STRIDE, FRAME_OFF, n, res, stream)
                    torch.cuda.synchronize()
                    svc.post(frames_b[0], n, out_b)
                    svc.wait()
                    leg[name] = {"ms": round(ms, 4), "vs_pn_classify": round(ms / leg["pn_classify_ms"], 3),
                                 "records_equal_pn_classify": bool(torch.equal(out_b, res))}
                finally:
                    svc.close()
            out["verified" if verify else "release_path"] = leg
        finally:
            ctx.set_verify(True)
    return out


def secondary_c4_shard(torch, pa, ctx_dev, steps, R, stream):
    """The N>1 workload on this one GPU: rank 0's C4 shard (BASELINE configs[3], 2 Mi x 1514-B frames over
    1024 flows = global frames [0, 2 Mi) of 16 Mi), R rotating resident copies, timed exactly as each rank
    times it at N>1 (HIP events around the K launches), sha256-gated against c4_shards[0].  The same-workload
    denominator for the 1->8-GPU curve (the headline at N=1 is C2, at N>1 C4)."""
    p = pa.rx.GenParams.for_config(4)
    table = pa.gen_conn_table(p)
    ctx = pa.RxContext(ctx_dev)
    ctx.set_conn_table(table)
    n = 1 << 21
    host = np.empty((n, STRIDE), dtype=np.uint8)
    pa.gen_frames(p, n, STRIDE, FRAME_OFF, first_index=0, threads=min(16, cpu_threads()), out=host)
    wire = pa.wire_bytes(host, STRIDE, FRAME_OFF, n)
    bufs = [torch.from_numpy(host.reshape(-1)).cuda()]
    del host
    for _ in range(1, R):
        bufs.append(bufs[0].clone())
    res = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    gd = golden_digest(4, 0, n)
    sha = []
    for b in bufs:
        ctx.classify(b, STRIDE, FRAME_OFF, n, res, stream)
        torch.cuda.synchronize()
        sha.append(gd is not None and hashlib.sha256(res.cpu().numpy().tobytes()).hexdigest() == gd["records_sha256"])
    kern = time_launches(torch, lambda d: ctx.classify(d, STRIDE, FRAME_OFF, n, res, stream), bufs, steps, stream)
    algo = int(wire) + 16 * n
    ctx.close()
    del bufs, res
    torch.cuda.empty_cache()
    return {"workload": WORKLOADS[4] + ": rank 0's shard, global frames [0, 2 Mi)", "frames": n,
            "resident_batches": R, "kernel_ms": round(kern, 5),
            "value": round(8 * wire / (kern * 1e-3) / 1e9, 2), "unit": "Gbit/s",
            "mframes_per_s": round(n / (kern * 1e-3) / 1e6, 2),
            "algorithmic_bytes_per_launch": algo, "frac": round(algo / (kern * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "batches_sha256_gated": f"{len(sha) if gd is not None else 0}/{R}",
            "gated_batches_sha256_match_golden": bool(gd is not None and all(sha)),
            "note": "the per-GPU workload of the N>1 line, on one GPU: N x this value is the ideal N-GPU aggregate"}


def e2e_host_ring(torch, pa, ctx, ring, n, got0, stream, dist, barrier, world, rank, numa, passes=5):
    """The end-to-end leg on every rank: the node's one host ring (pollnet_amd/host_ring.py), each rank's
    shard first-touched on its GPU's NUMA node and hipHostRegister-ed, classified in place by that rank's GPU
    (zero copy), the records written into the ring's shared record array.  Both modes: checksums verified (each
    frame's lines cross PCIe) and the release path (pn_set_verify(ctx, 0): one header line per frame).  Timed over
    one common window per mode (max over ranks), `passes` launches over the whole shard; value = all ranks' wire
    bytes / that window.  Every rank's records must equal its device-resident records of the same frames (already
    gated against the committed digests), with the TCP verdict taken out in release mode."""
    from pollnet_amd.shard import common_window

    reg_error = None
    try:
        ring.register()
    except Exception as ex:  # e.g. a pinning limit: every rank learns it before any barrier
        reg_error = f"rank {rank}: {ex!r}"
    if world > 1:
        errs = [None] * world
        dist.all_gather_object(errs, reg_error)
        reg_error = next((e for e in errs if e), None)
    if reg_error:
        return {"error": f"hipHostRegister of the shared ring failed: {reg_error}"}
    shard_ptr, rec_ptr = ring.addresses()
    wire = float(pa.wire_bytes(ring.shard(), STRIDE, FRAME_OFF, n))
    F = pa.rx.F
    out = {"note": "one host ring in POSIX shared memory, rank r's index shard first-touched from its GPU's NUMA node "
                   "and hipHostRegister-ed; pn_classify reads it in place over PCIe and writes the 16-B records into "
                   "the ring's shared record array (pollnet_amd/host_ring.py)", "passes": passes,
           "frames_per_rank": n}
    try:
        for mode in ("verified", "release_path"):
            ctx.set_verify(mode == "verified")
            ctx.classify(shard_ptr, STRIDE, FRAME_OFF, n, rec_ptr, stream)  # warm: TLB / page-table walk of the range
            torch.cuda.synchronize()
            t_own = [0.0]

            def body():
                t0 = time.perf_counter()
                for _ in range(passes):
                    ctx.classify(shard_ptr, STRIDE, FRAME_OFF, n, rec_ptr, stream)
                torch.cuda.synchronize()
                t_own[0] = time.perf_counter() - t0

            wall, _ = common_window(body, dist if world > 1 else None, barrier)
            exp = np.ascontiguousarray(got0).view(pa.RESULT_DTYPE).copy()
            if mode == "release_path":
                exp["flags"] = (exp["flags"] & ~np.uint16(F.TCP_OK | F.RFC_TCP_OK)) | np.uint16(F.TCP_UNCHECKED)
                exp["tcp_fold"] = 0xFFFF
            ok = bool(np.array_equal(ring.records().view(pa.RESULT_DTYPE), exp))
            # bytes the path needs across PCIe per frame: the frame + its record (verified), the 64-B header window
            # + the record (release); the line-granular bytes are up to 1.02x / 1.8x that
            need = (wire + 16 * n) if mode == "verified" else n * (64 + 16)
            mine = {"rank": rank, "numa_node": numa, "own_s": round(t_own[0], 5),
                    "needed_bytes_gb_per_s": round(need * passes / t_own[0] / 1e9, 2), "records_ok": ok}
            ranks = [mine]
            total_wire = wire
            if world > 1:
                ranks = [None] * world
                dist.all_gather_object(ranks, mine)
                w = torch.tensor([wire], dtype=torch.float64)
                dist.all_reduce(w, op=dist.ReduceOp.SUM)
                total_wire = float(w[0])
            out[mode] = {"gbit_per_s": round(total_wire * passes * 8 / wall / 1e9, 2),
                         "mframes_per_s": round(n * world * passes / wall / 1e6, 2),
                         "window_s": round(wall, 5), "every_rank_records_ok": all(r["records_ok"] for r in ranks),
                         "ranks": ranks}
    finally:
        ctx.set_verify(True)
    return out


def summary(out):
    """The line's figures a reader needs first, compact: kernel fractions of the 8 TB/s roofline, the per-GPU
    workload of the N>1 line, the release-path kernels, the CPU baselines with their spread, the host-ring rates."""
    def g(d, *path):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return d

    sec = out.get("secondary", {})
    cpu = out.get("cpu_baseline", {})
    s = {"value": out["value"], "unit": out["unit"], "n_gpus": out["n_gpus"], "frac": g(out, "roofline", "frac"),
         "kernel_ms": g(out, "roofline", "kernel_ms_avg"), "traffic_stale": g(out, "roofline", "traffic_stale"),
         "verified": out.get("verified_vs_oracle")}
    if sec:
        s.update({
            "c3_frac": g(sec, "c3", "frac"), "c5_frac": g(sec, "c5", "frac"),
            "c3_c5_traffic_over_stream_read": [g(sec, "c3", "traffic_rate_over_stream_read"),
                                               g(sec, "c5", "traffic_rate_over_stream_read")],
            "c4_shard_gbit_per_s": g(sec, "c4_shard", "value"), "c4_shard_kernel_ms": g(sec, "c4_shard", "kernel_ms"),
            "tx_off2_frac": g(sec, "tx_fill", "frame_off_2", "frac"), "tx_off14_frac": g(sec, "tx_fill", "frame_off_14", "frac"),
            "tx_off2_ms": g(sec, "tx_fill", "frame_off_2", "kernel_ms"),
            "tx_off14_ms": g(sec, "tx_fill", "frame_off_14", "kernel_ms"),
            "tx_off14_over_off2_same_buffers": g(sec, "tx_fill", "same_buffers_off14_over_off2", "ratio_median"),
            "match_streams_ms": g(sec, "match_streams", "kernel_ms"),
            "release_path_ms": g(sec, "c2_release_path", "kernel_ms"),
            "service_1mi_post_vs_pn_classify_verified_release": [
                g(sec, "service_large_post", "verified", "service_default", "vs_pn_classify"),
                g(sec, "service_large_post", "release_path", "service_default", "vs_pn_classify")],
            "server_512_mfps": g(sec, "tcp_server_poll", "gpu_rxbatch_512", "mframes_per_s"),
            "server_512_release_mfps": g(sec, "tcp_server_poll", "gpu_rxbatch_512_release_path", "mframes_per_s"),
            "server_cpu_512_mfps": g(sec, "tcp_server_poll", "cpu_rxbatch_512", "mframes_per_s"),
            "server_512_pipelined_mfps": g(sec, "tcp_server_poll", "gpu_rxbatch_512_pipelined", "mframes_per_s"),
            "server_512_pipelined_release_mfps": g(sec, "tcp_server_poll", "gpu_rxbatch_512_pipelined_release_path",
                                                   "mframes_per_s"),
            "server_512_resident_mfps": g(sec, "tcp_server_poll", "gpu_rxbatch_512_resident", "mframes_per_s"),
            "server_512_resident_release_mfps": g(sec, "tcp_server_poll", "gpu_rxbatch_512_resident_release_path",
                                                  "mframes_per_s"),
            "server_512_pipelined_resident_mfps": g(sec, "tcp_server_poll", "gpu_rxbatch_512_pipelined_resident",
                                                    "mframes_per_s"),
            "server_512_pipelined_resident_release_mfps": g(sec, "tcp_server_poll",
                                                            "gpu_rxbatch_512_pipelined_resident_release_path",
                                                            "mframes_per_s"),
            "server_cpu_512_release_mfps": g(sec, "tcp_server_poll", "cpu_rxbatch_512_release_path", "mframes_per_s"),
            "server_reference_release_mfps": g(sec, "tcp_server_poll", "reference_server_release_build", "mframes_per_s"),
            "server_hot_frames_resident_vs_reference_mfps": [
                g(sec, "tcp_server_poll", "hot", "gpu_rxbatch_512_pipelined_resident_release_path", "mframes_per_s_server_only")
                or g(sec, "tcp_server_poll", "gpu_rxbatch_512_pipelined_resident_release_path", "mframes_per_s_server_only"),
                g(sec, "tcp_server_poll", "hot", "reference_server_release_build", "mframes_per_s_server_only")
                or g(sec, "tcp_server_poll", "reference_server_release_build", "mframes_per_s_server_only")],
            "server_hot_pair_median3_mfps": [
                g(sec, "tcp_server_poll", "hot", "gpu_rxbatch_512_pipelined_resident_release_path", "mframes_per_s"),
                g(sec, "tcp_server_poll", "hot", "reference_server_release_build", "mframes_per_s")],
            "server_l3_frames_resident_vs_reference_mfps": [
                g(sec, "tcp_server_poll", "l3", "gpu_rxbatch_512_pipelined_resident_release_path",
                  "mframes_per_s_server_only"),
                g(sec, "tcp_server_poll", "l3", "reference_server_release_build", "mframes_per_s_server_only")],
            "server_cold_frames_resident_vs_reference_mfps": [
                g(sec, "tcp_server_poll", "cold", "gpu_rxbatch_512_pipelined_resident_release_path",
                  "mframes_per_s_server_only"),
                g(sec, "tcp_server_poll", "cold", "reference_server_release_build", "mframes_per_s_server_only")],
            "zero_copy_64_us_notify_vs_service": [g(sec, "small_batch_latency", "zero_copy", "64", "signal_us"),
                                                  g(sec, "small_batch_latency", "zero_copy", "64", "service_us")],
            "zero_copy_64_release_us_notify_vs_service": [
                g(sec, "small_batch_latency", "zero_copy_release_path", "64", "signal_us"),
                g(sec, "small_batch_latency", "zero_copy_release_path", "64", "service_us")],
            "service_release_device_us_64_512_1024": [
                g(sec, "small_batch_latency", "resident_release_path", m, "service_us") for m in ("64", "512", "1024")]})
    if cpu:
        s.update({"cpu_ref_gbit_per_s": cpu.get("value"), "cpu_ref_min_max": [cpu.get("min"), cpu.get("max")],
                  "cpu_ref_cores": cpu.get("cores"), "cpu_ref_consistent_with_sweep": cpu.get("consistent_with_sweep"),
                  "cpu_ref_release_gbit_per_s": g(cpu, "release_path", "value"),
                  "cpu_ref_release_min_max": [g(cpu, "release_path", "min"), g(cpu, "release_path", "max")],
                  "cpu_ref_release_cores": g(cpu, "release_path", "cores")})
    for k in ("e2e_pinned_host", "e2e_zero_copy_pinned_host", "e2e_zero_copy_pinned_host_release_path"):
        if k in out:
            s[k + "_gbit_per_s"] = g(out, k, "gbit_per_s")
    if "e2e_host_ring" in out:
        s["e2e_host_ring_gbit_per_s"] = g(out, "e2e_host_ring", "verified", "gbit_per_s")
        s["e2e_host_ring_release_gbit_per_s"] = g(out, "e2e_host_ring", "release_path", "gbit_per_s")
        s["e2e_host_ring_records_ok"] = (g(out, "e2e_host_ring", "verified", "every_rank_records_ok") and
                                         g(out, "e2e_host_ring", "release_path", "every_rank_records_ok"))
    return s


def device_identity(torch, dev):
    """The physical device a rank ran on (PCI domain:bus:device, name, uuid)."""
    pr = torch.cuda.get_device_properties(dev)
    return {"device_ordinal": dev,
            "pci_bus_id": f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}",
            "name": pr.name, "uuid": str(getattr(pr, "uuid", ""))}


def peak_rss_mib():
    import resource

    return round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1)


DUMP_ROWS = 1 << 20  # records written by --dump-outputs over all ranks: 6 float64 each = 48 MiB
DUMP_SEED = 20240611


def dump_outputs(path, res, n, rank, world):
    """--dump-outputs: what the timed path left in its caller's record buffer after the last timed step, one row
    per frame and one float64 column per field of the 16-B record (conn_id, seq, payload_off, payload_len, flags,
    tcp_fold: every field is exact in a float64).  At most DUMP_ROWS rows over all ranks: of a larger output a
    fixed, seeded sample of rows in ascending order, whose indices go beside it."""
    import pollnet_amd as pa

    os.makedirs(path, exist_ok=True)
    name = "records" if world == 1 else f"records_rank{rank}"
    rec = res.cpu().numpy().view(pa.RESULT_DTYPE)[:n]
    rows = max(1, DUMP_ROWS // world)
    if n > rows:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, rows, replace=False))
        np.save(os.path.join(path, name + "_rows.npy"), idx.astype(np.float64))
        rec = rec[idx]
    cols = np.empty((len(rec), len(pa.RESULT_DTYPE.names)), dtype=np.float64)
    for c, f in enumerate(pa.RESULT_DTYPE.names):
        cols[:, c] = rec[f]
    np.save(os.path.join(path, name + ".npy"), cols)
    return {"dir": path, "file": name + ".npy", "rows": len(rec), "of": n, "columns": list(pa.RESULT_DTYPE.names),
            "batch": "the resident batch of the last timed step"}


# ----------------------------------------------------------------------------- ranks
def _json_stdout():
    """stdout carries the one JSON line only: fd 1 is pointed at stderr for everything else
    (gloo's C++ connection log, library prints) and the line goes to the saved original."""
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    return os.fdopen(saved, "w")


def run_rank(rank, world, local_rank, args):
    t_rank = time.perf_counter()
    json_out = _json_stdout()
    import torch
    import torch.distributed as dist

    import pollnet_amd as pa
    from pollnet_amd.shard import ShmBarrier, common_window, shard_range

    ndev = max(1, torch.cuda.device_count())
    dev = local_rank % ndev
    torch.cuda.set_device(dev)
    if world > 1:  # host-side coordination only: barriers and two scalar reductions (no RCCL)
        dist.init_process_group("gloo", rank=rank, world_size=world)

    # N=1: BASELINE configs[1] (C2, 1 Mi single-flow frames).  N>1: configs[3] (C4, 16 Mi frames over
    # 1024 flows sharded by index across 8 GPUs = 2 Mi per GPU; rank r owns global [r*2Mi, (r+1)*2Mi)).
    cfg = args.config or (2 if world == 1 else 4)
    n = args.frames or ((1 << 21) if cfg == 4 else (1 << 20))
    params = pa.rx.GenParams.for_config(cfg)
    lo, _ = shard_range(rank, world, n)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    gen_threads = max(1, min(16, cpu_threads() // max(1, local_world)))
    t0 = time.perf_counter()
    R = max(1, args.batches)
    table = pa.gen_conn_table(params)
    entries, mask = table.snapshot()
    ctx = pa.RxContext(dev)
    ctx.set_conn_table(table)
    # R resident batches per rank, rotated over by the timed steps.  N=1: batch b holds global frames
    # [b*n, (b+1)*n) (distinct content).  N>1: batch 0 is this rank's index shard, generated on the
    # host; batches 1.. are device copies of it at other HBM addresses (a 4-GiB batch is ~16x the
    # memory-side cache, so a copy is as cold as new content), so every timed batch is the rank's own
    # shard and is gated against that shard's committed digest.
    firsts = [b * n if world == 1 else lo for b in range(R)]
    # the node's one host ring (pollnet_amd/host_ring.py): rank r's batch 0 is generated straight into its shard,
    # from CPUs of its GPU's NUMA node (first touch places the pages there), for the end-to-end leg
    ring, numa_node, numa_cpus, ring_error = None, -1, [], None
    if not args.no_e2e:
        from pollnet_amd.host_ring import SharedHostRing, device_numa

        pr = torch.cuda.get_device_properties(dev)
        numa_node, numa_cpus = device_numa(pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        try:
            ring = SharedHostRing(dist if world > 1 else None, rank, world, n, STRIDE)
        except RuntimeError as ex:  # every rank gets the same verdict from rank 0: the leg is skipped everywhere
            ring, ring_error = None, str(ex)
            log(f"[rank {rank}] e2e host ring skipped: {ex}")
    frames_b, wires = [], []
    host = np.empty((n, STRIDE), dtype=np.uint8) if (R > 1 and world == 1) or ring is None else None
    slots = None
    for b in range(R):
        if world > 1 and b > 0:
            frames_b.append(frames_b[0].clone())
            wires.append(wires[0])
            continue
        dst = ring.shard() if (b == 0 and ring is not None) else host
        from pollnet_amd.host_ring import cpu_affinity

        with cpu_affinity(numa_cpus if dst is not host else []):
            pa.gen_frames(params, n, STRIDE, FRAME_OFF, first_index=firsts[b], threads=gen_threads, out=dst)
        wires.append(pa.wire_bytes(dst, STRIDE, FRAME_OFF, n))
        frames_b.append(torch.from_numpy(dst.reshape(-1)).to(f"cuda:{dev}"))
        if b == 0 and args.full:
            # N=1 keeps batch 0 on the host (CPU baseline, e2e legs); N>1 ranks keep only the rows
            # the in-run oracle check reads
            if world == 1:
                slots = dst if dst is not host else host.copy()
            else:
                slots = dst[: min(n, 4096)].copy()
    del host
    frames = frames_b[0]
    log(f"[rank {rank}] device {dev}: C{cfg} shard [{lo}, {lo + n}), {R} x {n} frames "
        f"({sum(wires) / 1e9:.2f} GB wire) in {time.perf_counter() - t0:.1f}s")

    res = torch.empty(n * 16, dtype=torch.uint8, device=f"cuda:{dev}")
    stream = torch.cuda.current_stream()

    # correctness gate on the measured configuration, on every rank: each batch's records must satisfy
    # the workload's invariants; each batch whose global frame range has a committed digest (made by the
    # oracle: C2/C3/C5 [0, 1 Mi), each of C4's 8 shards) must hash to it; the first 4096 records of
    # batch 0 are re-checked against the oracle in this run
    gate = {"checked": False, "note": "the gate against the oracle and the committed digests runs with --full"}
    verified, fully_gated, got0 = False, False, None
    if args.full:
        inv_ok = True
        sha_ok, sha_gated = True, 0
        for b in range(R):
            ctx.classify(frames_b[b], STRIDE, FRAME_OFF, n, res, stream)
            torch.cuda.synchronize()
            rec = res.view(n, 16)
            flags = rec[:, 12].to(torch.int32) | (rec[:, 13].to(torch.int32) << 8)
            if cfg in (2, 4):  # every frame: valid IP header, a known flow, 54-B headers + 1460-B payload
                off_len = rec[:, 8:12].contiguous().view(torch.int32).flatten()
                inv_ok &= bool(torch.all((flags & 0x5) == 0x5)) and bool(torch.all(off_len == (54 | (1460 << 16))))
            else:
                inv_ok &= bool(torch.all((flags & 0x4000) == 0))
            host_rec = res.cpu().numpy()
            gd = golden_digest(cfg, firsts[b], n)
            if gd is not None:
                sha_gated += 1
                sha_ok &= hashlib.sha256(host_rec.tobytes()).hexdigest() == gd["records_sha256"]
            if b == 0:
                got0 = host_rec
        from oracle import pyoracle as orc

        k = min(n, 4096)
        exp = orc.classify_batch(slots, STRIDE, FRAME_OFF, k, entries, mask, table.max_conn_cnt, threads=8)
        gate = {"all_batches_invariants": inv_ok, "batches_sha256_gated": f"{sha_gated}/{R}",
                # None: no committed digest covers this frame range (e.g. a --frames override)
                "gated_batches_sha256_match_golden": bool(sha_ok) if sha_gated else None,
                "batch0_first_4096_vs_oracle": bool(np.array_equal(got0[: k * 16].view(pa.RESULT_DTYPE), exp))}
        verified = all(v for v in gate.values() if isinstance(v, bool))
        # without a committed digest for its frames a rank is checked by invariants and 4096 records only:
        # that is reported as "partial", never as verified
        fully_gated = sha_gated == R
        if not verified:
            log(f"ERROR [rank {rank}]: correctness gate failed: {gate}")
    setup_s = round(time.perf_counter() - t_rank, 1)

    for w in range(args.warmup):
        ctx.classify(frames_b[w % R], STRIDE, FRAME_OFF, n, res, stream)
    torch.cuda.synchronize()
    # one common window (pollnet_amd.shard.common_window): every rank opens it when the start barrier
    # releases and closes it after the end barrier, so each rank's window covers the slowest rank's last
    # launch; value = all ranks' bytes / the max over ranks of that window
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed_steps():
        ev0.record(stream)
        for k in range(args.steps):
            ctx.classify(frames_b[k % R], STRIDE, FRAME_OFF, n, res, stream)
        ev1.record(stream)
        torch.cuda.synchronize()

    # ranks on one node (the driver's launch) meet at a shared-memory barrier (microseconds); across nodes, gloo's
    shm_barrier = None
    if world > 1 and int(os.environ.get("LOCAL_WORLD_SIZE", str(world))) == world:
        shm_barrier = ShmBarrier(dist, rank, world)
    wall_max, own_max = common_window(timed_steps, dist if world > 1 else None, shm_barrier)
    kern_ms = ev0.elapsed_time(ev1) / args.steps
    dumped = dump_outputs(args.dump_outputs, res, n, rank, world) if args.dump_outputs else None
    gate.update(device_identity(torch, dev))
    gate.update({"kernel_ms": round(kern_ms, 5), "setup_s": setup_s, "peak_rss_mib": peak_rss_mib()})
    step_wire = float(sum(wires[k % R] for k in range(args.steps)))  # this rank's wire bytes over the K steps
    total_wire, kern_ms_max, all_verified, all_gated = step_wire, kern_ms, verified, fully_gated
    gates = [gate]
    if world > 1:
        t = torch.tensor([kern_ms, 0.0 if verified else 1.0, 0.0 if fully_gated else 1.0], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        kern_ms_max, all_verified, all_gated = float(t[0]), float(t[1]) == 0.0, float(t[2]) == 0.0
        w = torch.tensor([step_wire], dtype=torch.float64)
        dist.all_reduce(w, op=dist.ReduceOp.SUM)
        total_wire = float(w[0])
        gates = [None] * world
        dist.all_gather_object(gates, {"rank": rank, "shard": [lo, lo + n], **gate})
    e2e = None
    if ring is not None:
        try:
            e2e = e2e_host_ring(torch, pa, ctx, ring, n, got0, stream, dist, shm_barrier, world, rank, numa_node)
        except Exception as ex:  # measured extra; never blocks the bench line
            e2e = {"error": repr(ex)}
    total_frames = n * world * args.steps
    gbit = total_wire * 8 / wall_max / 1e9
    mfps = total_frames / wall_max / 1e6

    out = None
    if rank == 0:
        # every frame byte read once + the 16-B record written, averaged over the launches timed
        algo_bytes = int(step_wire / args.steps) + 16 * n
        achieved = algo_bytes / (kern_ms * 1e-3) / 1e9
        pmc = load_pmc(f"c{cfg}_n{n}")
        out = {
            "metric": METRIC,
            "value": round(gbit, 2),
            "unit": "Gbit/s",
            "mframes_per_s": round(mfps, 2),
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(wall_max * 1e3 / args.steps, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u16/u32 integer (one's-complement sums)",
            "data": "synthetic (deterministic seeded generator, pollnet_amd/csrc/framegen.cpp)",
            "config": {"workload": WORKLOADS[cfg], "frames_per_gpu": n, "slot_stride": STRIDE, "frame_off": FRAME_OFF,
                       "parallelism": f"index-sharded x{world}, no collective", "global_frames": n * world,
                       "resident_batches_per_gpu": R, "devices_visible": torch.cuda.device_count(),
                       "ranks_per_device": -(-world // ndev) if world > ndev else 1,
                       "coordination": "gloo (host): setup, max/sum of the timing, gates; the timed window between "
                                       "start/stop barriers" if world > 1 else
                       "single process"},
            "full": bool(args.full),
            # null: not checked in this run (the gate is one of --full's legs)
            "verified_vs_oracle": None if not args.full else (
                bool(all_verified) if all_gated or not all_verified else "partial"),
            "correctness_gate": gate if world == 1 else {
                "every_rank_verified": bool(all_verified) if args.full else None,
                "every_rank_sha256_gated": bool(all_gated) if args.full else None,
                "distinct_devices": len({g["pci_bus_id"] for g in gates}),
                "setup_s_max": max(g["setup_s"] for g in gates),
                "peak_rss_mib_max": max(g["peak_rss_mib"] for g in gates), "ranks": gates},
            "timing": ("one common window: max over ranks of start barrier -> end barrier (the end barrier inside "
                       "the window; " + ("shared-memory barrier, one node)" if shm_barrier is not None else "gloo barrier)")
                       if world > 1 else "wall clock around the K launches + device sync"),
            "rank_own_wall_ms_max": round(own_max * 1e3, 4),
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4),
                         **pmc_fields(pmc),
                         "kernel": "rx_classify_kernel", "kernel_ms_avg": round(kern_ms, 5),
                         "kernel_ms_avg_max_over_ranks": round(kern_ms_max, 5),
                         "algorithmic_bytes_per_launch": algo_bytes,
                         "bytes_per_frame": round(algo_bytes / n, 2)},
        }
    if rank == 0 and e2e is not None:
        out["e2e_host_ring"] = e2e
    elif rank == 0 and ring_error:
        out["e2e_host_ring"] = {"error": ring_error}
    if rank == 0 and dumped is not None:
        out["dumped_outputs"] = dumped
    if rank == 0 and world == 1 and args.full:
        out["roofline"]["same_run_ceilings"] = ceilings(torch, ctx, frames_b, n, res, stream,
                                                        stream_only=args.stream_ceiling_only)
    if rank == 0 and world == 1 and not args.no_secondary and cfg == 2 and n == 1 << 20:
        t_sec = time.perf_counter()
        sec = {}
        try:  # on the rotating C2 batches, before they are released
            sec["match_streams"] = secondary_streams(torch, pa, ctx, frames_b, slots, n, stream)
        except Exception as ex:  # measured extra; never blocks the bench line
            sec["match_streams"] = {"error": repr(ex)}
        try:
            sec["c2_release_path"] = secondary_release_path(torch, pa, ctx, frames_b, res, n, args.steps, stream)
        except Exception as ex:  # measured extra; never blocks the bench line
            sec["c2_release_path"] = {"error": repr(ex)}
        try:
            sec["service_large_post"] = secondary_service_large_post(torch, pa, ctx, frames_b, res, n, stream)
        except Exception as ex:  # measured extra; never blocks the bench line
            sec["service_large_post"] = {"error": repr(ex)}
        del frames_b[1:]  # the C2 batches rotated above are done; make room for the others
        torch.cuda.empty_cache()
        try:
            sec["c4_shard"] = secondary_c4_shard(torch, pa, dev, args.steps, R, stream)
        except Exception as ex:  # measured extra; never blocks the bench line
            sec["c4_shard"] = {"error": repr(ex)}
        try:
            sec["c3"] = secondary_rx(torch, pa, 3, n, 20, stream, packed=True)
            sec["c5"] = secondary_rx(torch, pa, 5, n, 20, stream)
            sec["tx_fill"] = secondary_tx(torch, pa, n, 20, stream)
        except Exception as ex:  # measured extras; never block the bench line
            sec["error"] = repr(ex)
        sec["tcp_server_poll"] = server_poll()
        sec["sniffer_streams"] = sniffer_streams()
        sec["small_batch_latency"] = small_batch_latency()
        sec["seconds"] = round(time.perf_counter() - t_sec, 1)
        out["secondary"] = sec
    if rank == 0 and world == 1 and not args.no_e2e:
        try:
            out["e2e_pinned_host"], _ = e2e_rate(torch, ctx, slots, n)
            if cfg in (2, 4):  # 1514-B frames + pad byte fit 1536-B slots: 25 % less PCIe per frame
                out["e2e_pinned_host_1536B_slots"], _ = e2e_rate(torch, ctx, slots, n, stride=1536)
            out["e2e_zero_copy_pinned_host"], zres = e2e_zero_copy(torch, ctx, slots, n)
            ctx.classify(frames, STRIDE, FRAME_OFF, n, res, stream)  # batch 0 resident, as the zero-copy run read it
            torch.cuda.synchronize()
            if not torch.equal(zres, res.cpu()):
                out["e2e_zero_copy_pinned_host"]["error"] = "records differ from the device-resident run"
            # the release path (pn_set_verify(ctx, 0)): only each frame's header line crosses PCIe
            ctx.set_verify(False)
            try:
                rel, rres = e2e_zero_copy(torch, ctx, slots, n)
            finally:
                ctx.set_verify(True)
            F = pa.rx.F
            exp = res.cpu().numpy().view(pa.RESULT_DTYPE).copy()
            exp["flags"] = (exp["flags"] & ~np.uint16(F.TCP_OK | F.RFC_TCP_OK)) | np.uint16(F.TCP_UNCHECKED)
            exp["tcp_fold"] = 0xFFFF
            rel["records_equal_full_path_less_tcp_verdict"] = bool(np.array_equal(rres.numpy().view(pa.RESULT_DTYPE), exp))
            rel["note"] = ("pn_set_verify(ctx, 0), the reference's release path: pn_classify reads one header line per "
                           "pinned host slot over PCIe, records to pinned host memory")
            out["e2e_zero_copy_pinned_host_release_path"] = rel
        except Exception as ex:  # measured extra; never blocks the bench line
            out["e2e_pinned_host"] = {"error": str(ex)}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(slots, n, entries, mask, table.max_conn_cnt, args.cpu_seconds,
                                           gpu_records=got0)
    if rank == 0:
        if "WORLD_SIZE" not in os.environ or os.environ.get("PN_BENCH_SPAWNED") == "1":
            assert out["n_gpus"] == args.gpus, (out["n_gpus"], args.gpus)
        out["summary"] = summary(out)  # last key: a driver keeping only the line's tail still sees it
        json_out.write(json.dumps(out) + "\n")
        json_out.flush()
    ctx.close()
    del slots
    if ring is not None:
        ring.close(dist if world > 1 else None)
    if shm_barrier is not None:
        shm_barrier.close(dist)
    if world > 1:
        dist.destroy_process_group()


def _spawned(rank, world, args, port):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "LOCAL_WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                       "PN_BENCH_SPAWNED": "1"})
    run_rank(rank, world, rank, args)


def main():
    args = parse()
    if not args.full:  # the plain run: the headline alone
        args.no_secondary = args.no_cpu_baseline = args.no_e2e = True
    if args.e2e:
        args.no_secondary = args.no_cpu_baseline = True
        args.no_e2e = False
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # one process per GPU, started here; the parent never initialises a GPU
        import socket

        import torch.multiprocessing as mp

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        mp.start_processes(_spawned, args=(args.gpus, args, port), nprocs=args.gpus, join=True, start_method="spawn")
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"note: --gpus {args.gpus} but WORLD_SIZE={world}; the launcher's WORLD_SIZE wins")
    run_rank(rank, world, local_rank, args)


if __name__ == "__main__":
    main()
