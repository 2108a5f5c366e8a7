#!/usr/bin/env python3
"""bench.py -- PDQ hashes/s (512x512 RGB8) + 256-bit Hamming Gpairs/s on 1..8 MI355X.

A "step" is one pass of the hot path over one resident batch:
  phase A (-> `value`): PDQ-hash `--images` synthetic 512x512 RGB8 images per GPU (BASELINE config 2:
           100 000 images on 1 GPU; weak scaling: every rank hashes its own 100 000);
  phase C (-> `e2e`):   BASELINE config 4 as ONE timed region over resident images: hash (hash + quality +
           8 dihedral hashes) -> RCCL all-gather of the per-file hash blocks -> every rank sweeps its share of the block
           pairs with the production rule of group_files_generic (8 variants, low-quality rule) -> edges to rank 0 ->
           union-find; the near-duplicate pairs of the synthetic sequence (k % 1000 == 999) must come out as groups.
           N > 1: 1 000 000 images in all, 1 000 000 / N per GPU (config 4 at its stated size; capped at 250 000 per GPU =
           197 GB of pixels, so N = 2 runs 500 000); N = 1: the 100 000 images of phase A;
  phase B (-> `hamming`): all-pairs 256-bit Hamming sweep, threshold 32, over 1M*sqrt(N) synthetic
           hashes (BASELINE config 3 at N=1; per-GPU pair count fixed as N grows): every rank generates
           its shard, one RCCL all-gather of the hash shards, then each rank sweeps its share of the tile pairs;
           (-> `hamming_10m`): BASELINE config 5, strong scaling: 10 000 000 hashes split over the ranks, same steps.
Inputs are generated on the device and resident in HBM before the timed regions.
A plain run measures phase A alone (set-up, --warmup steps, --steps timed steps, the result line); --full adds everything else:
phases C and B, the JPEG leg, the pure read stream of the roofline, the CPU baseline and the reference's own published cases.
--dump-outputs DIR writes the hashes of phase A's last timed step as DIR/pdq_hash.npy (float32, one row of 32 bytes per image;
DIR/pdq_hash_rank<R>.npy per rank when N > 1), so that two builds can be compared output for output on the same seeded images.
One JSON line on rank 0.  Launch: python bench.py [--gpus N --steps K --warmup W].  For N > 1 either start it under
torch.distributed.run (one process per GPU), or just run `python bench.py --gpus N`: with WORLD_SIZE unset it starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child BEFORE anything touches the GPU and exits
with the child's status.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IMG_BYTES = 512 * 512 * 3
ALGO_BYTES_PER_IMAGE = IMG_BYTES + 32          # 786 432 B read + 32 B hash written
HBM_PEAK_GBS = 8000.0                          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9     # 256 CU x 4 SIMD x 32 lanes x 2.4 GHz = 78.6e12 (full-rate VOP2 ops only)
MFMA_I8_OPS_PER_S = 256 * 4 * (32 * 32 * 32 * 2) / 32 * 2.4e9  # v_mfma_i32_32x32x32_i8: 65 536 ops / 32 clk / SIMD = 5.03e15
HAMMING_HBM_BYTES_PER_PAIR = 64.0 / 1024       # 2 T 32 B / T^2 with T = 1024-hash tiles
DUMP_BYTES = 64 << 20                          # --dump-outputs: at most this much over all ranks
ALL_PHASES = {"pdq", "e2e", "hamming", "hamming_10m", "jpeg"}


def cpu_inventory():
    """what the host offers and what the CPU baseline uses (print nproc and hardware_concurrency)"""
    nproc = os.cpu_count() or 1                      # = std::thread::hardware_concurrency()
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else nproc   # = `nproc`
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = max(1, int(int(q) / int(period)))
    except (OSError, ValueError):
        pass
    threads = min(affinity, quota) if quota else affinity
    if os.environ.get("RPH_CPU_THREADS"):
        threads = int(os.environ["RPH_CPU_THREADS"])
    return {"hardware_concurrency": nproc, "nproc_affinity": affinity, "cgroup_cpu_quota": quota, "threads_used": max(1, threads)}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=100_000, help="images per GPU per step")
    ap.add_argument("--hashes", type=int, default=1_000_000, help="hashes at N=1 (scaled by sqrt(N))")
    ap.add_argument("--threshold", type=int, default=32)
    ap.add_argument("--hamming-steps", type=int, default=0, help="default: same as --steps")
    ap.add_argument("--pdq-kernel", type=int, default=1, help="1 = fused, one wave per image, 64-px strips (default), 2 = the same with 128-px strips, "
                    "3 = fused low-latency form (eight waves per image), 0 = generic multi-pass")
    ap.add_argument("--hamming-kernel", type=int, default=2, help="2 = fp4 MFMA fast path (default: popcount-sorted {0,1} operands), 3 = fp4 MFMA with +-1 operands, "
                    "1 = int8 MFMA fast path, 0 = VALU xor + popcount")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend: nccl (= RCCL, default) or gloo (rehearsal: ranks may "
                    "share one GPU, collectives are staged through host memory)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-reference-cases", action="store_true", help="skip the reference's own published cases (keeps a profile of the default "
                    "workloads free of other launches of the same kernels)")
    ap.add_argument("--no-e2e", action="store_true", help="skip phase C (config 4 as one timed region)")
    ap.add_argument("--e2e-steps", type=int, default=3)
    ap.add_argument("--e2e-total", type=int, default=1_000_000, help="images of the e2e leg over all GPUs when N > 1 (BASELINE config 4)")
    ap.add_argument("--e2e-max-per-gpu", type=int, default=250_000, help="cap of resident images per GPU in the e2e leg (250 000 = 197 GB)")
    ap.add_argument("--hashes-strong", type=int, default=10_000_000, help="hashes of the strong-scaling sweep over all GPUs (BASELINE config 5); 0 = skip")
    ap.add_argument("--strong-steps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list of phases to run: pdq, e2e, hamming (default: all)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="CPU time budget per cpu_baseline leg")
    ap.add_argument("--jpeg-files", type=int, default=100_000, help="files per call of the JPEG leg (SURVEY 8f row N3; rank 0 at N = 1 only)")
    ap.add_argument("--jpeg-distinct", type=int, default=4096, help="distinct files of the JPEG leg (the first images of the synthetic sequence, repeated to --jpeg-files)")
    ap.add_argument("--no-jpeg", action="store_true", help="skip the JPEG leg")
    ap.add_argument("--full", action="store_true", help="run every leg and check, not only the timed PDQ steps of the headline figure")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the PDQ hashes of the last timed step under DIR as float32 .npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    only = set(p for p in args.only.split(",") if p)
    if only - ALL_PHASES:
        ap.error(f"--only: unknown phase(s) {sorted(only - ALL_PHASES)}")
    if not args.full and only - {"pdq"}:
        ap.error(f"--only {args.only} needs --full (a plain run times the PDQ phase alone)")
    if args.dump_outputs and only and "pdq" not in only:
        ap.error("--dump-outputs writes the PDQ phase's hashes: --only must include pdq")
    return args


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # self-launch: one process per GPU under torch.distributed.run.  Nothing in THIS process has touched the GPU (torch is
        # not even imported yet), and the parent never execs: it waits for the child and exits with its status.
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    phases = set(p for p in args.only.split(",") if p) or (set(ALL_PHASES) if args.full else {"pdq"})
    if args.hashes_strong <= 0:
        phases.discard("hamming_10m")
    if args.no_e2e:
        phases.discard("e2e")
    if args.no_jpeg:
        phases.discard("jpeg")

    # The CPU oracle (the checker and the cpu_baseline leg) is loaded BEFORE the GPU is initialised and is never built from
    # here: a `make` child of a process that holds the GPU (or runs under a profiler's preload) would be a forbidden exec.
    oracle = None
    want_cpu = rank == 0 and world == 1 and args.full and not args.no_cpu_baseline
    if want_cpu:
        os.environ["RPH_ORACLE_NO_BUILD"] = "1"
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle as oracle_mod

        oracle_mod.lib()  # raises if __graft_entry__.build() has not produced oracle/liboracle_ref.so
        oracle = oracle_mod

    import numpy as np
    import torch

    if args.backend == "gloo":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)  # rehearsal on fewer GPUs than ranks
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))  # RCCL over xGMI
        else:
            dist.init_process_group("gloo")

    from rupphash_amd import Engine
    from rupphash_amd import dist as D

    eng = Engine(local_rank)
    eng.set_pdq_kernel(args.pdq_kernel)
    eng.set_hamming_kernel(args.hamming_kernel)
    dev = torch.device("cuda", local_rank)
    # one explicit (non-null) HIP stream carries the kernels, torch's fills and the RCCL collective, so the
    # HIP events below bracket exactly the work they name
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream
    coll_dev = dev if args.backend == "nccl" else "cpu"

    def barrier_sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def sum_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.int64, device=coll_dev)
        dist.all_reduce(t)
        return int(t.item())

    valid = True
    problems = []
    result = {
        "metric": "pdq_hashes_per_sec_512x512_rgb", "value": None, "unit": "hashes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": None, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "ranks_in_collective": dist.get_world_size() if dist is not None else 1,
        "backend": (str(dist.get_backend()) + (" (RCCL)" if args.backend == "nccl" else "")) if dist is not None else "none (1 process)",
    }

    # ------------------------------------------------------------------ phase A: PDQ hashing
    n_img = args.images
    # the e2e leg (config 4) at N > 1 holds 1 000 000 / N images per GPU (capped); one buffer serves both legs
    e2e_total = n_img if world == 1 else min(args.e2e_total, args.e2e_max_per_gpu * world)
    e2e_lo, e2e_hi = D.shard_range(e2e_total, rank, world)
    n_buf = max(n_img, e2e_hi - e2e_lo) if "e2e" in phases else n_img
    imgs_all = torch.empty((n_buf, IMG_BYTES), dtype=torch.uint8, device=dev)
    imgs = imgs_all[:n_img]
    hashes = torch.empty((n_img, 32), dtype=torch.uint8, device=dev)
    first_k = rank * n_img  # every rank hashes its own contiguous range of the global image sequence
    eng.synth_images_dev(imgs.data_ptr(), first_k, n_img, 512, 512, stream=stream)
    torch.cuda.synchronize()

    def pdq_step():
        eng.pdq_hash_batch_dev(imgs.data_ptr(), n_img, 512, 512, 3, hashes.data_ptr(), stream=stream)

    pdq_sample = None
    if "pdq" in phases:
        for _ in range(args.warmup):
            pdq_step()
        ev = [(eng.event(), eng.event()) for _ in range(args.steps)]
        barrier_sync()
        t0 = time.perf_counter()
        for s in range(args.steps):
            eng.event_record(ev[s][0], stream)
            pdq_step()
            eng.event_record(ev[s][1], stream)
        barrier_sync()
        elapsed = max_over_ranks(time.perf_counter() - t0)
        kernel_ms = [eng.event_elapsed_ms(a, b) for a, b in ev]
        for a, b in ev:
            eng.event_destroy(a)
            eng.event_destroy(b)
        avg_kernel_ms = sum(kernel_ms) / len(kernel_ms)
        value = world * n_img * args.steps / elapsed
        achieved_gbs = ALGO_BYTES_PER_IMAGE * n_img / (avg_kernel_ms * 1e-3) / 1e9
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, hashes, rank, world, np)
        # what a pure read stream over the same resident images gets on this GPU (untimed part of the job; rank 0's figure is reported)
        read_gbs = None
        if rank == 0 and args.full:
            eng.read_stream_dev(imgs.data_ptr(), n_img * IMG_BYTES, stream=stream)
            ra, rb = eng.event(), eng.event()
            eng.event_record(ra, stream)
            for _ in range(3):
                eng.read_stream_dev(imgs.data_ptr(), n_img * IMG_BYTES, stream=stream)
            eng.event_record(rb, stream)
            torch.cuda.synchronize()
            read_gbs = 3.0 * n_img * IMG_BYTES / (eng.event_elapsed_ms(ra, rb) * 1e-3) / 1e9
            eng.event_destroy(ra)
            eng.event_destroy(rb)
        hash_checksum = int(hashes.to(torch.int64).sum().item())
        if want_cpu:
            pdq_sample = hashes[:min(n_img, 30_000)].cpu().numpy()  # every image the CPU baseline hashes is compared

        # L2 -> fabric read bytes per launch: rocprofv3 cannot run inside this process, so the figure is the PMC measurement of this
        # same kernel committed under profiles/ (FETCH_SIZE, corrected as MI355X_MICROARCH.md prescribes and calibrated on the read
        # stream kernel of the same run), scaled to this launch's image count.  The counter sits on the L2's memory side and counts
        # Infinity-Cache hits too, so it can exceed what HBM itself delivered (and the rate of a pure HBM read stream).
        traffic_bytes, traffic_source = None, None
        tfile = os.path.join(ROOT, "profiles", "pdq_traffic.json")
        if os.path.exists(tfile):
            with open(tfile) as f:
                tj = json.load(f)
            per_image = tj.get({0: "generic", 1: "fused512_strip64", 2: "fused512_strip128", 3: "fused512_low_latency"}[args.pdq_kernel])
            if per_image:
                traffic_bytes = per_image * n_img
                traffic_source = tj.get("source")
        result.update({
            "value": value, "ms_per_step": elapsed / args.steps * 1e3,
            "config": {"workload": f"batch PDQ hash of {n_img} synthetic 512x512 RGB8 images per GPU, resident in HBM "
                                   "(BASELINE config 2), hash-only output",
                       "images_per_gpu": n_img, "image": "512x512x3 u8",
                       "pdq_kernel": {0: "generic", 1: "fused512/strip64", 2: "fused512/strip128", 3: "fused512/low-latency"}[args.pdq_kernel],
                       "hash_checksum": hash_checksum},
            "roofline": {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved_gbs / HBM_PEAK_GBS, "traffic": traffic_bytes, "traffic_source": traffic_source,
                         "traffic_counts": "L2->fabric read bytes (Infinity-Cache hits included)",
                         "kernel": "pdq_fused512_kernel" if args.pdq_kernel else "generic multi-pass", "kernel_ms": avg_kernel_ms,
                         "algorithmic_bytes_per_image": ALGO_BYTES_PER_IMAGE, "algorithmic_bytes_per_launch": ALGO_BYTES_PER_IMAGE * n_img,
                         "measured_read_stream_gbs": read_gbs, "frac_of_measured_read_stream": (achieved_gbs / read_gbs) if read_gbs else None,
                         "mfma_utilisation": 0.0,
                         "mfma_utilisation_note": "the bit-exact 64->16 DCT is a strictly ordered f32 mul-then-add chain (pdqhash.rs:306-336): f32 MFMA "
                                                  "accumulates in another order and fuses, so the fused 512x512 kernel issues no matrix instruction "
                                                  "(SQ_INSTS_VALU_MFMA_* = 0); the matrix pipe carries the window sums of the streaming kernel for "
                                                  "other geometries (pdq_stream.hip) and the Hamming sweep"},
        })

    # ------------------------------------------------------------------ phase C: config 4 as one timed region
    if "e2e" in phases:
        n_total = e2e_total
        n_loc = e2e_hi - e2e_lo
        e2e_imgs = imgs_all[:n_loc]
        if world > 1:  # this rank's shard of the global sequence (untimed; the images are resident when the timed region starts)
            eng.synth_images_dev(e2e_imgs.data_ptr(), e2e_lo, n_loc, 512, 512, stream=stream)
            torch.cuda.synchronize()
        e2e_steps = max(1, args.e2e_steps)
        timings = {}
        groups, info = D.hash_and_group_device(eng, e2e_imgs, n_total, args.threshold, dist, variants=True)  # warm-up (allocations, RCCL channels)
        barrier_sync()
        t0 = time.perf_counter()
        for _ in range(e2e_steps):
            groups, info = D.hash_and_group_device(eng, e2e_imgs, n_total, args.threshold, dist, variants=True, timings=timings)
        barrier_sync()
        e2e_s = max_over_ranks(time.perf_counter() - t0) / e2e_steps
        sweep_ms_max = max_over_ranks(timings.get("sweep_ms", 0.0))
        hash_ms_max = max_over_ranks(timings.get("hash_ms", 0.0))
        gather_ms_max = max_over_ranks(timings.get("allgather_ms", 0.0))
        if world > 1:  # phase A's images back (the CPU baseline and the checksums refer to them; N > 1 runs no CPU baseline, but keep the state simple)
            eng.synth_images_dev(imgs.data_ptr(), first_k, n_img, 512, 512, stream=stream)
            torch.cuda.synchronize()
        if rank == 0:
            # image k of the global sequence with k % 1000 == 999 shares its block colours with image k - 1
            want_pairs = [[k - 1, k] for k in range(999, n_total, 1000)]
            gset = {tuple(g) for g in groups}
            missing = [p for p in want_pairs if tuple(p) not in gset]
            ok = not missing and len(groups) == len(want_pairs)
            if not ok:
                valid = False
                problems.append(f"e2e: {len(groups)} groups, {len(missing)} of {len(want_pairs)} near-duplicate pairs missing")
            result["e2e"] = {
                "workload": f"{n_total} synthetic 512x512 RGB8 images resident in HBM ({n_loc} on rank 0) -> PDQ hash + quality + 8 dihedral hashes -> "
                            "all-gather of the per-file hash blocks -> variant sweep (group_files_generic rule) -> edges to rank 0 -> union-find "
                            "(BASELINE config 4" + (": 1 000 000 images" if n_total == 1_000_000 else f" at {n_total} images") + ")",
                "is_baseline_config_4_size": n_total == 1_000_000, "scaling": "strong (total fixed)" if world > 1 else "one GPU",
                "seconds_per_run": e2e_s, "images_per_s": n_total / e2e_s, "runs": e2e_steps, "similarity": args.threshold,
                "groups": len(groups), "near_duplicate_pairs_expected": len(want_pairs), "near_duplicate_pairs_found": len(want_pairs) - len(missing),
                "comparison_count": info["edges_total"], "ranks_in_collective": info["ranks_in_collective"],
                "hash_and_exchange_s_rank0": timings.get("hash_and_exchange_s"), "hash_ms_max_over_ranks": hash_ms_max,
                "allgather_ms_max_over_ranks": gather_ms_max, "sweep_ms_max_over_ranks": sweep_ms_max,
                "allgather_bytes_per_rank": n_loc * 257, "all_pairs_evaluated": n_total * (n_total - 1) // 2 * 8,
                "exchange": ("RCCL all-gather of 8 x 32 B per file + 1 B flags" if args.backend == "nccl" else "gloo all-gather (host staged)") if world > 1 else "none (1 GPU)",
                "valid": ok}

    img_sample_dev = imgs  # kept for the CPU baseline (same images)

    # ------------------------------------------------------------------ phase B: Hamming sweeps
    all_h = None

    def hamming_leg(n_h, h_steps, scaling, workload):
        """all-pairs sweep over n_h synthetic hashes living sharded over the ranks: shard generator -> one all-gather -> every rank sweeps
        part = rank of nparts = world of the block pairs.  Returns (result dict, ok, the gathered hashes)."""
        shard = n_h // world
        n_clusters = min(1000, max(0, n_h // 5 - 1))
        hs = torch.empty((n_h, 32), dtype=torch.uint8, device=dev)
        mine = hs[rank * shard:(rank + 1) * shard]
        cap = 1 << 20
        d_edges = torch.empty((cap, 12), dtype=torch.uint8, device=dev)
        d_count = torch.zeros(1, dtype=torch.int64, device=dev)
        gather_ev = []

        def hamming_step(timed=False):
            # exchange step: every rank contributes its shard of hashes (in a real scan: the hashes it just computed)
            eng.synth_hashes_dev(mine.data_ptr(), rank * shard, shard, n_h, n_clusters=n_clusters, stream=stream)
            if dist is not None:
                if timed:
                    ea, eb = eng.event(), eng.event()
                    eng.event_record(ea, stream)
                if args.backend == "nccl":
                    dist.all_gather_into_tensor(hs, mine)  # the one exchange step of the path: RCCL all-gather of hash shards
                else:
                    host = torch.empty((n_h, 32), dtype=torch.uint8)
                    dist.all_gather_into_tensor(host, mine.cpu())
                    hs.copy_(host)
                if timed:
                    eng.event_record(eb, stream)
                    gather_ev.append((ea, eb))
            d_count.zero_()
            eng.hamming_all_pairs_dev(hs.data_ptr(), n_h, args.threshold, d_edges.data_ptr(), cap, d_count.data_ptr(),
                                      part=rank, nparts=world, stream=stream)

        for _ in range(max(1, min(args.warmup, 1))):
            hamming_step()
        hev = [(eng.event(), eng.event()) for _ in range(h_steps)]
        barrier_sync()
        t0 = time.perf_counter()
        for s in range(h_steps):
            eng.event_record(hev[s][0], stream)
            hamming_step(timed=True)
            eng.event_record(hev[s][1], stream)
        barrier_sync()
        h_elapsed = max_over_ranks(time.perf_counter() - t0)
        h_step_ms = sum(eng.event_elapsed_ms(a, b) for a, b in hev) / h_steps
        gather_ms = (sum(eng.event_elapsed_ms(a, b) for a, b in gather_ev) / len(gather_ev)) if gather_ev else 0.0
        h_kernel_ms = h_step_ms - gather_ms  # the sweep (+ the shard generator, ~0.01 ms) without the exchange
        sweep_ms_max = max_over_ranks(h_kernel_ms)
        gather_ms_max = max_over_ranks(gather_ms)
        n_pairs = n_h * (n_h - 1) // 2
        gpairs = n_pairs * h_steps / h_elapsed / 1e9
        n_edges_local = int(d_count.item())
        n_edges = sum_over_ranks(n_edges_local)
        expected_edges = n_clusters * 10 + (1 if n_h >= 10 else 0)
        h_ok = n_edges_local <= cap and (args.threshold != 32 or n_edges == expected_edges)
        pw = eng.L.rph_hamming_prefix_dwords(args.threshold, args.hamming_kernel)  # prefix dwords the fast path examines
        pairs_per_s_rank = (n_pairs / world) / (h_kernel_ms * 1e-3)
        hbm = {"hbm_bytes_per_pair": HAMMING_HBM_BYTES_PER_PAIR,
               "achieved_hbm_gbs": pairs_per_s_rank * HAMMING_HBM_BYTES_PER_PAIR / 1e9,
               "achieved_hbm_frac_of_peak": pairs_per_s_rank * HAMMING_HBM_BYTES_PER_PAIR / 1e9 / HBM_PEAK_GBS,
               "hbm_note": "algorithmic tile bytes (64/T B per pair, T = 1024) / sweep time: far below peak by design -- the tiles are "
                           "reused from LDS/registers; the binding roof is the matrix pipe"}
        if args.hamming_kernel >= 2:
            # fp4 MFMA fast path: one v_mfma_scale_f32_32x32x64_f8f6f4 (131 072 fp4 ops) per 64-bit slice of 1024 pairs -> 64 * PW ops per pair,
            # against the dense fp4 peak (2 x the fp8 / int8 peak)
            h_roof = {"bound": "mfma", "achieved": pairs_per_s_rank * 64 * pw / 1e12, "peak": 2 * MFMA_I8_OPS_PER_S / 1e12, "unit": "TOP/s (fp4)",
                      "frac": pairs_per_s_rank * 64 * pw / (2 * MFMA_I8_OPS_PER_S), "int8_equivalent_ops_per_pair": 64 * pw, "prefix_dwords": pw,
                      "kernel_ms": h_kernel_ms,
                      "kernel": "hamming_mfma_kernel<FmtFp4ZO> (popcount-sorted {0,1} operands)" if args.hamming_kernel == 2 and n_h >= 32768 else "hamming_mfma_kernel<FmtFp4> (+-1 operands)",
                      "note": "power-limited, not pipe-limited: the in-kernel clock under this MFMA load is 1.8-2.0 GHz (tools/sweep_loop.hip), "
                              "the peak above is priced at 2.4 GHz"}
        elif args.hamming_kernel == 1:
            # int8 MFMA fast path: one v_mfma_i32_32x32x32_i8 (65 536 int8 ops) per 32-bit slice of 1024 pairs -> 64 * PW ops per pair
            h_roof = {"bound": "mfma", "achieved": pairs_per_s_rank * 64 * pw / 1e12, "peak": MFMA_I8_OPS_PER_S / 1e12,
                      "unit": "TOP/s (int8)", "frac": pairs_per_s_rank * 64 * pw / MFMA_I8_OPS_PER_S, "prefix_dwords": pw,
                      "int8_ops_per_pair": 64 * pw, "kernel_ms": h_kernel_ms, "kernel": "hamming_mfma_kernel<FmtI8>"}
        else:
            lane_ops = 2 * pw * pairs_per_s_rank  # executed xor + bcnt lane-ops/s on this rank
            h_roof = {"bound": "valu", "achieved": lane_ops / 1e12, "peak": VALU_LANE_OPS_PER_S / 1e12, "unit": "Tlane-op/s",
                      "frac": lane_ops / VALU_LANE_OPS_PER_S, "prefix_dwords": pw, "lane_ops_per_pair": 2 * pw,
                      "kernel_ms": h_kernel_ms, "kernel": "hamming_sweep_kernel",
                      "note": "v_bcnt_u32_b32 is a half-rate op on gfx950 (tools/valu_rate.hip): the xor+bcnt bound is 6 clk per dword per wave"}
        h_roof.update(hbm)
        out = {"metric": "hamming256_pair_comparisons_per_sec", "value": gpairs, "unit": "Gpairs/s", "workload": workload,
               "n_hashes": n_h, "threshold": args.threshold, "steps": h_steps, "ms_per_step": h_elapsed / h_steps * 1e3,
               "scaling": scaling, "edges_found": n_edges, "edges_expected": expected_edges,
               "edge_capacity": cap, "valid": h_ok, "ranks_in_collective": dist.get_world_size() if dist is not None else 1,
               "exchange": "RCCL all-gather of hash shards" if world > 1 else "none (1 GPU)",
               "allgather_ms": gather_ms, "allgather_ms_max_over_ranks": gather_ms_max, "allgather_bytes_per_rank": shard * 32,
               "sweep_ms_rank0": h_kernel_ms, "sweep_ms_max_over_ranks": sweep_ms_max,
               "roofline": h_roof}
        if not h_ok:
            out["problem"] = f"{n_edges} edges found, {expected_edges} expected (local {n_edges_local}, cap {cap})"
        return out, h_ok, hs

    if "hamming" in phases:
        n_h = int(round(args.hashes * math.sqrt(world) / (1024 * world))) * 1024 * world if args.hashes >= 1024 * world else args.hashes
        result["hamming"], h_ok, all_h = hamming_leg(n_h, args.hamming_steps or args.steps, "weak (pairs per GPU fixed: n = 1M*sqrt(N))",
                                                     f"all pairs of {n_h} synthetic 256-bit hashes, threshold {args.threshold} (BASELINE config 3 at N = 1)")
        if not h_ok:
            valid = False
            problems.append("hamming: " + result["hamming"]["problem"])
    if "hamming_10m" in phases:
        n_s = (args.hashes_strong // world) * world  # equal shards for the collective (10 000 000 divides by 1, 2, 4 and 8)
        result["hamming_10m"], s_ok, hs10 = hamming_leg(n_s, max(1, args.strong_steps), "strong (total fixed: the hashes split over the ranks)",
                                                     f"all pairs of {n_s} pre-computed 256-bit hashes over {world} GPU(s), threshold {args.threshold} (BASELINE config 5)")
        result["hamming_10m"]["is_baseline_config_5_size"] = n_s == 10_000_000
        if not s_ok:
            valid = False
            problems.append("hamming_10m: " + result["hamming_10m"]["problem"])
        del hs10
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ CPU baseline (rank 0, N = 1 only)
    if want_cpu:
        inv = cpu_inventory()
        cores = inv["threads_used"]
        if "pdq" in phases:
            # PDQ: the oracle on the first images of the same synthetic sequence (downloaded from the GPU: the generators are
            # bit-identical, tests/test_gpu_parity.py), one image per task over all cores; >= 10 000 images in chunks of 2 048
            chunk = 2048
            first = img_sample_dev[:min(chunk, n_img)].cpu().numpy().reshape(-1, 512, 512, 3)
            t_pilot, _, _ = oracle.bench_pdq(first[:cores], cores)
            per_img = max(t_pilot / cores, 1e-5)
            n_cpu = int(min(max(args.cpu_seconds / per_img, 10_000), 30_000, n_img))
            secs, done, parity = 0.0, 0, True
            while done < n_cpu:
                m = min(chunk, n_cpu - done)
                host = first[:m] if done == 0 else img_sample_dev[done:done + m].cpu().numpy().reshape(-1, 512, 512, 3)
                s, cpu_hashes, _ = oracle.bench_pdq(host, cores)
                secs += s
                if pdq_sample is not None:  # ALL hashes of the CPU sample against the GPU's, bit for bit
                    parity = parity and bool(np.array_equal(cpu_hashes[:m], pdq_sample[done:done + m]))
                done += m
            if not parity:
                valid = False
                problems.append("pdq: GPU hashes differ from the CPU oracle on the sample")
            result["cpu_baseline"] = {"value": n_cpu / secs, "unit": "hashes/s", "cores": cores, "kind": "port",
                                      "sample": f"{n_cpu} of the same synthetic 512x512 RGB8 images, C oracle, {cores} threads ({secs:.1f} s)",
                                      "host": inv, "gpu_hashes_equal_cpu_hashes_on_sample": parity, "hashes_compared": n_cpu}
        if "hamming" in phases:
            # Hamming: brute-force XOR-popcount on a 64k subset (apples to apples), and the reference's own
            # algorithm (MIH find_groups) on a timed query sample of the full 1M set
            sub = all_h[:65536].cpu().numpy()
            bsecs, _ = oracle.bench_all_pairs256(sub, args.threshold, cores)
            full = all_h.cpu().numpy()
            q_pilot = 20000
            times, _ = oracle.bench_find_groups(oracle.KIND_PDQ, full, args.threshold, cores, q_limit=q_pilot)
            q_rate = q_pilot / max(times[1], 1e-6)
            result["hamming"]["cpu_baseline"] = {
                "value": (65536 * 65535 / 2) / bsecs / 1e9, "unit": "Gpairs/s", "cores": cores, "kind": "port", "host": inv,
                "sample": "brute-force XOR-popcount over all pairs of the first 65 536 hashes",
                "mih_find_groups": {"index_build_s": times[0], "queries_per_s": q_rate,
                                    "extrapolated_s_for_all_queries": n_h / q_rate,
                                    "sample": f"MIHIndex::new on all {n_h} hashes + the first {q_pilot} queries of find_groups "
                                              f"(max_dist {args.threshold}), {cores} threads"}}
    del imgs, img_sample_dev, imgs_all
    torch.cuda.empty_cache()

    # ------------------------------------------------------------------ JPEG files -> hashes (row N3; rank 0, N = 1)
    if "jpeg" in phases and rank == 0 and world == 1:
        try:
            result["jpeg"] = jpeg_leg(eng, np, args, oracle)
            if not result["jpeg"].get("valid", True):
                valid = False
                problems.append("jpeg: " + result["jpeg"].get("problem", "results differ"))
        except ImportError as e:  # Pillow writes the test files
            result["jpeg"] = {"skipped": str(e)}

    # ------------------------------------------------------------------ the reference's own published cases (rank 0, N = 1)
    if rank == 0 and world == 1 and args.full and not args.no_reference_cases:
        result["reference_cases"] = reference_cases(eng, np)

    result["valid"] = valid
    if problems:
        result["problems"] = problems
    if rank == 0:
        print(json.dumps(result))
        sys.stdout.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()
    if not valid:
        sys.exit(1)


def dump_outputs(out_dir, hashes, rank, world, np):
    """The hashes a caller of the timed path receives, as float32 (the byte values, exact).  Beyond this rank's share of DUMP_BYTES
    the rows are a fixed seeded sample, and their row numbers go beside them as pdq_hash_rows*.npy (float64)."""
    os.makedirs(out_dir, exist_ok=True)
    h = hashes.cpu().numpy()
    suffix = "" if world == 1 else f"_rank{rank}"
    max_rows = DUMP_BYTES // world // (h.shape[1] * 4 + 8)
    if len(h) > max_rows:
        rows = np.sort(np.random.default_rng(0).choice(len(h), max_rows, replace=False))
        np.save(os.path.join(out_dir, f"pdq_hash_rows{suffix}.npy"), rows.astype(np.float64))
        h = h[rows]
    np.save(os.path.join(out_dir, f"pdq_hash{suffix}.npy"), h.astype(np.float32))


def jpeg_leg(eng, np, args, oracle):
    """Row N3: JPEG FILES in host memory -> PDQ hashes (load_image_fast + generate_pdq_features, scanner.rs:461-508, :1410), as one call.
    Files: the first 4 096 images of the synthetic sequence, JPEG-coded by Pillow (baseline, 4:2:0, quality 85: what cameras write),
    repeated to --jpeg-files.  Timed around the C call (the file pointer / length arrays are what a C caller already holds); PCIe is
    inside the timed region by definition -- the files start in host memory."""
    import io

    from PIL import Image

    from concurrent.futures import ThreadPoolExecutor

    cores = cpu_inventory()["threads_used"]
    distinct = min(args.jpeg_distinct, args.jpeg_files)

    def encode(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=85, subsampling=2)
        return buf.getvalue()

    base = []
    with ThreadPoolExecutor(max_workers=cores) as pool:  # (Pillow's encoder releases the GIL)
        for first in range(0, distinct, 256):
            base += list(pool.map(encode, eng.synth_images(first, min(256, distinct - first))))
    n = args.jpeg_files
    files = eng.jpeg_file_list([base[k % distinct] for k in range(n)])
    file_bytes = sum(len(base[k % distinct]) for k in range(n))
    out = {"files": n, "distinct_files": distinct, "file": "512x512 baseline JPEG, 4:2:0, quality 85 (Pillow / libjpeg-turbo encoder)",
           "mean_file_bytes": file_bytes / n, "flavour": "zune (parity unpinned against zune-jpeg; the libjpeg flavour is pinned against libjpeg-turbo)"}
    # entropy decoding on the device: one file per lane
    eng.jpeg_set_entropy(1)
    eng.jpeg_pdq_hash_batch(files, threads=cores)  # buffers
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        dev = eng.jpeg_pdq_hash_batch(files, threads=cores)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out["device_entropy"] = {"files_per_s": n / best, "seconds_per_call": best, "jpeg_MB_per_s": file_bytes / best / 1e6, "pixel_GB_per_s": n * IMG_BYTES / best / 1e9,
                             "pcie_bytes_per_file": file_bytes / n, "host_threads": cores,
                             "what": "host: frame headers + entropy bytes copied with the stuffing undone; device: Huffman walk (one file per lane), IDCT, upsampling, colour, PDQ"}
    # entropy decoding on the host threads (what small batches and progressive files get)
    eng.jpeg_set_entropy(0)
    m = min(n, 8000)
    sub = eng.jpeg_file_list([base[k % distinct] for k in range(m)])
    eng.jpeg_pdq_hash_batch(sub, threads=cores)
    t0 = time.perf_counter()
    host = eng.jpeg_pdq_hash_batch(sub, threads=cores)
    dt = time.perf_counter() - t0
    eng.jpeg_set_entropy(2)
    out["host_entropy"] = {"files_per_s": m / dt, "files": m, "host_threads": cores, "pcie_bytes_per_file": 6144 * 128,
                           "what": "host threads: Huffman decoding to coefficients; device: IDCT, upsampling, colour, PDQ"}
    ok = bool(dev["valid"].all() and host["valid"].all() and np.array_equal(dev["hash"][:m], host["hash"]))
    # CPU: what one host thread does with the same files -- libjpeg-turbo through Pillow (SIMD; not the reference's zune-jpeg, which cannot
    # be built here) for the decode, and the C oracle for decode + hash of the distinct files (the parity check)
    t0 = time.perf_counter()
    for f in base[:256]:
        np.asarray(Image.open(io.BytesIO(f)))
    dec = (time.perf_counter() - t0) / min(256, distinct)
    out["cpu_baseline"] = {"value": 1.0 / dec, "unit": "files/s (decode only)", "cores": 1, "kind": "third party: libjpeg-turbo via Pillow",
                           "sample": f"{min(256, distinct)} distinct files, one thread; the reference decodes with zune-jpeg 0.5.15 on every rayon worker"}
    if oracle is not None:
        for k in range(0, distinct, max(1, distinct // 16)):
            rc, coeffs, _ = oracle.pdq_features(oracle.jpeg_decode(base[k], 0))
            ok = ok and rc == 0 and bool(np.array_equal(dev["hash"][k], oracle.to_hash(coeffs)))
        out["gpu_hashes_equal_cpu_oracle_on_sample"] = ok
    # Photo-sized and progressive files (what collections hold): the reference's own bench image (tests/golden/bench.jpg, 1280x854), 64 crops
    # re-coded baseline 4:2:0 q90 without restart markers (streams cut into segments that synchronise on the device) and as progressive files
    # (one lane per file through all scans); > 512 px, so the pre-downsample and the streaming hasher follow the decode.
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "bench.jpg")
    if os.path.exists(golden) and n >= 20000:
        im = Image.open(golden)
        im.load()  # (the encoder threads below crop it: decode once, here)
        eng.jpeg_set_entropy(1)
        def photo(args_):
            kx, ky, kw_ = args_
            buf = io.BytesIO()
            im.crop((kx, ky, kx + 1265, ky + 850)).save(buf, "JPEG", quality=90, subsampling=2, **kw_)
            return buf.getvalue()

        for label, kw in (("photos_baseline", {}), ("photos_progressive", {"progressive": True})):
            nv = 64  # distinct crops: 16 horizontal x 4 vertical offsets
            with ThreadPoolExecutor(max_workers=cores) as pool:
                variants = list(pool.map(photo, [(k % 16, k // 16, kw) for k in range(nv)]))
            m_ph = 20000
            ph = eng.jpeg_file_list([variants[k % nv] for k in range(m_ph)])
            eng.jpeg_pdq_hash_batch(ph, threads=cores)
            t0 = time.perf_counter()
            got = eng.jpeg_pdq_hash_batch(ph, threads=cores)
            dt = time.perf_counter() - t0
            good = bool(got["valid"].all())
            if oracle is not None:
                for k in (3, 37):
                    rc, coeffs, _ = oracle.pdq_features(oracle.jpeg_decode(variants[k], 0))
                    good = good and rc == 0 and bool(np.array_equal(got["hash"][k], oracle.to_hash(coeffs)))
            ok = ok and good
            out[label] = {"files_per_s": m_ph / dt, "files": m_ph, "distinct_files": nv, "mean_file_bytes": sum(len(v) for v in variants) / nv,
                          "geometry": "1265x850 (crops of tests/golden/bench.jpg) -> decode -> pre-downsample on the matrix pipe -> streaming hasher",
                          "jpeg_MB_per_s": sum(len(variants[k % nv]) for k in range(m_ph)) / dt / 1e6, "pixel_GB_per_s": m_ph * 1265 * 850 * 3 / dt / 1e9,
                          "hash_equals_cpu_oracle_on_sample": good}
        eng.jpeg_set_entropy(2)
    # per-stage rooflines: rocprofv3 cannot run inside this process, so the figures are those of the same workloads profiled by
    # tools/jpeg_stage_profile.sh and committed under profiles/ (kernel time per call from the trace, algorithmic bytes from the counts)
    for cand in sorted((f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("jpeg_stage_roofline.json")), reverse=True):
        with open(os.path.join(ROOT, "profiles", cand)) as f:
            out["stage_rooflines"] = json.load(f)
        out["stage_rooflines"]["file"] = "profiles/" + cand
        break
    out["valid"] = ok
    if not ok:
        out["problem"] = "device-entropy, host-entropy and oracle hashes differ"
    return out


def reference_cases(eng, np):
    rng = np.random.default_rng(1)
    # (1) hamminghash.rs:336-412 / NOTES.txt:19: find_groups over 1M random u64 + an injected 5-cluster, max_dist 5
    h64 = rng.integers(0, 2**64, 1_000_000, dtype=np.uint64)
    target = 0xABCD_1234_5678_90EF
    for v, i in zip([target, target ^ 1, target ^ 2, target ^ 0x8000, target ^ 0x8001], rng.choice(len(h64), 5, replace=False)):
        h64[i] = v
    eng.find_groups64(h64[:4096], 5)  # warm-up
    t0 = time.perf_counter()
    g64 = eng.find_groups64(h64, 5)
    t_u64 = time.perf_counter() - t0
    # (2) README.md:13: grouping 500 000 files (PDQ, 8 dihedral variants, default similarity 40)
    nf = 500_000
    coeffs = rng.normal(0, 20, (nf, 256)).astype(np.float32)
    coeffs[1::1000] = coeffs[0::1000][: len(coeffs[1::1000])] + rng.normal(0, 0.5, (len(coeffs[1::1000]), 256)).astype(np.float32)
    fh, _ = eng.pdq_hashes_from_coeffs(coeffs, want_hash=True, want_dihedral=False)
    qual = np.full(nf, 100, np.int32)
    t0 = time.perf_counter()
    groups, cmp_count = eng.group_files_pdq(fh, 40, coeffs=coeffs, quality=qual)
    t_group = time.perf_counter() - t0
    # (3) pdqhash.rs:659-712 / NOTES.txt:41-46: bench_pdq_performance on the reference's tests/bench.jpg (1280x854):
    #     100 x generate_pdq_features one image per call, and 30 000 x generate_dihedral_hashes
    bench_jpg = None
    jpg = os.path.join(ROOT, "tests", "golden", "bench.jpg")
    try:
        from PIL import Image
        photo = np.asarray(Image.open(jpg).convert("RGB"))
    except Exception as e:  # Pillow or the fixture missing: the case is simply not reported
        photo = None
        bench_jpg = {"skipped": repr(e)}
    if photo is not None:
        from rupphash_amd import pdqhash

        eng.pdq_batcher_config(max_batch=1, max_wait_us=0)
        one = eng.pdq_hash_one(photo)
        t0 = time.perf_counter()
        for _ in range(100):
            eng.pdq_hash_one(photo)
        t_one = (time.perf_counter() - t0) / 100
        eng.pdq_batcher_config()
        many = np.repeat(one[2][None, :], 30000, axis=0)
        eng.pdq_hashes_from_coeffs(many[:64])
        t0 = time.perf_counter()
        eng.pdq_hashes_from_coeffs(many, want_hash=False, want_dihedral=True)
        t_dih = time.perf_counter() - t0
        # the per-file form the scanner calls (scanner.rs:1622): host scalar, no GPU round trip
        feats = pdqhash.PdqFeatures(one[2])
        t0 = time.perf_counter()
        for _ in range(2000):
            feats.generate_dihedral_hashes()
        t_dih_host = (time.perf_counter() - t0) / 2000
        bench_jpg = {"generate_pdq_features_ms_per_call": t_one * 1e3, "image": "1280x854 RGB8 from host memory, one image per call "
                     "(H2D of 3.3 MB, GPU luma + box pre-downsample to 512x342, PDQ, D2H), decode excluded as in the reference",
                     "reference_published_ms_per_call": 4.286,
                     "generate_dihedral_hashes_30000_s": t_dih, "reference_published_30000_s": 0.2957,
                     "generate_dihedral_hashes_host_scalar_us_per_call": t_dih_host * 1e6, "reference_published_us_per_call": 9.86,
                     "reference_source": "NOTES.txt:41-47 (one thread, unstated CPU)"}
    return {
        "bench_pdq_performance_bench_jpg": bench_jpg,
        "find_groups_1M_u64_max_dist_5": {"seconds": t_u64, "groups": len(g64), "includes": "H2D copy, all-pairs sweep, host greedy clustering",
                                          "reference_published_seconds": 12.27, "reference_source": "NOTES.txt:19 (14 threads, unstated CPU)"},
        "group_500k_files_pdq_similarity_40": {"seconds": t_group, "groups": len(groups), "comparison_count": int(cmp_count),
                                               "includes": "8 dihedral variants per file from coefficients, variant sweep, union-find",
                                               "reference_published_seconds": "15-20", "reference_source": "README.md:13 (unstated CPU)"},
    }


if __name__ == "__main__":
    main()
