#!/usr/bin/env python3
"""bench.py -- BSGS diagonal matvec throughput on MI355X (BASELINE.json metric:
"BSGS matvecs/sec at d=2048, N=16384, L0=36; sec/RWKV-block at 1/2/4/8 GPU").

One step = one full BSGS matvec exactly as the reference issues it through pyPhantom:
the G-1 = 45 baby-step rotations (bg:215-220) followed by the fused
bsgs_multiply_accumulate (bg:459: 2048 ct x pt products, 44 giant-step rotations, final
rescale), on a fresh encryption of a replicated input and D = 2048 pre-encoded diagonals
resident in HBM (SURVEY.md §8d throughput workload: limbs i.i.d. uniform mod q_i).

Multi-GPU (one process per GPU): every rank runs its own projection (8 projections of an RWKV block,
one per GPU at N=8: BASELINE configs[3]) and the output ciphertexts are gathered to rank 0 over RCCL
every step -- weak scaling, `value` = matvecs/s summed over ranks.  `--gpus N` without WORLD_SIZE in the
environment starts the N ranks itself (torch.distributed.run as a child process, before anything
touches the GPU); under torchrun WORLD_SIZE must equal --gpus.  Rank 0 limb-checks every rank's
gathered output of the last timed step against the oracle digest of that rank's workload.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the headline
(`value`, `ms_per_step`, the sorted step times); `--dump-outputs DIR` also writes the last timed step's output
limbs as DIR/*.npy (dump_outputs).  Everything below is measured only with `--full` (the instrumented
per-kernel pass, the digest checks, the sustained run, the SEAL, block and cfg5 legs, the CPU baselines).
With `--full`, `roofline` is for the kernel that the newest hash-matched rocprofv3
record of this workload (profiles/r*/rocprof_summary_<config>.json, tools/rocprof_summary.py) shows
with the longest steady-state device time per step, measured live in the timed region with HIP events
on the library stream around its launches; `cpu_baseline` times full
matvecs of the same workload with the in-repo SEAL-class CPU port (oracle/cpu_port.c, OpenMP on the
host cores this process may use); `parity` checks the output limbs against the C oracle's digest.
The measured RWKV block (`rwkv_block`) carries its own limb check at N=1: the r projection's server call
of the block, recomputed on the CPU from its recorded input limbs (`rwkv_block.parity`).
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO / "fhe-spear_amd" / "python"))
# fixed seeds throughout: the timed output is checked against the oracle's digest of the same workload,
# so encryption randomness must be the reproducible kind (fhs_host.hip parity_rng)
os.environ.setdefault("FHESPEAR_PARITY_RNG", "1")
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

CONFIGS = {
    # BASELINE configs[1]: single BSGS matvec d=2048, N=16384, L0=36 (P=3: tf default, README.md:53)
    "cfg2": dict(N=16384, L0=36, P=3, D=2048, workload="BSGS matvec d=2048 N=16384 L0=36 P=3 (89 rotations)"),
    # the same matvec in SEAL's switch_key_inplace convention (north_star's bit-exact claim): P = 1, one
    # ModUp per rotation (the default line runs it as its seal_mode leg; --config cfg2seal profiles it)
    "cfg2seal": dict(N=16384, L0=36, P=1, D=2048, mode="seal", digest="cfg2_seal",
                     workload="BSGS matvec d=2048 N=16384 L0=36 P=1, SEAL switch_key_inplace convention "
                              "(89 rotations; the 45 baby steps share one decomposition, corrected to SEAL's)"),
    # BASELINE configs[0] shape (CPU-runnable case in the reference)
    "cfg1": dict(N=8192, L0=24, P=3, D=1024, workload="BSGS matvec d=1024 N=8192 L0=24 P=3 (62 rotations)"),
    "small": dict(N=4096, L0=6, P=3, D=256, workload="BSGS matvec d=256 N=4096 L0=6 P=3 (smoke size)"),
    # BASELINE configs[4] ring (tf --N 32768 --L0 36 --P 3): one BSGS matvec of that 24-block run
    "cfg5mv": dict(N=32768, L0=36, P=3, D=2048, workload="BSGS matvec d=2048 N=32768 L0=36 P=3 (cfg5 ring)"),
    # BASELINE configs[2]/[3]: one client-aided RWKV-7 block (8 BSGS projections, bg:756-899);
    # N GPUs = the block's projections dealt over ranks (strong scaling, sec/block)
    "cfg3": dict(N=16384, L0=36, P=3, D=2048, F=8192,
                 workload="client-aided RWKV-7 block d=2048 F=8192 N=16384 L0=36 P=3: 8 BSGS projections, "
                          "pre-encoded diagonals resident in HBM"),
    # the block leg's code path at test size (tests/test_bench_legs.py)
    "block_small": dict(N=4096, L0=6, P=3, D=64, F=256, workload="client-aided RWKV-7 block d=64 F=256 N=4096 "
                                                                  "L0=6 P=3 (test size)"),
}
SK_SEED, INPUT_SEED, DIAG_SEED = 1000, 10000, 2   # tests/golden/make_bench_digest.py
# BASELINE configs[4] (tf:233-298): the FFN chain at N=32768, L0=36, P=3, d=2048, F=4096, 24 blocks as the
# reference's command runs it (README.md:53): bootstraps whenever fewer than 4 levels remain
CFG5 = dict(N=32768, L0=36, P=3, D=2048, F=4096,
            workload="fully encrypted FFN chain (tf:26-118, 233-298) d=2048 F=4096 N=32768 L0=36 P=3, bootstrap when "
                     "< 4 levels remain")
CFG5_BLOCKS = 24   # README.md:53 --num_blocks 24 (four bootstraps)
HBM_PEAK_GBS = 8000.0          # MI355X spec (MI355X_MICROARCH.md chip table)
BFLY_PEAK_GOPS = 1466.6        # measured lazy NTT butterflies/s, registers only (tools/microbench/bfly.hip)


def bsgs_params(D):
    G = int(np.ceil(np.sqrt(D)))
    return G, int(np.ceil(D / G))


def algorithmic_bytes_per_matvec(name, cfg, l):
    """Unique HBM bytes kernel `name` must move for one matvec.  Rotations of one
    input share one ModUp (hoisting): the G-1 baby rotations have one input, each of the B-1
    giant rotations its own, so a matvec runs B ModUps for its G-1 + B-1 key-switches.  SEAL's
    convention (cfg mode "seal") hoists the baby rotations too (round 5, SealHoist): their key products
    also read one correction [2][E][N] per rotation."""
    N, P, D = cfg["N"], cfg["P"], cfg["D"]
    G, B = bsgs_params(D)
    E, dn = l + P, (l + P - 1) // P
    w = 8 * N
    rot = (G - 1) + (B - 1)
    modups = 1 + (B - 1)
    corr = (G - 1) * 2 * E if cfg.get("mode") == "seal" else 0
    if name == "k_bsgs_inner":   # diagonals + baby steps in, B inner products out
        return w * (D * l + 2 * G * l + 2 * B * l)
    if name == "k_modup":        # digit limbs (coefficient form) in, extended limbs out
        return w * modups * (l + dn * E)
    if name == "k_ks_ip":        # extended limbs per distinct input + key b halves per rotation in (the a_j are
        # regenerated from their seeds, fhs_host.hip key_words), accumulators out
        return w * (modups * dn * E + rot * (dn * E + 2 * E) + corr)
    return None


def matvec_bytes(cfg, l, key_components=2):
    """SURVEY.md §8(d) algorithmic bytes of one matvec: D diagonals + (G+B-2) Galois keys at level l
    + ciphertext in and out.  key_components=1: the bytes the kernels physically read, the keys' b
    halves (the uniform a_j are regenerated from stored seeds)."""
    N, P, D = cfg["N"], cfg["P"], cfg["D"]
    G, B = bsgs_params(D)
    E, dn = l + P, (l + P - 1) // P
    return 8 * N * (D * l + (G + B - 2) * dn * key_components * E + 2 * 2 * l)


def kernel_source_hash():
    """sha256 of the kernel sources: ties a committed PMC traffic record to the kernels it measured."""
    import hashlib
    h = hashlib.sha256()
    for f in ("fhs_kernels.hip", "fhs_ntt.h", "fhs_modarith.h", "fhs_buffer.h"):
        h.update((REPO / "fhe-spear_amd" / "csrc" / f).read_bytes())
    return h.hexdigest()[:16]


def latest_traffic_record(config):
    """The newest hash-matched profiles/r*/pmc_traffic_<config>.json (tools/pmc_traffic.py); (None, None)
    when none matches (then roofline.traffic is null)."""
    return latest_record("pmc_traffic", config)


def latest_record(kind, config):
    """The newest profiles/r*/<kind>_<config>.json whose kernel-source hash matches these sources
    (tools/rocprof_summary.py, tools/pmc_valu.py write it); (None, None) when none matches."""
    want = kernel_source_hash()
    for d in sorted((REPO / "profiles").glob("r*"), reverse=True):
        f = d / f"{kind}_{config}.json"
        if f.exists():
            rec = json.loads(f.read_text())
            if rec.get("kernel_source_sha256_16") == want:
                return rec, str(f.relative_to(REPO))
    return None, None


def kernel_roofline(name, ktimes, steps, cfg, l, traffic_rec, valu_rec, rrec):
    """HBM roofline of kernel family `name` from its live HIP-event time over `steps` timed steps
    (ktimes: name -> (ms, launches)): algorithmic bytes per launch (algorithmic_bytes_per_matvec /
    launches) over the average launch duration.  traffic: HBM-side bytes per launch from the hash-matched
    rocprofv3 PMC passes of this workload (FETCH_SIZE x2 + WRITE_SIZE, tools/pmc_traffic.py), null when
    absent; valu_busy from the VALU pass (tools/pmc_valu.py); rocprof_*: the same kernel's steady-state
    time in the hash-matched rocprofv3 trace record (tools/rocprof_summary.py)."""
    traffic, tsrc = traffic_rec
    valu_k, vsrc = valu_rec
    ms, n = ktimes.get(name, (0.0, 0))
    ab = algorithmic_bytes_per_matvec(name, cfg, l)
    if not ab or not n:
        return None
    launches = max(n // steps, 1)
    ach = ab / (ms / steps * 1e-3) / 1e9
    tr = traffic.get(name) or traffic.get(name + "_h")   # half-limb variant names
    tr_step = tr["traffic_bytes_per_step"] if tr else None
    vb = valu_k.get(name) or valu_k.get(name + "_h")
    out = {"kernel": name, "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": int(tr_step / launches) if tr else None,
           "traffic_source": tsrc if tr else None,
           "traffic_over_algorithmic": round(tr_step / ab, 3) if tr else None,
           "bytes_per_launch": ab // launches, "launches_per_step": launches,
           "ms_per_step": round(ms / steps, 4), "ms_per_launch": round(ms / n, 4),
           "valu_busy": vb["valu_busy"] if vb else None, "valu_source": vsrc if vb else None}
    if rrec and name in rrec.get("kernels", {}):
        rk = rrec["kernels"][name]
        out["rocprof_ms_per_step"] = rk["ms_per_step"]
        out["rocprof_frac"] = round(ab / (rk["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    return out


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(n):
    """`bench.py --gpus N` run directly: start the N ranks (one process per GPU) with
    torch.distributed.run as a child process and exit with its status.  Nothing here has touched the
    GPU (torch is not even imported), so no process that initialised HIP is replaced."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", str(Path(__file__).resolve())] + sys.argv[1:]
    return subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1")).returncode


def limb_digest_check(config, limbs, suffix=""):
    """SHA-256 of the output limbs vs the oracle's digest of the same workload (rank 0 seeds)."""
    import hashlib
    got = hashlib.sha256(np.ascontiguousarray(limbs).tobytes()).hexdigest()
    man = json.loads((REPO / "tests" / "golden" / "manifest.json").read_text()).get("bench_digests", {})
    rec = man.get(config + suffix)
    key = f"{config}{suffix}_sha256_match"
    if rec is None:
        return {key: None, "sha256": got, "note": "no oracle digest committed for this configuration"}
    return {key: got == rec["sha256"], "sha256": got, "oracle_sha256": rec["sha256"],
            "source": "tests/golden/manifest.json bench_digests (C oracle, tests/golden/make_bench_digest.py)"}


DUMP_MAX_BYTES = 64 * 2 ** 20


def dump_outputs(dirpath, arrays):
    """--dump-outputs: every array of `arrays` as DIR/<name>.npy in float64, so that two builds run with the same
    arguments can be compared output for output.  uint64 limbs (up to 59 bits: not exact in float64) are written
    as their two 32-bit halves, <name>_lo.npy and <name>_hi.npy (value = hi * 2**32 + lo), both exact.  All
    files together stay under 64 MB: an array over its share is written as a fixed sample of its flattened
    elements (indices from numpy's default_rng(0), sorted), the same sample in every run."""
    out = Path(dirpath)
    out.mkdir(parents=True, exist_ok=True)
    files = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            files[name + "_lo"] = (a & np.uint64(0xFFFFFFFF)).astype(np.float64)
            files[name + "_hi"] = (a >> np.uint64(32)).astype(np.float64)
        else:
            files[name] = a.astype(np.float64)
    share = DUMP_MAX_BYTES // max(1, len(files)) // 8 - 16      # elements per file (the .npy header is 128 bytes)
    for name, a in files.items():
        if a.size > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share, replace=False))
            a = a.reshape(-1)[idx]
        np.save(out / f"{name}.npy", a)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def ntt_butterflies_per_matvec(cfg, l):
    """Forward-NTT butterflies in k_modup per matvec: B ModUps x (dnum (l+P) - l) limbs x N/2 log N."""
    N, P, D = cfg["N"], cfg["P"], cfg["D"]
    G, B = bsgs_params(D)
    E, dn = l + P, (l + P - 1) // P
    logn = int(np.log2(N))
    return B * (dn * E - l) * (N // 2) * logn


PHASE = ["start"]


def heartbeat(rank, local, every=45.0):
    """A progress line on stderr every `every` s from rank 0 (the GPU pool kills a command that writes nothing
    for 3 minutes; an 8-rank rehearsal sharing one GPU can spend that long in one leg)."""
    import threading

    t0 = time.time()

    def beat():
        while True:
            time.sleep(every)
            mem = ""
            try:   # device memory in use by every process on this GPU (ranks sharing one GPU in a rehearsal);
                # only once torch has initialised the device itself, and named explicitly (this thread's
                # current device is not the main thread's)
                import torch
                if not torch.cuda.is_initialized():
                    raise RuntimeError
                free, total = torch.cuda.mem_get_info(local)
                mem = f", device memory used {(total - free) / 2**30:.1f} of {total / 2**30:.0f} GiB"
            except Exception:
                pass
            print(f"bench: rank {rank} in {PHASE[0]} at {time.time() - t0:.0f} s{mem}", file=sys.stderr, flush=True)

    if rank == 0:
        threading.Thread(target=beat, daemon=True).start()


def leg_failed(rank, e):
    print(f"bench: rank {rank} leg {PHASE[0]!r} failed: {type(e).__name__}: {e}", file=sys.stderr, flush=True)


def phase(name):
    # each leg starts from the memory it needs: the previous leg's contexts (and their allocation caches) are
    # destroyed when collected, torch's cached blocks go back to the device (ranks sharing one GPU in a rehearsal)
    import gc
    gc.collect()
    if "torch" in sys.modules:
        import torch
        if torch.cuda.is_initialized():
            torch.cuda.empty_cache()
    PHASE[0] = name
    print(f"bench: {name}", file=sys.stderr, flush=True)


def gpu_clocks(pci_bus_id=None):
    """SCLK / MCLK / power / temperature of this GPU, sampled by `rocm-smi` run as a child process (nothing is
    exec'd in this process), matched to the device by PCI bus id; {"error"} when unavailable.  VERDICT r5 weak #3:
    k_bsgs_inner ran 1.80 ms on a fresh box and 2.05 ms warm; the clocks say which state a figure was taken in."""
    import subprocess
    t = time.time()
    try:
        r = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showclocks", "--showpower", "--showtemp", "--showbus", "--json"],
                           capture_output=True, text=True, timeout=30)
        data = json.loads(r.stdout[r.stdout.index("{"):])
    except Exception as e:   # reported, never hidden
        return {"error": f"{type(e).__name__}: {e}"[:200]}
    cards = {k: v for k, v in data.items() if k.startswith("card")}
    pick = None
    for k, v in cards.items():
        bus = str(v.get("PCI Bus", "")).lower()
        if pci_bus_id and bus and bus.endswith(str(pci_bus_id).lower()[-7:]):
            pick = k
    if pick is None and len(cards) == 1:
        pick = next(iter(cards))
    if pick is None:
        return {"error": f"no card matches PCI bus {pci_bus_id} among {sorted(cards)}"}
    keep = {k: v for k, v in cards[pick].items()
            if any(s in k.lower() for s in ("sclk", "mclk", "fclk", "socclk", "power", "temperature", "pci bus"))}
    keep["card"], keep["sampled_s"] = pick, round(time.time() - t, 2)
    return keep


def leg_error(fault):
    """A failed or skipped leg in the line: its fault record (every rank agreed on it, FailureFence)."""
    return dict(fault)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)   # median of 20 after 3 warmups
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg2", choices=sorted(k for k in CONFIGS if k != "block_small"))
    ap.add_argument("--full", action="store_true",
                    help="besides the headline's timed steps: the instrumented per-kernel pass and rooflines, the limb "
                         "checks against the oracle digests, the sustained run, the SEAL-convention, RWKV-block and "
                         "cfg5 legs and the CPU baselines (each with its --no-* switch below)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-reps", type=int, default=3, help="timed full CPU matvecs (after one untimed)")
    ap.add_argument("--no-block", action="store_true",
                    help="skip the measured RWKV-block leg (cfg3 on the same ranks) of the default line")
    ap.add_argument("--block-steps", type=int, default=3)
    ap.add_argument("--no-seal", action="store_true", help="skip the SEAL-convention (P = 1) matvec leg")
    ap.add_argument("--seal-steps", type=int, default=5)
    ap.add_argument("--sustain-s", type=float, default=12.0,
                    help="seconds of back-to-back matvecs after the timed steps (sustained rate, clocks; 0: skip)")
    ap.add_argument("--block-dealt", action="store_true",
                    help="block leg over N GPUs: deal each stage's projections only (default at N > 1: latency "
                         "mode, each projection's giant steps sharded over a rank group as with --split)")
    ap.add_argument("--split", action="store_true",
                    help="cfg3 over N GPUs: latency mode, giant steps of each projection sharded over a rank group")
    ap.add_argument("--no-cfg5", action="store_true", help="skip the cfg5 leg (FFN chain at N=32768 with bootstraps)")
    ap.add_argument("--cfg5-blocks", type=int, default=CFG5_BLOCKS,
                    help="FFN blocks of the cfg5 leg (BASELINE configs[4]: 24, four bootstraps)")
    args = ap.parse_args()

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:     # the driver's plain `bench.py --gpus N`: start N ranks
        sys.exit(launch_ranks(args.gpus))
    if env_world is not None and int(env_world) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world} (launch with --nproc-per-node "
              f"{args.gpus}, or run without torchrun and let --gpus start the ranks)", file=sys.stderr)
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    heartbeat(rank, local)
    os.environ.setdefault("FHESPEAR_DEVICE", str(local))
    dist = None

    def say(m):
        print(m, file=sys.stderr, flush=True)
    import fhespear_dist
    fence = fhespear_dist.LocalFence(log=say)
    # FHESPEAR_BENCH_DIST=1 under torchrun at world 1: the multi-rank step (RCCL gather to rank 0) on one
    # GPU, to time its exchange ordering where no second GPU exists
    if world > 1 or (env_world is not None and os.environ.get("FHESPEAR_BENCH_DIST") == "1"):
        import datetime
        import torch
        import torch.distributed as dist
        # a failing rank is handled by the FailureFence (store-based agreement + process-group abort), not by the
        # RCCL watchdog: no race between the two aborts (torch: _abort_process_group wants the handling off)
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")
        backend = "gloo" if os.environ.get("FHESPEAR_DIST_BACKEND", "nccl") == "gloo" else "nccl"
        if backend == "gloo":
            # rehearsal only (several ranks sharing one GPU, host-staged exchange); timings meaningless
            timeout = datetime.timedelta(seconds=int(os.environ.get("FHESPEAR_GLOO_TIMEOUT", "600")))
            local = int(os.environ.get("FHESPEAR_DEVICE", "0"))
            torch.cuda.set_device(local)
            dist.init_process_group("gloo", timeout=timeout)
        else:
            # bounded: a collective whose peer never comes fails after this (the fence usually ends it first)
            timeout = datetime.timedelta(seconds=int(os.environ.get("FHESPEAR_PG_TIMEOUT", "900")))
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local), timeout=timeout)

        def reinit(store):   # after a failed leg: a fresh default group on a new store prefix (FailureFence)
            kw = {"device_id": torch.device("cuda", local)} if backend == "nccl" else {}
            dist.init_process_group(backend, store=store, rank=rank, world_size=world, timeout=timeout, **kw)
        fence = fhespear_dist.FailureFence(dist, rank, world, log=say, reinit=reinit)

    import pyPhantom as ph

    # every data-path exchange logged per kind (RCCL broadcast / gather / reduce / reduce-scatter / send-recv:
    # calls, bytes, event-timed ms), and every rank's device gathered to rank 0
    tdist = fhespear_dist.TimedDist(dist, fence) if dist is not None else None
    ident = fhespear_dist.device_identity(ph, local)
    idents = fhespear_dist.gather_identities(dist, ident) if dist is not None else [ident]
    ranks_rec = {"world_size": dist.get_world_size() if dist is not None else 1,
                 "backend": dist.get_backend() if dist is not None else None, "devices": idents,
                 "distinct_devices": len({d.get("pci_bus_id") for d in idents}) == len(idents)}

    if args.config == "cfg3":
        return bench_block(args, ph, tdist, rank, world, local)
    cfg = CONFIGS[args.config]
    faults = {}

    def leg(name, fn, *a, **k):
        """One leg on every rank through the fence: its result (None when it failed on any rank), the fault
        recorded under `faults[name]`."""
        phase(name)
        res, fault = fence.run(name, fn, *a, **k)
        if fault is not None:
            faults[name] = fault
        return res

    mv = leg("matvec", matvec_leg, args, ph, dist, tdist, rank, world, local, ident)
    seal = None
    if args.full and world == 1 and args.config == "cfg2" and not args.no_seal:
        # north_star's bit-exact claim is stated against SEAL's switch_key_inplace convention: the same
        # matvec in that mode (P = 1, dnum = L0, the baby rotations hoisted and corrected to SEAL's lift)
        seal = leg("seal", seal_leg, args, ph, cfg)
    block = None
    if args.full and not args.no_block and args.config == "cfg2":
        # the metric's second half, measured: one client-aided RWKV-7 block (cfg3 shapes) on the same
        # ranks, after the matvec leg's memory is released
        block = leg("block", run_block, args, ph, tdist, rank, world, local, args.block_steps, 1,
                    capture=world == 1 and not args.no_cpu_baseline)
        if world > 1:
            # north_star: "baby-step rotations are computed once and broadcast" -- the FFN key pair's shared
            # baby steps in that mode too (the line above recomputes them on each owning rank)
            bb = leg("block_broadcast", run_block, args, ph, tdist, rank, world, local, args.block_steps, 1,
                     baby_mode="broadcast")
            if rank == 0 and isinstance(block, dict):
                block["baby_broadcast"] = bb if bb is not None else leg_error(faults["block_broadcast"])
    cfg5 = None
    if args.full and not args.no_cfg5 and args.config == "cfg2":
        cfg5 = leg("cfg5", run_cfg5, args, ph, tdist, rank, world, local)
    if rank == 0:
        try:
            res = build_line(args, cfg, mv, seal, block, cfg5, faults, ranks_rec, world)
        except Exception as e:   # the line is still printed (and the other ranks still released below)
            import traceback
            traceback.print_exc()
            med = (mv or {}).get("median_ms")
            res = {"metric": "BSGS matvecs/sec at d=2048,N=16384,L0=36; sec/RWKV-block at 1/2/4/8 GPU",
                   "value": round(1000.0 * world / med, 3) if med and world == 1 else None, "unit": "matvec/s",
                   "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
                   "error": f"line builder: {type(e).__name__}: {e}"[:400], "leg_faults": faults}
        print(json.dumps(res, default=str), flush=True)
    fence.finish()


def matvec_leg(args, ph, dist, tdist, rank, world, local, ident):
    """The headline leg: K timed BSGS matvecs of `args.config` (one per rank per step, outputs gathered to rank 0
    at N > 1) and, with --full, the instrumented per-kernel pass before them, the sustained sub-leg after them
    (world 1), and the limb checks.  Returns what the line needs (rank 0; the timing reductions run on every rank)."""
    cfg = CONFIGS[args.config]
    N, L0, P, D = cfg["N"], cfg["L0"], cfg["P"], cfg["D"]
    G, B = bsgs_params(D)
    steps = list(range(1, G)) + [g * G for g in range(1, B)]
    primes = ph.create_coeff_modulus(N, [59] * (L0 + P))
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_special_modulus_size(P)
    parms.set_galois_elts(sorted(set(ph.get_elts_from_steps(steps, N))))
    parms.set_coeff_modulus(primes)
    ctx = ph.context(parms, device=local)
    if cfg.get("mode") == "seal":
        ctx.set_key_switch_mode("seal")
    sk = ph.secret_key(ctx, seed=SK_SEED + rank)
    gk = sk.create_galois_keys(ctx)
    scale = 2.0 ** 59
    # input: a fresh symmetric encryption of a uniformly random plaintext (integer-exact, so the C
    # oracle reproduces it: tests/golden/make_bench_digest.py) -- the key switches and products see
    # uniformly random limbs either way
    pt_x = ph.random_plaintexts(ctx, INPUT_SEED + rank, 1, 1, scale)[0]
    ct = sk.encrypt_symmetric(ctx, pt_x)
    level = ct.chain_index()
    pts = ph.random_plaintexts(ctx, DIAG_SEED + rank, D, level, scale)
    ctx.synchronize()

    gather_buf = None
    if dist is not None:
        import torch
        out_words = 2 * (L0 - 1) * N
        gather_buf = torch.empty(out_words, dtype=torch.int64, device=f"cuda:{local}")

    gathered = [None]
    SYNC_GATHER = os.environ.get("FHESPEAR_BENCH_SYNC_GATHER") == "1"

    def step(i=None):
        if i is not None and tdist is not None:
            tdist.point(f"step{i}")
        baby = [ct] + [ph.rotate(ctx, ct, b, gk) for b in range(1, G)]
        y = ph.bsgs_multiply_accumulate(ctx, baby, pts, G, B, D, gk)
        if dist is not None:     # cfg4: output ciphertexts to rank 0 over RCCL (xGMI)
            import torch
            if dist.get_backend() == "gloo":   # rehearsal: host-staged
                ph.ciphertext_copy_to_device(ctx, y, gather_buf.data_ptr())
                gathered[0] = fhespear_dist_gather(tdist, gather_buf.cpu(), world, rank)
            elif SYNC_GATHER:   # round 1-3 ordering (A/B knob): host waits for the step, then for the gather
                torch.cuda.current_stream().synchronize()
                ph.ciphertext_copy_to_device(ctx, y, gather_buf.data_ptr())
                gathered[0] = fhespear_dist_gather(tdist, gather_buf, world, rank)
            else:
                # device-side ordering only (fhespear_dist.to_buffer): the copy waits on the library stream
                # for torch's pending work on the buffer (the previous step's gather), RCCL's gather waits for
                # the copy -- the host never blocks, so it enqueues the next step while this one runs
                import fhespear_dist
                fhespear_dist.to_buffer(ph, ctx, y, gather_buf)
                gathered[0] = fhespear_dist_gather(tdist, gather_buf, world, rank)
        return y

    phase(f"{args.config} warmup")
    for _ in range(args.warmup):
        step()
    ctx.synchronize()
    phase(f"{args.config} timed steps")

    def barrier():
        if dist is not None:
            tdist.barrier()
            import torch
            torch.cuda.synchronize()

    kprof = prof_steps = dom = dom_rule = rrec = None
    if args.full:
        # per-kernel breakdown from an instrumented, untimed pass (every kernel bracketed by HIP events)
        prof_steps = max(1, min(3, args.steps))
        ph.kernel_timer_read(ctx, reset=True)
        ph.kernel_timer_arm(ctx, None)
        for _ in range(prof_steps):
            step()
        ctx.synchronize()
        kprof = ph.kernel_timer_read(ctx, reset=True)
        # the roofline kernel, by a fixed rule: the priced kernel (one with algorithmic bytes) with the
        # longest steady-state device time per step in the newest rocprofv3 record of this workload whose
        # kernel-source hash matches these sources (tools/rocprof_summary.py); without such a record, the
        # longest priced kernel of the instrumented pass above
        rrec, rsrc = latest_record("rocprof_summary", args.config)
        priced = [k for k in kprof if kprof[k][1] and algorithmic_bytes_per_matvec(k, cfg, L0 + 1 - level)]
        if rrec and rrec.get("longest_matvec_kernel") in priced:
            dom, dom_rule = rrec["longest_matvec_kernel"], f"longest priced kernel per step in {rsrc} (rocprofv3)"
        else:
            dom = max(priced or list(kprof), key=lambda k: kprof[k][0])
            dom_rule = "longest priced kernel of this run's instrumented pass (no hash-matched rocprof record)"
        # timed region: the ModUp and Hadamard kernels (and the dominant one) carry events, measured live on
        # the context stream they launch on (each event pair costs ~10 us of queue time)
        ph.kernel_timer_arm(ctx, sorted({dom, "k_modup", "k_bsgs_inner"}))
    barrier()
    ctx.synchronize()
    if tdist is not None:
        tdist.start()
    t0 = time.perf_counter()
    evs = []
    for i in range(args.steps):
        e0 = ph.Event(ctx)
        y = step(i)
        evs.append((e0, ph.Event(ctx)))
    ctx.synchronize()
    barrier()
    t1 = time.perf_counter()
    exchange = None
    if tdist is not None:
        tdist.stop()
        exchange = tdist.summary(per=args.steps)
    # per-step device time on the library stream (HIP events; the host enqueues ahead, so these
    # bracket the GPU work of each step): the value is quoted on their median
    step_ms = sorted(a.elapsed_ms(b) for a, b in evs)
    median_ms = float(np.median(step_ms))
    del evs
    ktimes = None
    if args.full:
        ktimes = ph.kernel_timer_read(ctx, reset=True)
        ph.kernel_timer_arm(ctx, [])
    # the pinned descriptor ring's segment re-entries so far, and how many had to wait for the GPU (a wait
    # drains the queue: the r03 host stall's candidate cause, now event-gated per segment)
    staging = dict(zip(("segment_reentries", "reentries_that_waited"), ph.staging_stats(ctx)))
    elapsed = t1 - t0
    if dist is not None:
        import torch
        tt = torch.tensor([elapsed, median_ms], dtype=torch.float64, device=f"cuda:{local}")
        if dist.get_backend() == "gloo":
            tt = tt.cpu()
        tdist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed, median_ms = float(tt[0].item()), float(tt[1].item())

    # correctness guard on the timed output: the level, and on rank 0 the SHA-256 of its limbs against
    # the digest the C oracle computed for this exact workload (tests/golden/manifest.json)
    assert y.chain_index() == level + 1
    if args.dump_outputs and rank == 0:
        # what the caller of the timed path holds after its last timed step: the output ciphertext's limbs
        dump_outputs(args.dump_outputs, {"y_limbs": y.to_numpy()})
    dkey = cfg.get("digest", args.config)
    parity = limb_digest_check(dkey, y.to_numpy()) if rank == 0 and args.full else None
    if dist is not None and rank == 0 and args.full:
        # every rank's output of the last timed step, as gathered over RCCL (gloo in rehearsals), against
        # the oracle digest of that rank's workload (seeds + rank, tests/golden/make_bench_digest.py --rank)
        shape = (2, L0 - 1, N)
        per = {}
        for r, t in enumerate(gathered[0]):
            limbs = t.cpu().numpy().view(np.uint64).reshape(shape)
            per[r] = limb_digest_check(dkey, limbs, f"_rank{r}" if r else "")
        keys = [next(k for k in v if k.endswith("_match")) for v in per.values()]
        parity["gathered_outputs"] = {"ranks_checked": len(per),
                                      "all_match": all(v[k] is True for v, k in zip(per.values(), keys)),
                                      "per_rank": {r: v[k] for (r, v), k in zip(per.items(), keys)}}
    sustained = None
    if args.full and world == 1 and args.sustain_s > 0:
        phase(f"{args.config} sustained")
        sustained = sustained_run(args, ph, ctx, step, dom, cfg, L0 + 1 - level, ident, dkey)
    del pts, ct, y, gk, sk, pt_x
    ctx.synchronize()
    return {"cfg": cfg, "level": level, "primes": [int(q) for q in primes], "kprof": kprof, "prof_steps": prof_steps,
            "ktimes": ktimes, "dom": dom, "dom_rule": dom_rule, "rrec": rrec, "median_ms": median_ms,
            "elapsed": elapsed, "exchange": exchange, "staging": staging, "parity": parity, "sustained": sustained,
            "step_ms": [round(v, 4) for v in step_ms]}


def fhespear_dist_gather(tdist, buf, world, rank):
    import fhespear_dist
    return fhespear_dist.gather_to_root(tdist, buf, world, rank)


def sustained_run(args, ph, ctx, step, dom, cfg, l, ident, dkey):
    """the K-step headline is a fraction of a second on a cold box.  Back-to-back matvecs for
    `--sustain-s` seconds on the same context (keys and diagonals resident), every step bracketed by HIP events;
    the median device time of the first and of the last 20 steps, the whole run's rate, the dominant kernel's HBM
    fraction over the last 20 steps (its own events), and the GPU clocks / power / temperature sampled before and
    after.  The last output's limbs are checked against the oracle digest too."""
    clk0 = gpu_clocks(ident.get("pci_bus_id"))
    ms, evs, kt = [], [], None
    t0 = time.perf_counter()
    y = None
    while time.perf_counter() - t0 < args.sustain_s or len(ms) + len(evs) < 40:
        n = len(ms) + len(evs)
        if kt is None and time.perf_counter() - t0 >= args.sustain_s - 0.3 and n >= 20:
            ctx.synchronize()          # the last stretch: the dominant kernel carries events again
            ph.kernel_timer_read(ctx, reset=True)
            ph.kernel_timer_arm(ctx, [dom])
            kt = n
        e0 = ph.Event(ctx)
        y = step()
        evs.append((e0, ph.Event(ctx)))
        if len(evs) == 50:             # bounded queue and event count: read 50 steps at a time
            ctx.synchronize()
            ms += [a.elapsed_ms(b) for a, b in evs]
            evs = []
    ctx.synchronize()
    wall = time.perf_counter() - t0
    ms += [a.elapsed_ms(b) for a, b in evs]
    del evs
    ktimes = ph.kernel_timer_read(ctx, reset=True)
    ph.kernel_timer_arm(ctx, [])
    clk1 = gpu_clocks(ident.get("pci_bus_id"))
    first, last = float(np.median(ms[:20])), float(np.median(ms[-20:]))
    n_last = len(ms) - (kt if kt is not None else len(ms))
    roof = None
    ms_dom, n_dom = ktimes.get(dom, (0.0, 0))
    ab = algorithmic_bytes_per_matvec(dom, cfg, l)
    if n_dom and n_last and ab:
        per_step = ms_dom / n_last
        roof = {"kernel": dom, "ms_per_step": round(per_step, 4), "steps": n_last,
                "achieved": round(ab / (per_step * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                "frac": round(ab / (per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    return {"steps": len(ms), "seconds": round(wall, 2), "value": round(len(ms) / wall, 3),
            "value_basis": "steps / wall seconds of the whole back-to-back run",
            "median_ms_first20": round(first, 4), "median_ms_last20": round(last, 4),
            "value_first20": round(1000.0 / first, 3), "value_last20": round(1000.0 / last, 3),
            "roofline_last_steps": roof, "clocks_start": clk0, "clocks_end": clk1,
            "parity": limb_digest_check(dkey, y.to_numpy())}


def build_line(args, cfg, mv, seal, block, cfg5, faults, ranks_rec, world):
    """Rank 0's JSON line.  Order: the contract's fields, `roofline`, `cpu_baseline`, the detail records, and
    last a compact `summary` of every leg (the driver keeps the line's tail: VERDICT r5 weak #6)."""
    N, L0, P, D = cfg["N"], cfg["L0"], cfg["P"], cfg["D"]
    G, B = bsgs_params(D)
    res = {"metric": "BSGS matvecs/sec at d=2048,N=16384,L0=36; sec/RWKV-block at 1/2/4/8 GPU", "value": None,
           "unit": "matvec/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": None,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u64",
           "data": "synthetic (random uniform diagonals mod q_i, fresh encryption of a random uniform plaintext)",
           "config": {"workload": cfg["workload"], "N": N, "L0": L0, "P": P, "d": D, "G": G, "B": B,
                      "rotations_per_matvec": (G - 1) + (B - 1), "projections_per_rank": 1,
                      "parallelism": f"projection-parallel x{world}" + (" + RCCL gather" if world > 1 else "")}}
    l = None
    if not args.full:
        # the plain line: the headline of the timed steps alone (everything below is the --full line)
        res["full"] = False
        if mv is not None:
            median_ms, elapsed = mv["median_ms"], mv["elapsed"]
            mean_value = args.steps * world / elapsed
            res.update({"value": round(1000.0 * world / median_ms if world == 1 else mean_value, 3),
                        "ms_per_step": round(1000.0 * elapsed / args.steps, 3),
                        "median_ms_per_step": round(median_ms, 3),
                        "value_basis": ("median of the K steps' HIP-event device times" if world == 1 else
                                        "K x N matvecs / wall time of the K steps (max over ranks)"),
                        "mean_value": round(mean_value, 3), "step_ms_sorted": mv["step_ms"],
                        "staging_ring": mv["staging"], "exchange_per_step": mv["exchange"]})
        else:
            res["error"] = leg_error(faults["matvec"])
        res["ranks"] = ranks_rec
        res["leg_faults"] = faults
        return res
    res["full"] = True
    if mv is not None:
        level, kprof, prof_steps, ktimes = mv["level"], mv["kprof"], mv["prof_steps"], mv["ktimes"]
        median_ms, elapsed, dom, rrec = mv["median_ms"], mv["elapsed"], mv["dom"], mv["rrec"]
        total = args.steps * world
        mean_value = total / elapsed
        # world 1: the median step; world > 1: wall clock over the K steps (max over ranks), since
        # each step's RCCL gather runs on torch's stream outside the library-stream events
        value = 1000.0 * world / median_ms if world == 1 else mean_value
        l = L0 + 1 - level
        rows = {}
        for name, (ms, n) in kprof.items():
            if n:
                rows[name] = {"ms_per_step": round(ms / prof_steps, 3), "launches_per_step": n // prof_steps,
                              "share": round(ms / sum(v[0] for v in kprof.values()), 3)}
        trec, tsrc = latest_traffic_record(args.config)
        traffic = trec["kernels"] if trec else {}
        vrec, vsrc = latest_record("pmc_valu", args.config)
        valu_k = vrec["kernels"] if vrec else {}

        def roofline_of(name):
            return kernel_roofline(name, ktimes, args.steps, cfg, l, (traffic, tsrc), (valu_k, vsrc), rrec)

        roof = roofline_of(dom)
        sus = mv.get("sustained") or {}
        if roof is not None:
            roof["selection"] = mv["dom_rule"]
            sr = sus.get("roofline_last_steps")
            if sr and sr.get("kernel") == dom:
                roof["sustained_frac"] = sr["frac"]
                roof["sustained_ms_per_step"] = sr["ms_per_step"]
            if "rocprof_frac" in roof:
                # the profile is taken in the warm state (after the sustained run: tools/gpu.sh profile): its frac is
                # compared with the sustained one; the K-step frac is the cold-box burst
                ref = roof.get("sustained_frac", roof["frac"])
                roof["rocprof_vs_line"] = round(roof["rocprof_frac"] / ref, 4) if ref else None
                if roof["rocprof_vs_line"] is not None and abs(roof["rocprof_vs_line"] - 1) > 0.03:
                    roof["rocprof_vs_line_note"] = (
                        "outside 3 %: the Hadamard's time follows where the process's 9.66 GB diagonal slab lands in "
                        "HBM -- one process re-allocating it ran 1.75-2.02 ms at constant clocks "
                        "(profiles/r06/alloc_spread/); the record and this line are different processes")
        mu_roof = roofline_of("k_modup")
        if mu_roof is not None:
            mu_roof["note"] = ("ModUp + forward NTT is INT-VALU-bound (valu_busy: SQ_ACTIVE_INST_VALU x 4 over SIMD "
                               "cycles), so its HBM fraction is low by construction; ntt_valu_roofline prices it "
                               "against the register-only butterfly ceiling")
        had_roof = roofline_of("k_bsgs_inner")
        mu_ms = (ktimes["k_modup"][0] / args.steps if ktimes["k_modup"][1]
                 else kprof["k_modup"][0] / prof_steps)
        valu = None
        if mu_ms > 0:
            bf = ntt_butterflies_per_matvec(cfg, l)
            valu = {"kernel": "k_modup", "bound": "int-valu", "achieved": round(bf / (mu_ms * 1e-3) / 1e9, 1),
                    "peak": BFLY_PEAK_GOPS, "unit": "G butterfly/s (register-only butterfly ceiling)",
                    "frac": round(bf / (mu_ms * 1e-3) / 1e9 / BFLY_PEAK_GOPS, 4)}
        # the whole matvec as one HBM-bound unit -- diagonals + 89 non-hoisted
        # Galois keys + ciphertext in/out -- against 8 TB/s
        mv_bytes = matvec_bytes(cfg, l)
        mv_phys = matvec_bytes(cfg, l, key_components=1)
        per_gpu = value / world
        matvec_roof = {"bound": "hbm", "bytes_per_matvec": mv_bytes,
                       "achieved": round(mv_bytes * per_gpu / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": round(mv_bytes * per_gpu / 1e9 / HBM_PEAK_GBS, 4),
                       "floor_matvec_per_s": round(HBM_PEAK_GBS * 1e9 / mv_bytes, 1),
                       "bytes_read_per_matvec": mv_phys,
                       "achieved_read": round(mv_phys * per_gpu / 1e9, 1),
                       "frac_read": round(mv_phys * per_gpu / 1e9 / HBM_PEAK_GBS, 4),
                       "note": "bytes_per_matvec = SURVEY §8(d) (keys with both components); bytes_read = what the "
                               "kernels read: diagonals + the keys' b halves (a_j regenerated from seeds) + ct in/out"}
        res.update({"value": round(value, 3), "ms_per_step": round(1000.0 * elapsed / args.steps, 3),
                    "median_ms_per_step": round(median_ms, 3),
                    "value_basis": ("median of the K steps' HIP-event device times (cold-box burst; the sustained "
                                    "rate is sustained.value)" if world == 1 else
                                    "K x N matvecs / wall time of the K steps (max over ranks)"),
                    "mean_value": round(mean_value, 3), "roofline": roof})
    else:
        res["error"] = leg_error(faults["matvec"])
        res["roofline"] = None
    if world == 1 and not args.no_cpu_baseline and mv is not None:
        phase("cpu baseline")
        try:
            res["cpu_baseline"] = cpu_baseline(cfg, mv["primes"], args, cfg.get("mode", "exact"))
        except Exception as e:   # reported, never hidden
            res["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        if seal is not None and "error" not in seal:
            # the SEAL-convention leg's own CPU baseline: the same matvec in the same convention
            try:
                seal["cpu_baseline"] = cpu_baseline(CONFIGS["cfg2seal"], seal.pop("_primes"), args, "seal")
                seal["gpu_over_cpu"] = round(seal["value"] / seal["cpu_baseline"]["value"], 1)
            except Exception as e:   # reported, never hidden
                seal["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        cap = block.pop("_capture", None) if isinstance(block, dict) else None
        if cap is not None:
            try:
                block["parity"] = cpu_check_block_projection(cap)
            except Exception as e:   # reported, never hidden
                block["parity"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        cap = cfg5.pop("_capture", None) if isinstance(cfg5, dict) else None
        if cap is not None:
            try:
                cfg5["parity"]["first_bsgs"] = cpu_check_block_projection(
                    cap, "cfg5 chain block 0, key chunk 0: the chain's first BSGS call (tf:48 -> bg:459-485), "
                         "recomputed on the CPU from its recorded input limbs and diagonals")
            except Exception as e:   # reported, never hidden
                cfg5["parity"]["first_bsgs"] = {"error": f"{type(e).__name__}: {e}"[:400]}
    for rec in (block, cfg5):
        if isinstance(rec, dict):
            rec.pop("_capture", None)
    if isinstance(seal, dict):
        seal.pop("_primes", None)
    if mv is not None:
        res.update({"kernels": rows,
                    "kernels_basis": (f"instrumented untimed pass of {prof_steps} steps before the timed region, every "
                                      "kernel bracketed by HIP events (each bracket adds queue time); the roofline "
                                      "entries time their kernel inside the timed region"),
                    "modup_roofline": mu_roof, "hadamard_roofline": had_roof, "ntt_valu_roofline": valu,
                    "matvec_roofline": matvec_roof, "step_ms_sorted": mv["step_ms"],
                    "staging_ring": mv["staging"], "parity": mv["parity"], "exchange_per_step": mv["exchange"],
                    "sustained": mv.get("sustained")})
        # north_star's block as 8 independent projections, one per GPU, outputs gathered to rank 0:
        # this line's matvec leg at N ranks is exactly that (one projection per rank per step + RCCL
        # gather), so 8 projections take 8 / value seconds; the client-aided block keeps the
        # reference's stage dependencies (r,k,v -> o -> FFN key -> FFN value) and is the latency figure
        res["sec_per_8proj_independent"] = round(8.0 / res["value"], 6)
    res["ranks"] = ranks_rec
    res["seal_mode"] = seal if seal is not None else (leg_error(faults["seal"]) if "seal" in faults else None)
    res["rwkv_block"] = block if block is not None else (leg_error(faults["block"]) if "block" in faults else None)
    res["cfg5_chain"] = cfg5 if cfg5 is not None else (leg_error(faults["cfg5"]) if "cfg5" in faults else None)
    res["leg_faults"] = faults
    res["schema_errors"] = line_schema_errors(res)
    res["summary"] = line_summary(res)
    return res


def line_summary(res):
    """The compact tail of the line: every leg's headline figure and parity flag (the driver's record keeps the
    line's last ~8 KB)."""
    def g(d, *ks):
        for k in ks:
            if not isinstance(d, dict):
                return None
            d = d.get(k)
        return d
    sus, seal, blk, c5 = res.get("sustained"), res.get("seal_mode"), res.get("rwkv_block"), res.get("cfg5_chain")
    par = res.get("parity") or {}
    out = {"value": res.get("value"), "unit": res.get("unit"), "n_gpus": res.get("n_gpus"),
           "parity_match": next((v for k, v in par.items() if k.endswith("_sha256_match")), None),
           "roofline": {k: g(res, "roofline", k) for k in ("kernel", "frac", "sustained_frac", "rocprof_frac")},
           "cpu_baseline": g(res, "cpu_baseline", "value"),
           "sustained": None if not isinstance(sus, dict) else {
               k: sus.get(k) for k in ("value", "seconds", "value_first20", "value_last20")},
           "sustained_clocks": None if not isinstance(sus, dict) else {
               "start": {k: v for k, v in (sus.get("clocks_start") or {}).items() if "clk" in k.lower() or "power" in k.lower()},
               "end": {k: v for k, v in (sus.get("clocks_end") or {}).items() if "clk" in k.lower() or "power" in k.lower()}},
           "seal_mode": None if not isinstance(seal, dict) else {
               "value": seal.get("value"), "parity_match": g(seal, "parity", "cfg2_seal_sha256_match"),
               "gpu_over_cpu": seal.get("gpu_over_cpu"), "error": seal.get("error")},
           "rwkv_block": None if not isinstance(blk, dict) else {
               "sec_per_block": blk.get("sec_per_block"), "baby_mode": blk.get("baby_mode"),
               "limbs_match_cpu_port": g(blk, "parity", "r_projection_limbs_match_cpu_port"),
               "baby_broadcast_sec": g(blk, "baby_broadcast", "sec_per_block"), "error": blk.get("error")},
           "cfg5_chain": None if not isinstance(c5, dict) else {
               k: c5.get(k) for k in ("blocks", "total_seconds", "sec_per_block", "bootstraps",
                                      "bootstrap_seconds", "min_corr", "error")},
           "leg_faults": sorted(res.get("leg_faults") or {}),
           "schema_errors": res.get("schema_errors")}
    if isinstance(c5, dict):
        out["cfg5_chain"]["matches_one_rank"] = g(c5, "parity", "matches_one_rank")
        out["cfg5_chain"]["first_bsgs_limbs_match_cpu_port"] = g(c5, "parity", "first_bsgs", "limbs_match_cpu_port")
    return out


def line_schema_errors(res):
    """What the driver's N > 1 runs must carry, checked on the line itself and, by
    tests/test_cpu.py, on the committed rehearsal records: world size and one device record (with its PCI bus
    id) per rank; per-kind exchange records {calls, MB, ms}; the block leg with its baby-step mode (both modes
    at N > 1); the cfg5 leg with per-block seconds, bootstrap seconds and a digest compared with the one-rank
    digest.  A leg that failed carries {"error"} instead and is reported as such.  [] when complete."""
    err = []
    n = res.get("n_gpus")
    rk = res.get("ranks") or {}
    if rk.get("world_size") != n:
        err.append(f"ranks.world_size {rk.get('world_size')} != n_gpus {n}")
    devs = rk.get("devices") or []
    if len(devs) != n or any("pci_bus_id" not in d for d in devs):
        err.append("ranks.devices: one record with pci_bus_id per rank")

    def exchange_ok(ex, where):
        if not isinstance(ex, dict) or not all(isinstance(v, dict) and set(v) == {"calls", "MB", "ms"}
                                               for v in ex.values()):
            err.append(f"{where}: per-kind {{calls, MB, ms}}")

    if n and n > 1:
        exchange_ok(res.get("exchange_per_step"), "exchange_per_step")
    blk = res.get("rwkv_block")
    if isinstance(blk, dict) and "error" not in blk and "skipped" not in blk:
        if blk.get("baby_mode") not in ("recompute", "broadcast"):
            err.append("rwkv_block.baby_mode")
        if n and n > 1:
            exchange_ok(blk.get("exchange_per_block_rank0"), "rwkv_block.exchange_per_block_rank0")
            bb = blk.get("baby_broadcast")
            if not isinstance(bb, dict) or ("error" not in bb and "skipped" not in bb
                                            and bb.get("baby_mode") != "broadcast"):
                err.append("rwkv_block.baby_broadcast (north_star's broadcast baby steps, timed at N > 1)")
    c5 = res.get("cfg5_chain")
    if isinstance(c5, dict) and "error" not in c5 and "skipped" not in c5:
        for k in ("block_seconds", "bootstrap_seconds", "blocks", "n_gpus"):
            if k not in c5:
                err.append(f"cfg5_chain.{k}")
        if "sec_per_block" not in c5 and "sec_per_block_median" not in c5:   # round 6 / round 5 records
            err.append("cfg5_chain.sec_per_block")
        par = c5.get("parity") or {}
        if "ct_sha256" not in par or "matches_one_rank" not in par:
            err.append("cfg5_chain.parity {ct_sha256, matches_one_rank}")
        if n and n > 1:
            exchange_ok(c5.get("exchange_per_block_rank0"), "cfg5_chain.exchange_per_block_rank0")
    return err


def seal_leg(args, ph, cfg):
    """cfg2's matvec with context.set_key_switch_mode('seal'): primes [59] x (L0 + 1), one special
    prime, SEAL's switch_key_inplace limbs (DESIGN.md §4 SEAL convention; round 5: the 45 baby rotations
    share one decomposition, corrected per Galois key to SEAL's per-rotation lift -- `hoisting` counts the
    flushes taken each way).  Same seeds as the main leg; output limbs checked against the oracle's digest of
    this mode (bench_digests cfg2_seal: the oracle rotates one rotation at a time).
    One instrumented step gives the per-kernel breakdown; the roofline kernel is chosen as for the main
    leg (hash-matched rocprof_summary_cfg2seal record, else the instrumented step) and timed live with
    HIP events in the timed steps; `matvec_roofline` prices the whole matvec at SURVEY §8(d)'s bytes for
    P = 1 (diagonals + 89 keys of 36 digits x 2 x 37 limbs + ct in/out: 40.8 GB)."""
    scfg = CONFIGS["cfg2seal"]
    N, L0, D = scfg["N"], scfg["L0"], scfg["D"]
    G, B = bsgs_params(D)
    steps = list(range(1, G)) + [g * G for g in range(1, B)]
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_special_modulus_size(1)
    parms.set_galois_elts(sorted(set(ph.get_elts_from_steps(steps, N))))
    primes = ph.create_coeff_modulus(N, [59] * (L0 + 1))
    parms.set_coeff_modulus(primes)
    ctx = ph.context(parms)
    ctx.set_key_switch_mode("seal")
    sk = ph.secret_key(ctx, seed=SK_SEED)
    gk = sk.create_galois_keys(ctx)
    scale = 2.0 ** 59
    ct = sk.encrypt_symmetric(ctx, ph.random_plaintexts(ctx, INPUT_SEED, 1, 1, scale)[0])
    level = ct.chain_index()
    pts = ph.random_plaintexts(ctx, DIAG_SEED, D, level, scale)

    def step():
        baby = [ct] + [ph.rotate(ctx, ct, b, gk) for b in range(1, G)]
        return ph.bsgs_multiply_accumulate(ctx, baby, pts, G, B, D, gk)
    step()
    ctx.synchronize()
    ph.kernel_timer_read(ctx, reset=True)
    ph.kernel_timer_arm(ctx, None)
    step()
    ctx.synchronize()
    kprof = ph.kernel_timer_read(ctx, reset=True)
    l = L0 + 1 - level
    rrec, rsrc = latest_record("rocprof_summary", "cfg2seal")
    priced = [k for k in kprof if kprof[k][1] and algorithmic_bytes_per_matvec(k, scfg, l)]
    if rrec and rrec.get("longest_matvec_kernel") in priced:
        dom, rule = rrec["longest_matvec_kernel"], f"longest priced kernel per step in {rsrc} (rocprofv3)"
    else:
        dom = max(priced or list(kprof), key=lambda k: kprof[k][0])
        rule = "longest priced kernel of the leg's instrumented step (no hash-matched rocprof record)"
    ph.kernel_timer_arm(ctx, [dom])
    evs = []
    for _ in range(args.seal_steps):
        e0 = ph.Event(ctx)
        y = step()
        evs.append((e0, ph.Event(ctx)))
    ctx.synchronize()
    med = float(np.median([a.elapsed_ms(b) for a, b in evs]))
    ktimes = ph.kernel_timer_read(ctx, reset=True)
    ph.kernel_timer_arm(ctx, [])
    trec, tsrc = latest_traffic_record("cfg2seal")
    vrec, vsrc = latest_record("pmc_valu", "cfg2seal")
    roof = kernel_roofline(dom, ktimes, args.seal_steps, scfg, l, (trec["kernels"] if trec else {}, tsrc),
                           (vrec["kernels"] if vrec else {}, vsrc), rrec)
    if roof is not None:
        roof["selection"] = rule
    mvb = matvec_bytes(scfg, l)
    value = 1000.0 / med
    hoisted, fallback = ctx.seal_hoist_stats()
    res = {"value": round(value, 3), "unit": "matvec/s", "median_ms_per_step": round(med, 3),
           "steps": args.seal_steps, "P": 1, "dnum": L0,
           "hoisting": {"baby_steps": "one decomposition, per-key correction (SealHoist)" if hoisted else False,
                        "flushes_hoisted": hoisted, "flushes_fallback": fallback},
           "workload": scfg["workload"],
           "parity": limb_digest_check("cfg2", y.to_numpy(), "_seal"),
           "roofline": roof,
           "matvec_roofline": {"bound": "hbm", "bytes_per_matvec": mvb, "achieved": round(mvb * value / 1e9, 1),
                               "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(mvb * value / 1e9 / HBM_PEAK_GBS, 4),
                               "floor_matvec_per_s": round(HBM_PEAK_GBS * 1e9 / mvb, 1)},
           "kernels": {k: {"ms_per_step": round(v[0], 3), "launches_per_step": v[1]} for k, v in kprof.items() if v[1]},
           "_primes": [int(q) for q in primes]}
    del y, pts, ct, gk, sk
    ctx.synchronize()
    return res


def run_block(args, ph, dist, rank, world, local, steps, warmup, capture=False, config="cfg3", baby_mode="recompute"):
    """One client-aided RWKV-7 block (cfg3 shapes, tools/rwkv_block.py = bg:756-899) on these ranks:
    8 BSGS projections in 4 dependent stages, pre-encoded diagonals resident, stage projections
    dealt over the ranks.  Returns rank 0's {sec_per_block (median), ...} (None elsewhere).
    capture (one rank): after the timed blocks, one more block records the r projection's server
    call -- input ciphertext, output ciphertext and its 2048 diagonal plaintexts, as limbs -- for the
    CPU leg's limb check (cpu_check_block_projection), returned under "_capture"."""
    sys.path.insert(0, str(REPO / "tools"))
    import rwkv_block as rb
    cfg = CONFIGS[config]
    D, F = cfg["D"], cfg["F"]
    H = max(1, D // 64)
    rng = np.random.default_rng(5)
    blk = rb.BlockWeights(rng, 1, D, F, H)
    srv = rb.Server(ph, cfg["N"], cfg["L0"], cfg["P"], D, device=local)
    # sec/block is one token's latency: at N > 1 the stages' projections shard their giant steps over
    # rank groups unless --block-dealt
    split = getattr(args, "split", False) or (world > 1 and not getattr(args, "block_dealt", False)
                                              and args.config == "cfg2")
    run = rb.BlockRunner(srv, blk, True, dist, rank, world, split=split, baby_mode=baby_mode)
    x = rng.standard_normal(D)
    st = (x, np.zeros(D), np.zeros(D), np.zeros((H, 64, 64)), rng.standard_normal(D))

    def barrier():
        srv.ctx.synchronize()
        if dist is not None:
            import torch
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(warmup):
        out = rb.client_aided_block(run, *st)
    if hasattr(dist, "start"):
        dist.start()
    secs, stage = [], {}
    for _ in range(steps):
        barrier()
        t0 = time.perf_counter()
        out = rb.client_aided_block(run, *st)
        barrier()
        secs.append(time.perf_counter() - t0)
        for k, v in out[5].items():
            stage[k] = stage.get(k, 0.0) + v
    exchange = None
    if hasattr(dist, "start"):
        dist.stop()
        exchange = dist.summary(per=steps)
    sec = float(np.median(secs))
    if dist is not None:
        import torch
        tt = torch.tensor([sec], dtype=torch.float64, device=f"cuda:{local}")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        sec = float(tt.item())
    cap = None
    if capture and rank == 0 and world == 1:
        orig, rec = run.stage, {}

        def recording_stage(idx, ins):
            outs = orig(idx, ins)
            if idx == 0:
                rec["ct_in"], rec["ct_out"] = ins["r"][0].to_numpy(), outs["r"].to_numpy()
            return outs
        run.stage = recording_stage
        rb.client_aided_block(run, *st)
        run.stage = orig
        rec["pts"] = [p.to_numpy() for p in run.pts["r"]]
        rec.update(N=cfg["N"], L0=cfg["L0"], P=cfg["P"], D=D, sk_seed=srv.seed)
        cap = rec
    res = None
    if rank == 0:
        ref = rb.plaintext_block(blk, *st)
        err = float(np.max(np.abs(out[0] - ref[0])))
        if not err < 1e-6 * max(1.0, float(np.max(np.abs(ref[0])))):
            raise AssertionError(f"RWKV block: decrypted output off the plaintext block by {err:.3e}")
        res = {"sec_per_block": round(sec, 5), "steps": steps, "warmup": warmup,
               "sec_per_block_all": [round(v, 5) for v in secs],
               "stages_ms": {k: round(1e3 * v / steps, 2) for k, v in stage.items()},
               "server_ms": round(1e3 * sum(v for k, v in stage.items() if k.startswith("server_")) / steps, 2),
               "client_ms": round(1e3 * sum(v for k, v in stage.items() if k.startswith("client_")) / steps, 2),
               "max_abs_err_vs_plaintext_block": err,
               "workload": cfg["workload"], "n_gpus": world, "baby_mode": run.baby_mode,
               "exchange_per_block_rank0": exchange,
               "parallelism": (f"giant-step-split projections x{world}" if split
                               else f"stage-dealt projections x{world}") + (" + RCCL broadcast/gather" if world > 1 else "")}
        if cap is not None:
            res["_capture"] = cap
    del run, srv
    return res


def run_cfg5(args, ph, dist, rank, world, local):
    """BASELINE configs[4] on these ranks (tf:233-298): the fully encrypted FFN chain at N=32768, L0=36, P=3,
    d=2048, F=4096 -- `--cfg5-blocks` blocks (24 as the reference runs it, README.md:53: a bootstrap whenever
    fewer than 4 levels remain), fresh random weights per block re-encoded at the ciphertext's level as tf does
    (tf:48, 76).  Over N ranks (tools/ffn_block.py FfnRanks): each block's F/D key chunks and value chunks dealt
    to rank groups, each chunk's giant groups sharded inside its group, the bootstrap's CoeffToSlot /
    SlotToCoeff giant groups over every rank.  Reports the whole chain's seconds (blocks + bootstraps),
    sec/block = that total / blocks, every block's seconds with its chain index and its decrypted corr against
    the plaintext chain (tf:272-298 pass criterion > 0.999), every bootstrap's seconds and the block it preceded
    (device-synchronised, barrier-bracketed, max over ranks), the exchange per block, and two limb checks: the
    final ciphertext's digest against the committed one-rank digest (tests/golden/manifest.json
    gpu_chain_digests), and at one rank the chain's first BSGS call recomputed by the CPU port (_capture)."""
    sys.path.insert(0, str(REPO / "tools"))
    import ffn_block
    c = CFG5
    if hasattr(dist, "start"):
        dist.start()
    capture = world == 1 and not args.no_cpu_baseline
    r = ffn_block.chain_over_ranks(ph, c["N"], c["L0"], c["P"], c["D"], c["F"], args.cfg5_blocks, True, dist, rank,
                                   world, f"cuda:{local}", record_first=capture)
    exchange = None
    if hasattr(dist, "start"):
        dist.stop()
        exchange = dist.summary(per=max(1, len(r["block_seconds"])))
    blk = np.asarray(r["block_seconds"])
    boot = np.asarray(r["bootstrap_seconds"] or [0.0])
    if dist is not None:
        import torch
        tt = torch.tensor(np.concatenate([blk, boot]), dtype=torch.float64, device=f"cuda:{local}")
        if dist.get_backend() == "gloo":
            tt = tt.cpu()
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        v = tt.cpu().numpy()
        blk, boot = v[:len(blk)], v[len(blk):]
    if rank != 0:
        return None
    man = json.loads((REPO / "tests" / "golden" / "manifest.json").read_text()).get("gpu_chain_digests", {})
    key = f"cfg5_{args.cfg5_blocks}blk"
    want = man.get(key, {}).get("sha256")
    boots = [round(float(v), 4) for v in boot] if r["bootstrap_seconds"] else []
    total = float(np.sum(blk)) + float(np.sum(boots))
    out = {"workload": c["workload"], "n_gpus": world, "blocks": len(blk),
           "total_seconds": round(total, 4), "sec_per_block": round(total / max(1, len(blk)), 4),
           "sec_per_block_basis": "(sum of block seconds + sum of bootstrap seconds) / blocks",
           "block_only_mean": round(float(np.mean(blk)), 4),
           "block_seconds": [round(float(v), 4) for v in blk], "chain_index": r["chain_index"],
           "corr": [round(v, 8) for v in r["corr"]], "min_corr": round(min(r["corr"]), 8),
           "bootstraps": len(r["bootstrap_seconds"]), "bootstrap_seconds": boots,
           "bootstrap_before_block": r["bootstrap_before"],
           "setup_s": round(r["setup_s"], 2), "max_err_vs_plaintext": max(r["max_err"]), "exchange_per_block_rank0": exchange,
           "parallelism": (f"FfnRanks x{world}: chunks dealt to rank groups, giant groups sharded, bootstrap linear "
                           f"transforms sharded" if world > 1 else "one rank"),
           "parity": {"ct_sha256": r["ct_sha256"], "one_rank_sha256": want,
                      "matches_one_rank": (r["ct_sha256"] == want) if want else None,
                      "source": f"tests/golden/manifest.json gpu_chain_digests.{key} (one-rank GPU run of the same "
                                "seeds; the FFN encodes with the float64 GPU encoder, so the digest is the GPU's own; "
                                "first_bsgs is the oracle-side check)"}}
    fb = r.get("first_bsgs")
    if fb is not None:
        out["_capture"] = dict(fb, N=c["N"], L0=c["L0"], P=c["P"], D=c["D"], sk_seed=1)   # ffn_block.Ckks seed
    return out


def bench_block(args, ph, dist, rank, world, local):
    """cfg3 / cfg4: one step = the server side of one client-aided RWKV-7 block (tools/rwkv_block.py,
    bg:756-899): 8 BSGS projections in 4 dependent stages, each input encrypted and each output
    decrypted by rank 0 (the client), diagonals pre-encoded and resident.  N ranks deal each stage's
    projections round-robin (RCCL broadcast of the input ciphertexts, gather of the outputs)."""
    sys.path.insert(0, str(REPO / "tools"))
    import rwkv_block as rb
    cfg = CONFIGS["cfg3"]
    D, F = cfg["D"], cfg["F"]
    H = D // 64
    rng = np.random.default_rng(5)
    block = rb.BlockWeights(rng, 1, D, F, H)
    srv = rb.Server(ph, cfg["N"], cfg["L0"], cfg["P"], D, device=local)
    run = rb.BlockRunner(srv, block, True, dist, rank, world, split=args.split)
    x = rng.standard_normal(D)
    st = (x, np.zeros(D), np.zeros(D), np.zeros((H, 64, 64)), rng.standard_normal(D))

    def barrier():
        srv.ctx.synchronize()
        if dist is not None:
            import torch
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        out = rb.client_aided_block(run, *st)
    barrier()
    t0 = time.perf_counter()
    stage = {}
    for _ in range(args.steps):
        out = rb.client_aided_block(run, *st)
        for k, v in out[5].items():
            stage[k] = stage.get(k, 0.0) + v
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        import torch
        tt = torch.tensor([elapsed], dtype=torch.float64, device=f"cuda:{local}")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if rank == 0:
        ref = rb.plaintext_block(block, *st)
        err = float(np.max(np.abs(out[0] - ref[0])))
        if not err < 1e-6 * max(1.0, float(np.max(np.abs(ref[0])))):
            raise AssertionError(f"bench cfg3: decrypted block output off the plaintext block by {err:.3e}")
        if args.dump_outputs:
            # the client's decrypted results of the last timed block (tools/rwkv_block.py client_aided_block)
            dump_outputs(args.dump_outputs, dict(zip(("x", "x_ln", "x_ffn_ln", "state", "v_first"), out[:5])))
        sec = elapsed / args.steps
        l = cfg["L0"]
        mv = matvec_bytes(dict(cfg), l)
        res = {
            "metric": "BSGS matvecs/sec at d=2048,N=16384,L0=36; sec/RWKV-block at 1/2/4/8 GPU",
            "value": round(sec, 5), "unit": "s/RWKV-block", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * sec, 3), "higher_is_better": False,
            "scaling": "strong", "vs_baseline": None, "dtype": "u64",
            "data": "synthetic (random-init RWKV-7 block weights, random token state); max |x - plaintext block| "
                    f"= {err:.2e}",
            "config": {"workload": cfg["workload"], "N": cfg["N"], "L0": l, "P": cfg["P"], "d": D, "d_ffn": F,
                       "projections": 8, "parallelism": (f"giant-step-split projections x{world}" if args.split
                                                         else f"stage-dealt projections x{world}")
                       + (" + RCCL broadcast/gather" if world > 1 else "")},
            "stages_ms": {k: round(1e3 * v / args.steps, 2) for k, v in stage.items()},
            "matvec_roofline": {"bound": "hbm", "bytes_per_block": 8 * mv, "achieved": round(8 * mv / sec / 1e9, 1),
                                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(8 * mv / sec / 1e9 / HBM_PEAK_GBS, 4)},
        }
        print(json.dumps(res))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def cpu_baseline(cfg, primes, args, mode="exact"):
    """SURVEY.md §8(d)'s CPU baseline: the build's own CPU restatement with SEAL-class arithmetic
    (oracle/cpu_port.c: Harvey lazy NTT with Shoup twiddles, Barrett-reduced lazy sums, OpenMP), timed
    over FULL matvecs of this exact workload -- the G-1 baby rotations and the B-1 giant rotations
    issued one at a time (non-hoisted, as the reference's CPU path issues them), D multiply_plain+add,
    the final rescale -- on the host cores this process may use.  One untimed matvec, then
    args.cpu_reps timed; the median is reported.  Its output limbs are checked against the oracle
    digest of the workload (the same one the GPU output is checked against).
    Cores: `cores` = the OpenMP threads used = the box's CPU share (OMP_NUM_THREADS, 16 on the GPU box:
    the pool gives each GPU 16 of the node's cores, so that is what this process may use); `cores_usable`
    records the affinity mask, the cgroup quota and that share.  The same matvec is also timed on half
    the threads, and `whole_host_extrapolated` scales the per-core rate linearly to every physical core
    of the node -- an upper bound on the node's CPU throughput (memory bandwidth does not scale that way),
    so the GPU/CPU ratio against it is a lower bound.
    mode="seal": the SEAL-convention matvec (P = 1, 37 one-limb digits, SEAL's switch_key_inplace
    rounding), checked against the oracle's digest of that mode."""
    from oracle import cpu_port
    N, L0, P, D = cfg["N"], cfg["L0"], cfg["P"], cfg["D"]
    if mode == "seal":
        P = 1
    G, B = bsgs_params(D)
    assert [int(q) for q in primes] == [int(q) for q in cpu_port.create_coeff_modulus(N, [59] * (L0 + P))]
    threads = cpu_port.box_threads()
    secs, y, t_setup, threads = cpu_port.baseline(N, L0, P, D, reps=args.cpu_reps, threads=threads, sk_seed=SK_SEED,
                                                  input_seed=INPUT_SEED, diag_seed=DIAG_SEED, mode=mode)
    med = float(np.median(secs))
    half = None
    if threads >= 2:
        hs, _, _, _ = cpu_port.baseline(N, L0, P, D, reps=1, threads=threads // 2, sk_seed=SK_SEED,
                                        input_seed=INPUT_SEED, diag_seed=DIAG_SEED, mode=mode)
        half = {"threads": threads // 2, "sec_per_matvec": round(float(np.median(hs)), 4)}
    phys = physical_cores()
    res = {"value": round(1.0 / med, 5), "unit": "matvec/s", "cores": threads, "kind": "port",
           "cpu_model": cpu_model(), "host_cpus_visible": os.cpu_count(), "cores_usable": cpu_port.usable_cores(),
           "sample": f"full matvec x {len(secs)}, median (after 1 untimed): oracle/cpu_port.c, SEAL-class CPU "
                     f"restatement (Harvey NTT + Shoup, Barrett lazy sums, OpenMP over rotations/giant groups), "
                     f"{(G - 1) + (B - 1)} non-hoisted rotations + {D} multiply_plain/add + rescale at N={N}, "
                     f"L0={L0}, P={P}" + (", SEAL switch_key_inplace convention" if mode == "seal" else "")
                     + "; not TenSEAL (not importable, SURVEY §8c)",
           "sec_per_matvec": round(med, 4), "sec_per_matvec_all": [round(v, 4) for v in secs],
           "half_threads": half, "setup_s": round(t_setup, 1),
           "parity": limb_digest_check("cfg2" if args.config == "cfg2" else args.config, y,
                                       "_seal" if mode == "seal" else "")}
    if phys:
        res["whole_host_extrapolated"] = {
            "physical_cores": phys, "value": round(phys / threads / med, 4), "unit": "matvec/s",
            "basis": f"{threads}-thread rate x {phys}/{threads} (linear per-core scaling: an upper bound)"}
    return res


def physical_cores():
    """Physical cores of the host (/proc/cpuinfo: distinct (physical id, core id) pairs), None if unknown."""
    try:
        pairs, pid = set(), None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pid = line.split(":")[1].strip()
            elif line.startswith("core id"):
                pairs.add((pid, line.split(":")[1].strip()))
        return len(pairs) or None
    except OSError:
        return None


def cpu_check_block_projection(cap, check=None):
    """Limb check of the block leg: the r projection's server call recorded in the
    measured block (its GPU-encoded input ciphertext and diagonals) recomputed by the CPU port with the
    oracle's Galois keys for the block's secret-key seed -- the reference loop bg:464-485 one rotation at
    a time -- must give the GPU's output limbs exactly.  (The block's inputs come from the float64 GPU
    encoder, so no digest can be committed ahead of time as for the matvec leg.)"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import cpu_port
    from oracle.oracle import Oracle, galois_elt
    N, L0, P, D, seed = cap["N"], cap["L0"], cap["P"], cap["D"], cap["sk_seed"]
    G, B = bsgs_params(D)
    t0 = time.perf_counter()
    primes = [int(q) for q in cpu_port.create_coeff_modulus(N, [59] * (L0 + P))]
    o = Oracle(N, primes, P)
    s = o.gen_secret(seed)
    threads = cpu_port.box_threads()
    with ThreadPoolExecutor(threads) as ex:
        bk = dict(zip(range(1, G), ex.map(lambda b: o.gen_galois_key(seed, s, galois_elt(b, N)), range(1, G))))
        gk = dict(zip(range(1, B), ex.map(lambda g: o.gen_galois_key(seed, s, galois_elt(g * G, N)), range(1, B))))
    y = cpu_port.CpuPort(N, primes, P, threads).matvec(cap["ct_in"], bk, gk, cap["pts"], G, B, D)
    ok = bool(np.array_equal(y, cap["ct_out"]))
    out = {"limbs_match_cpu_port": ok, "sha256": cpu_port.sha256(cap["ct_out"]), "cpu_port_sha256": cpu_port.sha256(y),
           "check": (check or "r projection's server call (bg:545-659 real D->D) of the measured block, recomputed "
                              "on the CPU (oracle/cpu_port.c, keys from the C oracle) from the recorded input limbs")
           + f"; N={N}, L0={L0}, P={P}, D={D}",
           "seconds": round(time.perf_counter() - t0, 1)}
    if check is None:
        out["r_projection_limbs_match_cpu_port"] = ok
    return out


if __name__ == "__main__":
    main()
