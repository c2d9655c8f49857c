#!/usr/bin/env python3
"""Throughput benchmark of the north-star path: per-clip forward of TCE-RVOS on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1:  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

A "step" = one B=1 clip forward on every rank: Swin-T backbone, T=5 frames of 360x640, a 32-token text
(RoBERTa-base, random init, evaluated every step as the reference does), FTF/IQT deformable transformer,
cross-modal FPN, dynamic mask head -- BASELINE.json config 2 -- followed (N > 1) by the caller harness kernel
(best query, resize, sigmoid, threshold) and the RCCL all-gather of the per-clip uint8 masks.  Clips are independent
units sharded over ranks (weak scaling, no data-path collective besides the gather).  Inputs and weights are
synthetic and already resident in HBM when the timed region starts.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the steps and prints the headline fields (`value`,
`ms_per_step`, ...).  --dump-outputs DIR writes the arrays the last timed step returned as DIR/<name>.npy (float32; fixed,
seeded samples of the largest ones past 64 MB in all); inputs and weights are seeded, so two builds compare output for output.
--full adds the passes below (each of them runs after the timed region):
  roofline          : the kernel that carries the most algorithmic FLOPs of a step -- its FLOPs / its summed launch
                      durations, measured live with events on the launch stream in a second, instrumented (eager) pass
                      (the headline `value` comes from the un-instrumented pass).  `traffic` is NOT measured by this
                      run: it is read from the committed PMC summary named in `traffic_source` (or null).
  roofline_hbm      : the dominant HBM-side kernel (the encoder's multi-scale deformable attention call): SURVEY 8d's
                      algorithmic bytes / its launch duration (same instrumented pass) against the 8 TB/s HBM peak.
  cpu_baseline      : the CPU oracle (a port of the reference path) timed on this box's host cores, rank 0, N=1 only:
                      3 timed forwards at min(32, all) threads (`samples`), and one single-thread forward of ONE frame of
                      the same clip scaled to the clip (`one_thread`).
  value_c2/value_c4 : clips/s with 2 / 4 independent B=1 forwards in flight per GPU (one stream + replay slot each): the
                      per-GPU shape of BASELINE config 4 (8 clips per GPU).  The headline `value` is one clip at a time.
  value_f32_exact   : clips/s of the same step with every GEMM on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32) instead
                      of the 3 x fp16 split (N=1 only, short pass).
  value_text_cached : clips/s with the per-expression text cache on (RoBERTa evaluated once per distinct caption
                      instead of every clip like the reference; N=1 only, short pass).
  parity            : the masks of one step against the CPU oracle's on the same clip and weights (with cpu_baseline).
  value_group8      : N > 1 only: clips/s with 8 clips per forward as one launch program, gather included.
  group_first_clip_vs_b1_max_rel_err : N > 1 with --group G only: the group's first clip against its own B=1 forward.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRIC = "clips/s (T=5, 360×640, Swin-T) at 1/2/4/8 MI355X; mask IoU vs ref"
PMC_SUMMARY = os.path.join("profiles", "r05_pmc_traffic.json")
PMC_FALLBACK = os.path.join("profiles", "r04_pmc_traffic.json")
LATENCY_SUMMARY = os.path.join("profiles", "r05_latency_bound.json")


def _pmc_traffic(kernel_prefix):
    """HBM bytes per launch of `kernel_prefix` from the committed PMC summary (separate rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE passes of this same command, aggregated by tools/pmc_traffic.py).  (None, None) when absent."""
    for summary in (PMC_SUMMARY, PMC_FALLBACK):
        try:
            with open(os.path.join(ROOT, summary)) as f:
                k = json.load(f)["kernels"]
            hits = [v for name, v in k.items() if name.startswith(kernel_prefix)]
            if hits:  # several instantiations share a prefix: the one that moved the most bytes over the pass
                hit = max(hits, key=lambda v: v["hbm_bytes_per_launch"] * v.get("launches", 1))
                return round(hit["hbm_bytes_per_launch"]), summary + " (rocprofv3 --pmc passes, not this run)"
        except Exception:  # noqa: BLE001
            pass
    return None, None


def _latency_summary(cfg_name):
    """How latency-bound the clip is: launches per clip, how many are shorter than 15 us and what they sum
    to, the share of the clip during which exactly one kernel is in flight.  NOT measured by this run: read from the
    committed summary of a rocprofv3 --kernel-trace of this same command (tools/latency_summary.py), labelled so."""
    try:
        with open(os.path.join(ROOT, LATENCY_SUMMARY)) as f:
            d = json.load(f)
        ent = d.get(cfg_name)
        if ent:
            return dict(ent, source=LATENCY_SUMMARY + " (rocprofv3 --kernel-trace of this command, not this run)")
    except Exception:  # noqa: BLE001
        pass
    return None


DUMP_BUDGET = 64 << 20  # bytes written by --dump-outputs, all files together


def _dump_outputs(out_dir, outs):
    """Writes every tensor of the last step's output dicts (`aux_outputs` and the like flattened into the name) as
    out_dir/<name>.npy in float32 (float64 for integer tensors).  Past DUMP_BUDGET, the largest arrays are replaced, largest
    first, by 2^20 of their flattened elements at fixed seeded positions (out_dir/<name>_sample.npy), so a dump of the same
    arguments always holds the same elements."""
    import numpy as np
    import torch
    arrays = []

    def walk(prefix, v):
        if torch.is_tensor(v):
            arrays.append((prefix, v))
        elif isinstance(v, dict):
            for k in sorted(v):
                walk(f"{prefix}_{k}" if prefix else str(k), v[k])
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{prefix}_{i}", x)

    for j, o in enumerate(outs):
        walk("" if len(outs) == 1 else f"clip{j}", o)
    host = []
    for name, t in arrays:
        t = t.detach().cpu()
        host.append((name, t.double() if not (t.is_floating_point() or t.is_complex()) else t.float()))
    total = sum(t.numel() * t.element_size() for _, t in host)
    sample = set()
    for name, t in sorted(host, key=lambda nt: -nt[1].numel() * nt[1].element_size()):
        if total <= DUMP_BUDGET:
            break
        sample.add(name)
        total -= t.numel() * t.element_size()
        total += (1 << 20) * t.element_size()
    os.makedirs(out_dir, exist_ok=True)
    for name, t in host:
        a = t.numpy()
        if name in sample:
            g = torch.Generator().manual_seed(0)
            idx = torch.randperm(a.size, generator=g)[:1 << 20].sort().values.numpy()
            np.save(os.path.join(out_dir, name + "_sample.npy"), a.reshape(-1)[idx])
        else:
            np.save(os.path.join(out_dir, name + ".npy"), a)


def _ensure_built(local_rank, world):
    """Fresh checkout: the shared object is git-ignored.  Runs BEFORE any GPU / RCCL call (the compiler children must
    not be spawned from a process that has initialised the GPU); local rank 0 builds (the linker output is renamed
    into place atomically, tce_rvos_amd/build.py), the other ranks wait for the file."""
    from tce_rvos_amd import build as _b
    if os.path.exists(_b.LIB):
        return
    if local_rank == 0:
        _b.build(verbose=False)
    else:
        t0 = time.time()
        while not os.path.exists(_b.LIB):
            if time.time() - t0 > 1800:
                raise SystemExit("bench.py: timed out waiting for local rank 0 to build libtce_rvos.so")
            time.sleep(1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=250, help="timed steps (default: ~2.3 s of timed region at config 2)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--backbone", default="swin_t_p4w7")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the roofline, variant, CPU-baseline / parity and N > 1 group passes")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-variants", action="store_true", help="skip the value_f32_exact / value_text_cached passes")
    ap.add_argument("--gemm-mode", default="f16x3", choices=["f32", "f16x3", "f16"],
                    help="f16x3 (default): fp32-accurate 3 x fp16 split; f32: exact fp32 MFMA; f16: one fp16 MFMA per product (config 5)")
    ap.add_argument("--arith-policy", default="uniform",  # validated against model.ARITH_POLICIES after _ensure_built()
                    help="per-site arithmetic (tce_rvos_amd.model.ARITH_POLICIES): 'uniform' = --gemm-mode everywhere; "
                         "'cfg5_mixed' = single-pass fp16 in the site groups the committed sensitivity table allows")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo (+ TCE_BENCH_ONE_DEVICE=1: every rank on cuda:0) rehearses the N>1 control flow on a 1-GPU box")
    ap.add_argument("--clips-in-flight", type=int, default=1,
                    help="independent B=1 clip forwards kept in flight per GPU and per step (one stream + replay slot each)")
    ap.add_argument("--ranks-per-gpu", type=int, default=1,
                    help="processes sharing one GPU (rank r runs on cuda:(LOCAL_RANK // R)): each process has its own HIP "
                         "hardware queues, which one process's graph replays do not (DESIGN.md section 6)")
    ap.add_argument("--group", type=int, default=1,
                    help="clips per forward as ONE launch program (model.forward_group): independent clips, block-diagonal across "
                         "clips, each clip's result = its B=1 forward's; the latency-bound stages are shared by the group")
    ap.add_argument("--same-clip", action="store_true",
                    help="with --group G: the G forwards of a group are G captions on ONE clip (the expressions of a video): the "
                         "backbone runs once per group; `value` then counts (clip, expression) pairs per second")
    ap.add_argument("--no-gather", action="store_true",
                    help="N > 1 without the per-step mask all-gather (barrier + max-over-ranks timing only): isolates the "
                         "compute side of a ranks-per-GPU measurement from gloo's host-side copies")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world == 1 and args.gpus > 1:
        raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run --nproc-per-node N")
    _ensure_built(local_rank, world)
    # the pool's driver only supports dmabuf IPC: without this RCCL's buffer exchange fails (hipIpcGetMemHandle)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import torch
    import torch.distributed as dist

    if os.environ.get("TCE_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    local_rank //= max(1, args.ranks_per_gpu)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # TCE_BENCH_FORCE_DIST=1: a world of ONE still initialises the process group and sends every step's masks through the
    # collective (RCCL's all_gather_into_tensor on device tensors, the barrier, the max-over-ranks all_reduce): the N > 1 code
    # path executed on a one-GPU box.  Ranks sharing a GPU cannot use RCCL (one communicator per device): they meet over gloo.
    force_dist = os.environ.get("TCE_BENCH_FORCE_DIST") == "1"
    dist_on = world > 1 or force_dist
    if args.ranks_per_gpu > 1 and args.backend == "nccl" and world > 1:
        raise SystemExit("--ranks-per-gpu > 1 needs --backend gloo (RCCL allows one rank per device in a communicator)")
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    from tce_rvos_amd import build_model, ops
    from tce_rvos_amd.dist import gather_clip_masks_async
    if os.environ.get("TCE_GEMM_TILE_RULES") == "r4":  # A/B aid (tools/runs/): tile selection by the previous round's rules
        from tce_rvos_amd._lib import lib as _l
        _l().tce_gemm_force_tile(-1)
    if os.environ.get("TCE_CONV3_FORM"):  # A/B aid: 4 / 8 = one form of the 3x3 convolution everywhere (no mixed launches)
        from tce_rvos_amd._lib import lib as _l
        _l().tce_debug_conv3x3_set_waves(int(os.environ["TCE_CONV3_FORM"]))
    if os.environ.get("TCE_FFN_HALF"):  # A/B aid: -1 = the C <= 128 fused MLP never as half workgroups, 1 = always
        from tce_rvos_amd._lib import lib as _l
        _l().tce_debug_ffn_set_half(int(os.environ["TCE_FFN_HALF"]))
    from tce_rvos_amd.model import ARITH_POLICIES
    if args.arith_policy not in ARITH_POLICIES:
        raise SystemExit(f"--arith-policy: unknown policy {args.arith_policy!r}; choose from {sorted(ARITH_POLICIES)}")

    margs = argparse.Namespace(backbone=args.backbone, with_box_refine=True, binary=True, freeze_text_encoder=True,
                               f_token=8, qtrans=True, num_feature_levels=4)
    model, _, _ = build_model(margs)
    ops.set_gemm_mode(args.gemm_mode)  # before the weights are packed: packed streams carry the mode's rounding
    model = model.to(dev).eval()
    if args.arith_policy != "uniform":
        model.set_arith_policy(args.arith_policy)
    C = max(1, args.clips_in_flight)
    if C > 1 and not model.use_graph:
        raise SystemExit("--clips-in-flight > 1 needs graph replay (TCE_GRAPH=1): eager launches share one stream per slot")

    T, H, W = args.frames, args.height, args.width
    g = torch.Generator().manual_seed(1234 + rank)
    n_pool = 4
    clips = [torch.randn(T, 3, H, W, generator=g).to(dev) for _ in range(n_pool)]
    ids_host = torch.randint(3, 50264, (n_pool, 1, args.tokens), generator=g)
    ids_host[:, :, 0], ids_host[:, :, -1] = 0, 2
    ids = ids_host.to(dev)
    targets = [{"size": torch.tensor([H, W])}]
    gather_buf, pending = None, None
    last_local = [None]  # this rank's masks of the last gathered step (the forced world-1 run checks the collective's result)
    last_outs = [None]  # the per-clip output dicts of the last step (--dump-outputs)
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(C, 4))]
    use_host_ids = False  # the text-cache pass keys the cache on host ids

    Gp = max(1, args.group)
    ids_groups = [torch.cat([ids[(k + j) % n_pool] for j in range(Gp)], 0) for k in range(n_pool)] if Gp > 1 else None

    def one(i, slot=0):
        """the forward(s) of one unit of a step: a list of per-clip output dicts (Gp of them for a clip group)"""
        if Gp > 1:
            k = (i * Gp) % n_pool
            if args.same_clip:
                return model.forward_group([clips[k]] * Gp, ids_groups[k], targets, slot=slot)
            return model.forward_group([clips[(k + j) % n_pool] for j in range(Gp)], ids_groups[k], targets, slot=slot)
        tok = ids_host[i % n_pool] if use_host_ids else ids[i % n_pool]
        return [model([clips[i % n_pool]], tok, targets, slot=slot)]

    def step(i, gather=True):
        nonlocal gather_buf, pending
        if C == 1:
            outs = one(i)
        else:  # C independent forwards in flight, one per stream / replay slot
            cur = torch.cuda.current_stream()
            outs = []
            for c in range(C):
                streams[c].wait_stream(cur)
                with torch.cuda.stream(streams[c]):
                    outs.extend(one(i * C + c, slot=c))
            for c in range(C):
                cur.wait_stream(streams[c])
        if dist_on and gather and not args.no_gather:
            # what meets on every rank is what the callers keep: the harness's uint8 masks (inference_ytvos.py:238-250
            # on the GPU), 4x fewer bytes than the fp32 logits.  The collective of step i runs on RCCL's stream while
            # step i+1 computes, and is completed (stream-ordered) before step i+1's own gather starts.
            local = torch.stack([ops.select_masks(o["pred_logits"][0], o["pred_masks"][0], (H, W))[0] for o in outs], 0)
            if pending is not None:
                gather_buf = pending.wait()
            pending = gather_clip_masks_async(local if args.backend == "nccl" else local.cpu(), world * C * Gp, force=force_dist)
            last_local[0] = local
        last_outs[0] = outs
        return outs[0]

    def fence():
        nonlocal gather_buf, pending
        if pending is not None:  # the last step's masks must have met inside the timed region
            gather_buf = pending.wait()
            pending = None
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(n_steps, n_warm, gather=True):
        for i in range(n_warm):
            step(i, gather)
        fence()
        t0 = time.perf_counter()
        for i in range(n_steps):
            step(i, gather)
        fence()
        return time.perf_counter() - t0

    elapsed = timed(args.steps, args.warmup)
    if args.dump_outputs and rank == 0:  # before any later pass reuses the replayed graph's output buffers
        _dump_outputs(args.dump_outputs, last_outs[0])
    collective = None
    if dist_on and not args.no_gather:
        # the last step's gathered masks must hold this rank's block at this rank's place (checked on every rank)
        lo = rank * C * Gp
        ok = gather_buf is not None and bool((gather_buf[lo:lo + C * Gp].to(last_local[0].device) == last_local[0]).all())
        collective = {"backend": dist.get_backend(), "world": world, "forced_world1": bool(force_dist and world == 1),
                      "bytes_per_rank_per_step": int(last_local[0].numel() * last_local[0].element_size()),
                      "gathered_shape": list(gather_buf.shape), "own_block_matches": ok}
        if not ok:
            raise SystemExit(f"bench.py: rank {rank}: the gathered masks do not hold this rank's block")
    if dist_on:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    ops.check_range(dev)  # split-fp16 range guard: a tripped flag invalidates the number

    def max_over_ranks(sec):
        if not dist_on:
            return sec
        t = torch.tensor([sec], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    dist_variants = {}
    if args.full and dist_on and Gp > 1 and rank == 0:
        # BASELINE config 4's per-rank shape is a clip GROUP (64 clips over 8 GPUs = 8 per rank): the first clip of rank 0's group
        # must be what its own B = 1 forward gives (forward_group's contract; another kernel route at the group's row count is
        # allowed: 2e-5 of the tensor's range)
        k0 = 0
        grp = model.forward_group([clips[(k0 + j) % n_pool] for j in range(Gp)], ids_groups[k0], targets)
        solo_out = model([clips[k0 % n_pool]], ids[k0 % n_pool], targets)
        torch.cuda.synchronize()
        rel = {k: float((grp[0][k] - solo_out[k]).abs().max() / solo_out[k].abs().max().clamp_min(1e-30))
               for k in ("pred_logits", "pred_boxes", "pred_masks")}
        dist_variants["group_first_clip_vs_b1_max_rel_err"] = rel
        if max(rel.values()) > 2e-5:
            raise SystemExit(f"bench.py: the group's first clip differs from its B = 1 forward: {rel}")
    if args.full and dist_on and world > 1 and Gp == 1 and C == 1 and model.use_graph and args.gemm_mode != "f32" and not args.no_variants:
        # N > 1 lines also carry the rate at config 4's per-rank shape (8 clips per rank as ONE launch program), gather included;
        # every rank runs it (the step holds the collective)
        Gp = 8
        ids_groups = [torch.cat([ids[(k + j) % n_pool] for j in range(Gp)], 0) for k in range(n_pool)]
        n_var = max(6, min(args.steps, 30))
        t_g8 = max_over_ranks(timed(n_var, 3))
        dist_variants["value_group8"] = round(n_var * world * Gp / t_g8, 3)
        Gp = 1

    roofline, roofline_hbm = None, None
    C_saved, C = C, 1  # the instrumented pass, the variants and the parity check run one clip at a time
    Gp_saved, Gp = Gp, 1
    solo = rank == 0 and world == 1 and not force_dist
    if args.full and rank == 0 and not args.no_roofline:
        n_inst = min(args.steps, 40)
        graph_mode, model.use_graph = model.use_graph, False  # per-launch events need eager launches
        step(0, gather=False)  # rank-0-only passes must not enter the collective
        ops.GEMM_PROFILE, ops.HBM_PROFILE = [], []
        for i in range(n_inst):
            step(i, gather=False)
        torch.cuda.synchronize()
        prof, ops.GEMM_PROFILE = ops.GEMM_PROFILE, None
        hprof, ops.HBM_PROFILE = ops.HBM_PROFILE, None
        model.use_graph = graph_mode
        agg = {}
        for tile, conv, flops, e0, e1 in prof:
            a = agg.setdefault((tile, conv), [0.0, 0.0, 0])
            a[0] += flops
            a[1] += e0.elapsed_time(e1) * 1e-3
            a[2] += 1
        key = max(agg, key=lambda k: agg[k][0])  # the kernel instance that carries the most algorithmic FLOPs
        fl, sec, n = agg[key]
        mode = ops.get_gemm_mode()
        # f32: v_mfma_f32_32x32x2_f32 (157.3 TFLOP/s).  f16x3: three v_mfma_f32_32x32x16_f16 per algorithmic product
        # (dense fp16 peak 2500 TFLOP/s): `achieved` stays ALGORITHMIC 2*M*N*K, the MFMA pipe issues 3x that.
        peak = 157.3 if mode == "f32" else 2500.0
        passes = {"f32": 1, "f16x3": 3, "f16": 1}[mode]
        ach = fl / sec / 1e12
        if isinstance(key[0], str):
            kname = key[0]
        else:
            tname = {256128: "256, 128", 128128: "128, 128", 12864: "128, 64", 6464: "64, 64", 6465: "64, 64"}[key[0]]
            kname = ("gemm_f32_kernel" if mode == "f32" else "gemm_f16x3_kernel") + f"<{tname}" + (" conv>" if key[1] else ">")
        traffic, tsrc = _pmc_traffic(kname.split(" conv")[0].rstrip(">"))
        roofline = {"bound": "mfma", "kernel": kname, "gemm_mode": mode,
                    "mfma_issued_tflops": round(ach * passes, 2),
                    "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                    # what a bare loop of this MFMA + an LDS fragment feed sustains with all 256 CUs issuing: the chip
                    # lowers its clock under matrix load; informative, `peak` stays the guide's
                    "sustained_mfma_ceiling_tflops": None if mode == "f32" else 1650.0,
                    "traffic": traffic, "traffic_source": tsrc,
                    "launches_per_step": n // n_inst, "avg_launch_us": round(sec / n * 1e6, 2),
                    "flops_per_launch_avg": fl / n, "instrumented_steps": n_inst,
                    # an EAGER, instrumented, serialised sum over every matrix-core launch (events around each launch on one
                    # stream): it can exceed ms_per_step, where the same launches overlap in the replayed graph's branches
                    "all_mfma_kernels_ms_per_step": round(sum(v[1] for v in agg.values()) / n_inst * 1e3, 3),
                    "all_mfma_kernels_note": "eager serial sum of instrumented launches; not comparable with ms_per_step (graph branches overlap)",
                    "all_mfma_kernels_tflops": round(sum(v[0] for v in agg.values()) / sum(v[1] for v in agg.values()) / 1e12, 2)}

        # the matrix-core kernel that carries the most TIME (not FLOPs): on the larger configurations it is another one
        tkey = max(agg, key=lambda k: agg[k][1])
        tfl, tsec, tn = agg[tkey]
        if isinstance(tkey[0], str):
            tname = tkey[0]
        else:
            tname = ("gemm_f32_kernel" if mode == "f32" else "gemm_f16x3_kernel") + "<" + \
                {256128: "256, 128", 128128: "128, 128", 12864: "128, 64", 6464: "64, 64", 6465: "64, 64"}[tkey[0]] + (" conv>" if tkey[1] else ">")
        roofline["top_time_kernel"] = {"kernel": tname, "ms_per_step": round(tsec / n_inst * 1e3, 3), "launches_per_step": tn // n_inst,
                                       "avg_launch_us": round(tsec / tn * 1e6, 2), "achieved": round(tfl / tsec / 1e12, 2),
                                       "frac": round(tfl / tsec / 1e12 / peak, 4),
                                       "share_of_mfma_time": round(tsec / sum(v[1] for v in agg.values()), 3)}

        # HBM side: the encoder's MSDA calls (the launches with the most query rows)
        mprof = [h for h in hprof if h[0] == "msda_fused_q4u_kernel"]
        if mprof:
            rows_max = max(h[1] for h in mprof)
            enc = [h for h in mprof if h[1] == rows_max]
            hb = sum(h[2] for h in enc)
            hs = sum(h[3].elapsed_time(h[4]) for h in enc) * 1e-3
            htraffic, hsrc = _pmc_traffic("msda_fused_q4")
            roofline_hbm = {"bound": "hbm", "kernel": "msda_fused_q4u_kernel<4> (encoder self-attention call)",
                            "achieved": round(hb / hs / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                            "frac": round(hb / hs / 8e12, 4), "traffic": htraffic, "traffic_source": hsrc,
                            "launches_per_step": len(enc) // n_inst, "avg_launch_us": round(hs / len(enc) * 1e6, 2),
                            "bytes_per_launch": hb / len(enc),
                            "note": "gathers 1.58 GB of bilinear corner rows per launch through the CUs' vector L1s (not algorithmic bytes)"}
            # the other HBM-bound kernels that report their algorithmic bytes: largest launch of each kind
            others = {}
            for name in sorted(set(h[0] for h in hprof) - {"msda_fused_q4u_kernel"}):
                rows_k = max(h[1] for h in hprof if h[0] == name)
                sel = [h for h in hprof if h[0] == name and h[1] == rows_k]
                kb = sum(h[2] for h in sel)
                ks = sum(h[3].elapsed_time(h[4]) for h in sel) * 1e-3
                others[name] = {"rows": rows_k, "launches_per_step": len(sel) // n_inst, "avg_launch_us": round(ks / len(sel) * 1e6, 2),
                                "achieved_GBps": round(kb / ks / 1e9, 1), "frac_of_8TBps": round(kb / ks / 8e12, 4)}
            roofline_hbm["other_hbm_bound_kernels"] = others

    variants = {}
    exact_masks, product_err = None, {}
    if args.full and solo and not args.no_variants:
        n_var = max(10, min(args.steps, 60))
        if model.use_graph and C_saved == 1:
            for cc in (2, 4):
                C = cc
                variants[f"value_c{cc}"] = round(n_var * cc / timed(n_var, 4, gather=False), 3)
            C = 1
        if model.use_graph and C_saved == 1 and Gp_saved == 1 and args.gemm_mode != "f32":
            # clip groups (model.forward_group): G independent clips as ONE launch program, each clip's result its B = 1 forward's
            for gg in (2, 4, 8):
                Gp = gg
                ids_groups = [torch.cat([ids[(k + j) % n_pool] for j in range(Gp)], 0) for k in range(n_pool)]
                variants[f"value_group{gg}"] = round(n_var * gg / timed(n_var, 4, gather=False), 3)
            Gp = 1
        model.text_cache_size, use_host_ids = 8, True
        variants["value_text_cached"] = round(n_var / timed(n_var, 6, gather=False), 3)
        model.text_cache_size, use_host_ids = 0, False
        if args.gemm_mode != "f32":
            ops.set_gemm_mode("f32")
            model.repack()  # captured graphs hold the split-mode kernels
            variants["value_f32_exact"] = round(n_var / timed(n_var, 6, gather=False), 3)
            exact_masks = step(0, gather=False)["pred_masks"].cpu()  # the exact-fp32 pass's own result, for the parity leg
            ops.set_gemm_mode(args.gemm_mode)
            model.repack()
            # per-product error of both arithmetics, measured here: one 512 x 512 x 1024 GEMM with four decades of dynamic range
            # along K against fp64, as max |c - ref| / sum_k |a||b|  (tests/test_kernels_gpu.py::test_gemm_split_fp16_is_fp32_accurate)
            gq = torch.Generator().manual_seed(11)
            qa = torch.randn(512, 1024, generator=gq) * torch.logspace(-2, 2, 1024)[None, :]
            qw = torch.randn(512, 1024, generator=gq) / 32.0
            qref, qscale = qa.double() @ qw.double().T, qa.double().abs() @ qw.double().abs().T
            for qm in ("f32", args.gemm_mode):
                ops.set_gemm_mode(qm)
                qo = ops.gemm(qa.to(dev), qw.to(dev)).cpu().double()
                product_err[qm] = float(((qo - qref).abs() / qscale).max())
            ops.set_gemm_mode(args.gemm_mode)

    cpu_baseline, parity = None, None
    if args.full and solo and not args.no_cpu_baseline:
        from oracle import tce_oracle as O
        cores = min(32, os.cpu_count() or 1)  # oneDNN/MKL scale poorly past ~32 threads on this graph
        torch.set_num_threads(cores)
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith("text_encoder.")}
        frames_cpu = clips[0].cpu()
        with torch.no_grad():
            hid, pooled = model.forward_text_encoder(ids[0], dev)
            hid, pooled = hid.cpu(), pooled.cpu()
            from tce_rvos_amd.config import BACKBONES
            bb = BACKBONES[args.backbone]
            cfg = O.OracleConfig(backbone=args.backbone, **{k: bb[k] for k in ("embed_dim", "depths", "num_heads") if k in bb})
            times = []
            for _ in range(4):  # one warm-up + 3 timed forwards
                t1 = time.perf_counter()
                ref = O.forward(sd, cfg, frames_cpu, hid, pooled, img_size=(H, W))
                times.append(time.perf_counter() - t1)
            times = times[1:]
            med = sorted(times)[1]
            # single thread: ONE frame of the same clip (bounded sample), scaled to the clip's T frames
            torch.set_num_threads(1)
            t1 = time.perf_counter()
            O.forward(sd, cfg, frames_cpu[:1], hid, pooled, img_size=(H, W))
            t_one = (time.perf_counter() - t1) * T
            torch.set_num_threads(cores)
        cpu_baseline = {"value": round(1.0 / med, 4), "unit": "clips/s", "cores": cores, "kind": "port",
                        "samples": [round(1.0 / t, 4) for t in times],
                        "sample": f"1 clip (T={T}, {H}x{W}, {args.tokens} tokens) per sample, median of 3 timed oracle forwards "
                                  f"after one warm-up ({med:.2f} s); text encoder excluded",
                        "one_thread": {"value": round(1.0 / t_one, 5), "cores": 1,
                                       "sample": f"one forward of 1 of the clip's {T} frames on 1 thread, time x {T} "
                                                 f"({t_one:.1f} s per clip)"}}
        out = step(0, gather=False)
        torch.cuda.synchronize()
        pm = out["pred_masks"].cpu()
        err = float((pm - ref["pred_masks"]).abs().max())
        iou = O.mask_iou(pm > 0, ref["pred_masks"] > 0)
        parity = {"mask_iou_vs_oracle": round(iou, 6), "criterion": "1 - IoU <= 1e-3", "criterion_met": bool(iou >= 1 - 1e-3),
                  "max_abs_logit_err": err, "max_rel_logit_err": err / float(ref["pred_masks"].abs().max()),
                  # pixels where a sign flip is numerically meaningless
                  "frac_pixels_abs_logit_lt_1e-3": float((ref["pred_masks"].abs() < 1e-3).float().mean())}
        if exact_masks is not None:  # the exact-fp32 pass (every product on v_mfma_f32_32x32x2_f32) against the same oracle output
            e_err = float((exact_masks - ref["pred_masks"]).abs().max())
            parity["f32_exact"] = {"mask_iou_vs_oracle": round(O.mask_iou(exact_masks > 0, ref["pred_masks"] > 0), 6),
                                   "max_abs_logit_err": e_err, "max_rel_logit_err": e_err / float(ref["pred_masks"].abs().max())}

    if parity is not None and not parity["criterion_met"]:
        print(f"bench.py: PARITY FAILURE: mask IoU vs the oracle {parity['mask_iou_vs_oracle']} misses the 1e-3 criterion in this "
              f"arithmetic ({args.gemm_mode}, policy {args.arith_policy}): the throughput below is NOT a valid result", file=sys.stderr)
    C, Gp = C_saved, Gp_saved
    if rank == 0:
        known = {("resnet50", 1, 360, 640): "BASELINE config 1", ("swin_t_p4w7", 5, 360, 640): "BASELINE config 2",
                 ("video_swin_t_p4w7", 8, 384, 640): "BASELINE config 3", ("swin_b_p4w7", 10, 480, 854): "BASELINE config 5"}
        cfg_name = known.get((args.backbone, T, H, W), "not a BASELINE config")
        metric = METRIC if cfg_name == "BASELINE config 2" else \
            f"clips/s (T={T}, {H}×{W}, {args.backbone}; {cfg_name}) at {world} MI355X; mask IoU vs ref"
        clips_total = args.steps * world * C * Gp
        line = {"metric": metric, "value": round(clips_total / elapsed, 3), "unit": "clips/s", "n_gpus": (world + args.ranks_per_gpu - 1) // args.ranks_per_gpu,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                "timed_region_s": round(elapsed, 3),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": {"f32": "f32", "f16x3": "f32 (3xf16-split MFMA, f32 accumulate)",
                          "f16": "f16 (operands rounded to fp16, one MFMA per product, f32 accumulate)"}[args.gemm_mode] +
                         ("" if not model.arith_policy else "; single-pass f16 MFMA in site groups " +
                          ",".join(sorted(g for g, m in model.arith_policy.items() if m == "f16"))),
                "data": "synthetic",
                "config": {"workload": f"{args.backbone} T={T} {H}x{W} + {args.tokens}-token text, B=1 clip per forward, "
                                       f"flags --with_box_refine --binary --f_token 8 --qtrans ({cfg_name})",
                           "clips_per_step": world * C * Gp, "clips_in_flight_per_gpu": C, "clips_per_forward": Gp, "same_clip_in_group": bool(args.same_clip and Gp > 1),
                           "ranks_per_gpu": args.ranks_per_gpu,
                           "parallelism": f"clip-sharded x{world}" +
                                          ((" + harness kernel + " + ("RCCL" if args.backend == "nccl" else "gloo") +
                                            " all_gather(uint8 masks)") if dist_on else "")},
                "collective": collective,
                "launch": "hipGraph replay" if model.use_graph else "eager",
                "graphs": model.graph_state(),
                "valid": None if parity is None else parity["criterion_met"],
                "latency_bound": _latency_summary(cfg_name),
                "roofline": roofline, "roofline_hbm": roofline_hbm, "cpu_baseline": cpu_baseline, "parity": parity}
        if roofline is not None and "value_f32_exact" in variants:
            # The precision story in one place.  The headline arithmetic is NOT the reference's fp32 FMA chain: it is
            # fp32-CLASS (each operand = two RTZ fp16 halves, three fp16 MFMAs per product, lo*lo dropped, fp32 accumulate).
            # What that costs per product and end to end is measured by this run, next to the same clip on the exact fp32 MFMA.
            ex = variants["value_f32_exact"]
            flop_per_clip = 1.19e12  # SURVEY 8d (config 2; other configurations: not restated, frac fields omitted)
            prec = {"headline_arithmetic": args.gemm_mode, "value": line["value"], "value_f32_exact": ex,
                    "ms_per_step_f32_exact": round(1e3 / ex, 3),
                    "per_product_err_over_sum_abs": {k: float(f"{v:.3e}") for k, v in product_err.items()},
                    "per_product_err_ratio_vs_f32": (round(product_err[args.gemm_mode] / product_err["f32"], 2)
                                                     if product_err.get("f32") else None),
                    "max_rel_logit_err": None if parity is None else {args.gemm_mode: parity["max_rel_logit_err"],
                                                                      "f32": parity.get("f32_exact", {}).get("max_rel_logit_err")},
                    "note": "f32 pass: every matrix product on v_mfma_f32_32x32x2_f32 (bit-exact fp32 FMA chains), tiled GEMM "
                            "kernels only (the fused FFN / cross-attention / Swin / convolution kernels exist in the split arithmetic)"}
            if cfg_name == "BASELINE config 2":
                prec["whole_clip_tflops"] = {args.gemm_mode: round(flop_per_clip / (elapsed / clips_total) / 1e12, 1),
                                             "f32": round(flop_per_clip * ex / 1e12, 1)}
                n_pass = {"f32": 1, "f16x3": 3, "f16": 1}[args.gemm_mode]  # MFMAs issued per algorithmic product
                prec["whole_clip_frac"] = {"of_fp16_dense_2500_issued": round(n_pass * flop_per_clip / (elapsed / clips_total) / 2.5e15, 4),
                                           "of_fp16_dense_2500_algorithmic": round(flop_per_clip / (elapsed / clips_total) / 2.5e15, 4),
                                           "f32_exact_of_fp32_matrix_157.3": round(flop_per_clip * ex / 157.3e12, 4)}
            roofline["precision"] = prec
        line.update(variants)
        line.update(dist_variants)
        print(json.dumps(line), flush=True)
    if dist_on:
        dist.barrier()  # rank 0's extra (collective-free) passes are done: leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
